// transform_host_main.hip - a program of its own (host code only, linked against the library for the layout functions) that
// runs what evc_online_transform (csrc/evc_transform_plan.h) and evc_online_learn_fresh (csrc/evc_online_plan.h) decide on the
// host and prints it: tests/test_minibatch_host.py
// builds it, once plainly and once under the address and undefined-behaviour sanitizers, and checks the lines.
//   carve <M R T n_utt esize> shift <s> : <byte offsets of chg and of the activation half> bytes <b> query <q>
//                          carve_transform from an aligned and a misaligned base
//   args <case> <status>   transform_args_check over a grid of bad and good arguments
//   slots <max_iter> <n>   transform_slots
//   fcarve <M R T bs esize> shift <s> : <byte offsets of the learner's workspace, chg and the final solve's> bytes <b> query <q>
//   fargs <case> <status> [fresh <n> final <n> slots <n> batch_size <n>]    online_fresh_args_check
#include "../exemplars_vc_amd/csrc/evc_online_plan.h"
#include "../exemplars_vc_amd/csrc/evc_transform_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace evc;

static void carve_line(int M, int R, int T_, int n_utt, int dtype, size_t shift) {
    std::vector<char> mem(4096);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~uintptr_t(255)) + shift;
    const TrWs w = carve_transform(base, M, R, T_, n_utt, dtype);        // addresses only: nothing is dereferenced
    const char* arr[] = {(const char*)w.chg, w.beta_ws};
    printf("carve %d %d %d %d %d shift %zu :", M, R, T_, n_utt, dtype == EVC_F64 ? 8 : 4, shift);
    long prev = -1;
    for (const char* a : arr) {
        const long off = (long)(a - base);
        if (off <= prev || (reinterpret_cast<uintptr_t>(a) & 255) != 0) {
            printf(" BAD");
            exit(3);
        }
        prev = off;
        printf(" %ld", off);
    }
    const size_t need = transform_workspace_bytes(M, R, T_, n_utt, dtype);
    const size_t chg_bytes = (size_t)frame_tile_cap(T_, BT_F, n_utt) * BT_F * 2 * sizeof(double);
    if (w.bytes > need || (size_t)prev + w.beta_bytes > w.bytes || (size_t)(w.beta_ws - (const char*)w.chg) < chg_bytes) {
        printf(" BAD SIZE");
        exit(4);
    }
    printf(" bytes %zu query %zu\n", w.bytes, need);
}

static void args_lines() {
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
    auto opts = [] {
        evc_transform_opts o{};
        o.struct_bytes = (int)sizeof(o);
        o.dtype = EVC_F64; o.layout = EVC_FRAME_MAJOR; o.max_iter = 200; o.init_mode = EVC_INIT_SKLEARN;
        o.beta = 0.5; o.tol = 1e-4;
        return o;
    };
    const int offs_ok[] = {0, 30, 30, 70}, offs_bad[] = {0, 40, 30, 70};
    auto run = [&](const char* name, const evc_transform_opts& o, int M, int R, int T, size_t ws, const int* offs = nullptr,
                   int n_utt = 1, bool with_x = true) {
        const int st = transform_args_check(p, M, with_x ? p : nullptr, M, p, R, M, R, T, offs, n_utt, &o, p, ws);
        printf("args %s %d\n", name, st);
    };
    const size_t big = size_t(1) << 40;
    run("ok", opts(), 25, 17, 70, big);
    run("ok_exact", opts(), 25, 17, 70, transform_workspace_bytes(25, 17, 70, 1, EVC_F64));
    run("short_by_one", opts(), 25, 17, 70, transform_workspace_bytes(25, 17, 70, 1, EVC_F64) - 1);
    run("ok_utts", opts(), 25, 17, 70, big, offs_ok, 3);
    run("bad_utts", opts(), 25, 17, 70, big, offs_bad, 3);
    run("no_frames_no_x", opts(), 25, 17, 0, big, nullptr, 1, false);
    run("frames_no_x", opts(), 25, 17, 70, big, nullptr, 1, false);
    { auto o = opts(); o.struct_bytes = 4; run("struct_bytes", o, 25, 17, 70, big); }
    { auto o = opts(); o.max_iter = -1; run("max_iter_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.max_iter = 0; run("max_iter_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.max_iter = BETA_MAX_SLOTS; run("max_iter_4097", o, 25, 17, 70, big); }
    { auto o = opts(); o.max_iter = BETA_MAX_SLOTS + 1; run("max_iter_4098", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 1; run("reserved", o, 25, 17, 70, big); }
    { auto o = opts(); o.init_mode = 3; run("init_mode", o, 25, 17, 70, big); }
    { auto o = opts(); o.beta = __builtin_inf(); run("beta_inf", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = -1e-9; run("tol_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = 0.0; run("tol_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.l2 = __builtin_nan(""); run("l2_nan", o, 25, 17, 70, big); }
    { auto o = opts(); o.init_value = __builtin_inf(); run("init_value_inf", o, 25, 17, 70, big); }
    run("M_528", opts(), 528, 17, 70, big);
    run("M_529", opts(), 529, 17, 70, big);
    run("M_529_small_ws", opts(), 529, 17, 70, 16);
    run("R_100000", opts(), 25, 100000, 70, big);
    { auto o = opts(); o.beta = __builtin_nan(""); run("nan_before_limits", o, 529, 17, 70, 16); }
}

static void fcarve_line(int M, int R, int T_, int batch, int dtype, size_t shift) {
    std::vector<char> mem(4096);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~uintptr_t(255)) + shift;
    const FreshWs w = carve_fresh(base, M, R, T_, batch, dtype);        // addresses only: nothing is dereferenced
    const char* arr[] = {w.online_ws, (const char*)w.chg, w.final_ws};
    printf("fcarve %d %d %d %d %d shift %zu :", M, R, T_, batch, dtype == EVC_F64 ? 8 : 4, shift);
    long prev = -1;
    for (const char* a : arr) {
        const long off = (long)(a - base);
        if (off <= prev || (reinterpret_cast<uintptr_t>(a) & 255) != 0) {
            printf(" BAD");
            exit(5);
        }
        prev = off;
        printf(" %ld", off);
    }
    const size_t need = online_fresh_workspace_bytes(M, R, T_, batch, dtype);
    const int bs = batch < T_ ? batch : T_, nb = (T_ + bs - 1) / bs;
    const size_t chg_bytes = (size_t)frame_tile_cap(T_, BT_F, nb) * BT_F * 2 * sizeof(double);
    if (w.bytes > need || (size_t)prev + w.final_bytes > w.bytes || (size_t)(w.final_ws - (const char*)w.chg) < chg_bytes ||
        (size_t)((const char*)w.chg - w.online_ws) < w.online_bytes || w.online_bytes != online_workspace_bytes(M, R, T_, batch, dtype)) {
        printf(" BAD SIZE");
        exit(6);
    }
    printf(" bytes %zu query %zu\n", w.bytes, need);
}

static void fargs_lines() {
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
    auto opts = [] {
        evc_online_fresh_opts o{};
        o.struct_bytes = (int)sizeof(o);
        o.dtype = EVC_F64; o.layout = EVC_FRAME_MAJOR; o.batch_size = 32; o.max_iter = 5; o.max_no_improvement = 10;
        o.fresh_max_iter = 30; o.final_max_iter = 200;
        o.beta = 0.5; o.tol = 1e-4; o.forget_factor = 0.7;
        return o;
    };
    auto run = [&](const char* name, const evc_online_fresh_opts& o, int M, int R, int T, size_t ws) {
        evc_online_opts oo{};
        FreshPlan plan{0, 0};
        int forced = -1;
        bool fused = false;
        const int st = online_fresh_args_check(p, M, p, M, p, R, p, p, M, M, R, T, &o, p, ws, &oo, &plan, &forced, &fused);
        printf("fargs %s %d", name, st);
        if (st == 0) printf(" fresh %d final %d slots %d batch_size %d fused %d", plan.fresh_max_iter, plan.final_max_iter,
                            plan.slots(), oo.batch_size, fused ? 1 : 0);
        printf("\n");
    };
    const size_t big = size_t(1) << 40;
    run("ok", opts(), 25, 17, 70, big);
    run("ok_exact", opts(), 25, 17, 70, online_fresh_workspace_bytes(25, 17, 70, 32, EVC_F64));
    run("short_by_one", opts(), 25, 17, 70, online_fresh_workspace_bytes(25, 17, 70, 32, EVC_F64) - 1);
    run("plain_ws_is_too_small", opts(), 25, 17, 70, online_workspace_bytes(25, 17, 70, 32, EVC_F64));
    { auto o = opts(); o.struct_bytes = (int)sizeof(evc_online_opts); run("struct_bytes", o, 25, 17, 70, big); }
    { auto o = opts(); o.fresh_max_iter = 0; run("fresh_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.fresh_max_iter = BETA_MAX_SLOTS + 1; run("fresh_4098", o, 25, 17, 70, big); }
    { auto o = opts(); o.final_max_iter = -1; run("final_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.final_max_iter = 0; run("final_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.final_max_iter = BETA_MAX_SLOTS + 1; run("final_4098", o, 25, 17, 70, big); }
    { auto o = opts(); o.forget_factor = 0.0; run("forget_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.resume = 2; run("resume", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 1 << 16; run("fused_257", o, 25, 257, 70, big); }
    run("R_65", opts(), 25, 65, 70, big);
    run("M_529", opts(), 529, 17, 70, 16);
    { auto o = opts(); o.fresh_max_iter = 0; run("count_before_limits", o, 529, 17, 70, 16); }
}

int main() {
    for (size_t shift : {size_t(0), size_t(8)}) {
        carve_line(25, 24, 70, 1, EVC_F64, shift);
        carve_line(25, 24, 70, 4, EVC_F64, shift);
        carve_line(201, 512, 11008, 16, EVC_F32, shift);
        carve_line(50, 512, 65536, 1, EVC_F64, shift);
        carve_line(528, 4096, 0, 1, EVC_F32, shift);
        carve_line(1, 1, 1, 1, EVC_F64, shift);
    }
    args_lines();
    for (int k : {0, 1, 200, BETA_MAX_SLOTS}) printf("slots %d %d\n", k, transform_slots(k));
    for (size_t shift : {size_t(0), size_t(8)}) {
        fcarve_line(25, 24, 300, 100, EVC_F64, shift);
        fcarve_line(25, 24, 330, 100, EVC_F64, shift);
        fcarve_line(201, 32, 200, 1024, EVC_F32, shift);
        fcarve_line(50, 512, 65536, 1024, EVC_F64, shift);
        fcarve_line(1, 1, 1, 1, EVC_F64, shift);
    }
    fargs_lines();
    return 0;
}
