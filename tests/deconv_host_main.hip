// deconv_host_main.hip - a program of its own (host code only, linked against the library for the activation half's size
// query) that runs what evc_deconv_solve and evc_deconv_synthesize (csrc/evc_deconv_plan.h) decide on the host and prints it:
// tests/test_deconv_host.py builds it, once plainly and once under the address and undefined-behaviour sanitizers, and checks
// the lines.
//   carve <M N T n_utt taps esize> shift <s> : <byte offsets of Ap1, Ap3, Qn, Qd and the activation half> bytes <b> query <q>
//   args <case> <status>    deconv_args_check over a grid of bad and good arguments
//   sargs <case> <status>   deconv_synth_args_check
#include "../exemplars_vc_amd/csrc/evc_deconv_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace evc;

static void carve_line(int M, int N, int T_, int n_utt, int taps, int dtype, size_t shift) {
    std::vector<char> mem(4096);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~uintptr_t(255)) + shift;
    const DcWs w = carve_deconv(base, M, N, T_, n_utt, taps, dtype);        // addresses only: nothing is dereferenced
    const char* arr[] = {w.Ap1, w.Ap3, w.Qn, w.Qd, w.beta_ws};
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t MP = (size_t)round_up(M, 16), NP = (size_t)round_up(N, 16);
    const size_t dict = (size_t)taps * NP * MP * es, img = (size_t)frame_tile_cap(T_, BT_F, n_utt) * MP * BT_F * es;
    const size_t room[] = {dict, dict, img, img, w.beta_bytes};
    printf("carve %d %d %d %d %d %zu shift %zu :", M, N, T_, n_utt, taps, es, shift);
    for (int i = 0; i < 5; ++i) {
        const size_t off = (size_t)(arr[i] - base);
        const size_t end = i < 4 ? (size_t)(arr[i + 1] - base) : w.bytes;
        if ((reinterpret_cast<uintptr_t>(arr[i]) & 255) != 0 || off + room[i] > end) {
            printf(" BAD");
            exit(3);
        }
        printf(" %zu", off);
    }
    const size_t need = deconv_workspace_bytes(M, N, T_, n_utt, taps, dtype);
    if (w.bytes > need) {
        printf(" BAD SIZE");
        exit(4);
    }
    printf(" bytes %zu query %zu\n", w.bytes, need);
}

static void args_lines() {
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
    auto opts = [] {
        evc_deconv_opts o{};
        o.struct_bytes = (int)sizeof(o);
        o.dtype = EVC_F64; o.layout = EVC_FRAME_MAJOR; o.loss = EVC_LOSS_KL; o.taps = 4; o.iters = 100;
        o.init_mode = EVC_INIT_SKLEARN; o.check_every = 10; o.stop_rule = EVC_STOP_SKLEARN; o.tol = 1e-4;
        return o;
    };
    const int offs_ok[] = {0, 30, 30, 70}, offs_bad[] = {0, 40, 30, 70};
    auto run = [&](const char* name, const evc_deconv_opts& o, int M, int N, int T, size_t ws, const int* offs = nullptr,
                   int n_utt = 1, bool with_x = true, long tap_stride = 25 * 17) {
        const int st = deconv_args_check(p, M, tap_stride, with_x ? p : nullptr, M, p, N, M, N, T, offs, n_utt, &o, p, ws);
        printf("args %s %d\n", name, st);
    };
    const size_t big = size_t(1) << 40;
    run("ok", opts(), 25, 17, 70, big);
    run("ok_exact", opts(), 25, 17, 70, deconv_workspace_bytes(25, 17, 70, 1, 4, EVC_F64));
    run("short_by_one", opts(), 25, 17, 70, deconv_workspace_bytes(25, 17, 70, 1, 4, EVC_F64) - 1);
    run("fewer_taps_ws", opts(), 25, 17, 70, deconv_workspace_bytes(25, 17, 70, 1, 3, EVC_F64));
    run("ok_utts", opts(), 25, 17, 70, big, offs_ok, 3);
    run("bad_utts", opts(), 25, 17, 70, big, offs_bad, 3);
    run("no_frames_no_x", opts(), 25, 17, 0, big, nullptr, 1, false);
    run("frames_no_x", opts(), 25, 17, 70, big, nullptr, 1, false);
    run("tap_stride_0", opts(), 25, 17, 70, big, nullptr, 1, true, 0);
    run("tap_stride_neg", opts(), 25, 17, 70, big, nullptr, 1, true, -1);
    { auto o = opts(); o.struct_bytes = 4; run("struct_bytes", o, 25, 17, 70, big); }
    { auto o = opts(); o.taps = 0; run("taps_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.taps = 1; run("taps_1", o, 25, 17, 70, big); }
    { auto o = opts(); o.taps = DC_MAX_TAPS; run("taps_16", o, 25, 17, 70, big); }
    { auto o = opts(); o.taps = DC_MAX_TAPS + 1; run("taps_17", o, 25, 17, 70, big); }
    { auto o = opts(); o.taps = DC_MAX_TAPS + 1; run("taps_17_small_ws", o, 25, 17, 70, 16); }
    { auto o = opts(); o.loss = 2; run("loss", o, 25, 17, 70, big); }
    { auto o = opts(); o.loss = EVC_LOSS_FROBENIUS; run("frobenius", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = -1; run("iters_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = 0; run("iters_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.check_every = 1; o.iters = BETA_MAX_SLOTS - 1; run("slots_4097", o, 25, 17, 70, big); }
    { auto o = opts(); o.check_every = 1; o.iters = BETA_MAX_SLOTS; run("slots_4098", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 1; run("reserved", o, 25, 17, 70, big); }
    { auto o = opts(); o.init_mode = 3; run("init_mode", o, 25, 17, 70, big); }
    { auto o = opts(); o.stop_rule = EVC_STOP_PYMF; run("stop_rule", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = -1e-9; run("tol_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = 0.0; run("tol_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.l1 = -1.0; run("l1_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.l2 = __builtin_nan(""); run("l2_nan", o, 25, 17, 70, big); }
    { auto o = opts(); o.init_value = __builtin_inf(); run("init_value_inf", o, 25, 17, 70, big); }
    { auto o = opts(); o.dtype = 7; run("dtype", o, 25, 17, 70, big); }
    run("M_256", opts(), 256, 17, 70, big);
    run("M_257", opts(), 257, 17, 70, big);
    run("M_257_small_ws", opts(), 257, 17, 70, 16);
    run("N_100000", opts(), 25, 100000, 70, big);
    { auto o = opts(); o.tol = __builtin_nan(""); run("nan_before_limits", o, 257, 17, 70, 16); }
    { auto o = opts(); o.taps = 0; run("taps_0_before_limits", o, 257, 17, 70, 16); }
}

static void sargs_lines() {
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
    const int offs_ok[] = {0, 30, 30, 70}, offs_bad[] = {0, 40, 30, 70};
    auto run = [&](const char* name, int Mb, int N, int T, int taps, int layout = EVC_FRAME_MAJOR, int dtype = EVC_F64,
                   const int* offs = nullptr, int n_utt = 1, bool with_h = true, long tap_stride = 1) {
        const bool fm = layout == EVC_FRAME_MAJOR;
        const int st = deconv_synth_args_check(p, fm ? Mb : N, tap_stride, with_h ? p : nullptr, fm ? N : T, p, fm ? Mb : T, Mb, N,
                                               T, offs, n_utt, taps, layout, dtype);
        printf("sargs %s %d\n", name, st);
    };
    run("ok", 513, 17, 70, 4);
    run("ok_bin_major", 513, 17, 70, 4, EVC_BIN_MAJOR, EVC_F32);
    run("ok_utts", 513, 17, 70, 4, EVC_FRAME_MAJOR, EVC_F64, offs_ok, 3);
    run("bad_utts", 513, 17, 70, 4, EVC_FRAME_MAJOR, EVC_F64, offs_bad, 3);
    run("no_frames_no_h", 513, 17, 0, 4, EVC_FRAME_MAJOR, EVC_F64, nullptr, 1, false);
    run("frames_no_h", 513, 17, 70, 4, EVC_FRAME_MAJOR, EVC_F64, nullptr, 1, false);
    run("Mb_0", 0, 17, 70, 4);
    run("Mb_1056", DC_MAX_MB, 17, 70, 4);
    run("Mb_1057", DC_MAX_MB + 1, 17, 70, 4);
    run("taps_0", 513, 17, 70, 0);
    run("taps_16", 513, 17, 70, DC_MAX_TAPS);
    run("taps_17", 513, 17, 70, DC_MAX_TAPS + 1);
    run("taps_0_before_limits", DC_MAX_MB + 1, 17, 70, 0);
    run("layout", 513, 17, 70, 4, 5);
    run("dtype", 513, 17, 70, 4, EVC_FRAME_MAJOR, 9);
    run("tap_stride_neg", 513, 17, 70, 4, EVC_FRAME_MAJOR, EVC_F64, nullptr, 1, true, -5);
}

int main() {
    for (size_t shift : {size_t(0), size_t(8)}) {
        carve_line(25, 24, 70, 1, 4, EVC_F64, shift);
        carve_line(25, 24, 70, 4, 1, EVC_F64, shift);
        carve_line(201, 4096, 11008, 16, 4, EVC_F32, shift);
        carve_line(25, 4096, 11008, 16, 8, EVC_F64, shift);
        carve_line(256, 100000, 0, 1, 16, EVC_F64, shift);
        carve_line(1, 1, 1, 1, 1, EVC_F32, shift);
    }
    args_lines();
    sargs_lines();
    return 0;
}
