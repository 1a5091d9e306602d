// kmeans_host_main.hip - a program of its own (host code only) that runs what evc_kmeans (csrc/evc_kmeans_plan.h) decides on
// the host and prints it: tests/test_kmeans_host.py builds it, once plainly and once under the address and
// undefined-behaviour sanitizers, and checks the lines.
//   carve <R T S esize> shift <s> : <byte offsets of xn, wn, s1, s2, ps1, ps2, pi1, flag, lab, prev, chg, cnt, err2, trace, eprev, stop> bytes <b> query <q>
//   args <case> <status> <S>   kmeans_args_check over a grid of bad and good arguments, and the centre ranges it leaves
//   query <case> <bytes>       kmeans_workspace_bytes at the limits and one past them
//   splits <T R> <S>           kmeans_splits over a grid of sizes
#include "../exemplars_vc_amd/csrc/evc_kmeans_plan.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace evc;

static void carve_line(int R, int T_, int S, int dtype, size_t shift) {
    std::vector<char> mem(4096);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~uintptr_t(255)) + shift;
    const KmWs w = carve_kmeans(base, R, T_, S, dtype);        // addresses only: nothing is dereferenced
    const char* arr[] = {w.xn, w.wn, w.s1, w.s2, w.ps1, w.ps2, reinterpret_cast<char*>(w.pi1), reinterpret_cast<char*>(w.flag),
                         reinterpret_cast<char*>(w.lab), reinterpret_cast<char*>(w.prev), reinterpret_cast<char*>(w.chg),
                         reinterpret_cast<char*>(w.cnt), reinterpret_cast<char*>(w.err2), reinterpret_cast<char*>(w.trace),
                         reinterpret_cast<char*>(w.eprev), reinterpret_cast<char*>(w.stop)};
    const size_t es = dtype == EVC_F64 ? 8 : 4, t = (size_t)T_, st = S > 1 ? (size_t)S * t : 0;
    const size_t room[] = {t * es, (size_t)R * es, t * es, t * es, st * es, st * es, st * 4, t * 4, t * 4, t * 4, t * 4, (size_t)R * 4,
                           t * 8, (size_t)KM_MAX_SLOTS * 8, 8, 4};
    printf("carve %d %d %d %zu shift %zu :", R, T_, S, es, shift);
    for (int i = 0; i < 16; ++i) {
        const size_t off = (size_t)(arr[i] - base);
        const size_t end = i < 15 ? (size_t)(arr[i + 1] - base) : w.bytes;
        if ((reinterpret_cast<uintptr_t>(arr[i]) & 255) != 0 || off + room[i] > end) {
            printf(" BAD");
            exit(3);
        }
        printf(" %zu", off);
    }
    const size_t need = kmeans_workspace_bytes(25, R, T_, dtype, S);
    if (w.bytes > need) {
        printf(" BAD SIZE");
        exit(4);
    }
    printf(" bytes %zu query %zu\n", w.bytes, need);
}

static void args_lines() {
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
    auto opts = [] {
        evc_kmeans_opts o{};
        o.struct_bytes = (int)sizeof(o);
        o.dtype = EVC_F64; o.layout = EVC_FRAME_MAJOR; o.iters = 10;
        o.update = EVC_KM_BOTH; o.stop_rule = EVC_KM_STOP_PYMF; o.tol = 2.22e-16;
        return o;
    };
    // frame-major: ldx >= M, ldw >= M
    auto run = [&](const char* name, const evc_kmeans_opts& o, int M, int R, int T, size_t ws, int ldx = -1, int ldw = -1,
                   bool with_x = true, bool with_w = true, bool with_ws = true) {
        int S = 0;
        const int st = kmeans_args_check(with_x ? p : nullptr, ldx < 0 ? M : ldx, with_w ? p : nullptr, ldw < 0 ? M : ldw, M, R, T, &o,
                                         with_ws ? p : nullptr, ws, &S);
        printf("args %s %d %d\n", name, st, S);
    };
    const size_t big = size_t(1) << 40;
    run("ok", opts(), 25, 17, 70, big);
    run("ok_exact", opts(), 25, 17, 70, kmeans_workspace_bytes(25, 17, 70, EVC_F64));
    run("short_by_one", opts(), 25, 17, 70, kmeans_workspace_bytes(25, 17, 70, EVC_F64) - 1);
    run("f32_ws", opts(), 25, 17, 70, kmeans_workspace_bytes(25, 17, 70, EVC_F32));
    run("no_x", opts(), 25, 17, 70, big, -1, -1, false);
    run("no_w", opts(), 25, 17, 70, big, -1, -1, true, false);
    run("no_ws", opts(), 25, 17, 70, big, -1, -1, true, true, false);
    run("ldx_short", opts(), 25, 17, 70, big, 24);
    run("ldw_short", opts(), 25, 17, 70, big, -1, 24);
    run("ld_padded", opts(), 25, 17, 70, big, 40, 33);
    { auto o = opts(); o.layout = EVC_BIN_MAJOR; run("bin_major", o, 25, 17, 70, big, 70, 17); }
    { auto o = opts(); o.layout = EVC_BIN_MAJOR; run("bin_major_ldx_short", o, 25, 17, 70, big, 69, 17); }
    { auto o = opts(); o.layout = EVC_BIN_MAJOR; run("bin_major_ldw_short", o, 25, 17, 70, big, 70, 16); }
    { auto o = opts(); o.struct_bytes = 4; run("struct_bytes", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = -1; run("iters_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = 0; run("iters_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = KM_MAX_SLOTS - 1; run("slots_4097", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = KM_MAX_SLOTS; run("slots_4098", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = INT_MAX; run("iters_int_max", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 1; run("redecide", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 2; run("reserved_bit1", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 1 << 16; run("reserved_high", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 7 << 8; run("forced_s7", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 7 << 8; run("forced_s7_plan_ws", o, 25, 17, 70, kmeans_workspace_bytes(25, 17, 70, EVC_F64)); }
    { auto o = opts(); o.reserved = 7 << 8; run("forced_s7_own_ws", o, 25, 17, 70, kmeans_workspace_bytes(25, 17, 70, EVC_F64, 7)); }
    { auto o = opts(); o.reserved = (16 << 8) | 1; run("forced_s16_redecide", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 17 << 8; run("forced_s17", o, 25, 17, 70, big); }
    { auto o = opts(); o.update = EVC_KM_ASSIGN_ONLY; run("assign_only", o, 25, 17, 70, big); }
    { auto o = opts(); o.update = 2; run("update_2", o, 25, 17, 70, big); }
    { auto o = opts(); o.stop_rule = EVC_KM_STOP_NONE; run("stop_none", o, 25, 17, 70, big); }
    { auto o = opts(); o.stop_rule = EVC_KM_STOP_LABELS; run("stop_labels", o, 25, 17, 70, big); }
    { auto o = opts(); o.stop_rule = 3; run("stop_3", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = -1e-9; run("tol_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = 0.0; run("tol_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = __builtin_nan(""); run("tol_nan", o, 25, 17, 70, big); }
    { auto o = opts(); o.dtype = 7; run("dtype", o, 25, 17, 70, big); }
    { auto o = opts(); o.layout = 5; run("layout", o, 25, 17, 70, big); }
    run("M_0", opts(), 0, 17, 70, big);
    run("R_0", opts(), 25, 0, 70, big);
    run("T_0", opts(), 25, 17, 0, big);
    run("M_1056", opts(), KM_MAX_M, 17, 70, big);
    run("M_1057", opts(), KM_MAX_M + 1, 17, 70, big);
    run("M_1057_small_ws", opts(), KM_MAX_M + 1, 17, 70, 16);
    run("T_max", opts(), 25, 17, KM_MAX_T, big);
    run("T_max_small_ws", opts(), 25, 17, KM_MAX_T, size_t(1) << 20);
    run("T_past", opts(), 25, 17, KM_MAX_T + 1, big);
    run("T_past_small_ws", opts(), 25, 17, KM_MAX_T + 1, 16);
    run("R_4096", opts(), 25, KM_MAX_R, 8192, big);
    run("R_4097", opts(), 25, KM_MAX_R + 1, 8192, big);
    run("R_eq_T", opts(), 25, 70, 70, big);
    run("R_above_T", opts(), 25, 71, 70, big);
    run("R_above_T_small_ws", opts(), 25, 71, 70, 16);
    { auto o = opts(); o.update = EVC_KM_ASSIGN_ONLY; run("R_above_T_assign_only", o, 25, 71, 70, big); }
    { auto o = opts(); o.update = EVC_KM_ASSIGN_ONLY; run("R_4097_assign_only", o, 25, KM_MAX_R + 1, 70, big); }
    { auto o = opts(); o.tol = __builtin_nan(""); run("nan_before_limits", o, KM_MAX_M + 1, 17, 70, 16); }
    { auto o = opts(); o.reserved = 4; run("reserved_before_limits", o, 25, 17, KM_MAX_T + 1, 16); }
}

static void query_lines() {
    auto q = [](const char* name, int M, int R, int T_, int dtype) { printf("query %s %zu\n", name, kmeans_workspace_bytes(M, R, T_, dtype)); };
    q("small", 25, 17, 70, EVC_F64);
    q("small_f32", 25, 17, 70, EVC_F32);
    q("M_1056", KM_MAX_M, 17, 70, EVC_F64);
    q("M_1057", KM_MAX_M + 1, 17, 70, EVC_F64);
    q("T_max", 25, 17, KM_MAX_T, EVC_F64);
    q("T_past", 25, 17, KM_MAX_T + 1, EVC_F64);
    q("R_4096", 25, KM_MAX_R, KM_MAX_T, EVC_F64);
    q("R_4097", 25, KM_MAX_R + 1, KM_MAX_T, EVC_F64);
    q("zero_M", 0, 17, 70, EVC_F64);
    q("zero_R", 25, 0, 70, EVC_F64);
    q("zero_T", 25, 17, 0, EVC_F64);
    q("dtype", 25, 17, 70, 9);
}

int main() {
    for (size_t shift : {size_t(0), size_t(8)}) {
        carve_line(8, 70, 1, EVC_F64, shift);
        carve_line(17, 257, 4, EVC_F32, shift);
        carve_line(1024, 16384, 1, EVC_F64, shift);
        carve_line(KM_MAX_R, KM_MAX_T, 1, EVC_F64, shift);
        carve_line(KM_MAX_R, KM_MAX_T, KM_MAX_S, EVC_F64, shift);
        carve_line(1, 1, 1, EVC_F32, shift);
        carve_line(64, 4096, 2, EVC_F32, shift);
    }
    args_lines();
    query_lines();
    const int Ts[] = {1, 5, 16, 17, 63, 64, 65, 129, 257, 300, 1000, 1024, 2048, 4095, 4096, 4097, 8192, 16383, 16384, 16385, 65536, KM_MAX_T};
    const int Rs[] = {1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 130, 256, 257, 512, 1024, 4096};
    for (int T_ : Ts)
        for (int R : Rs)
            if (R <= T_) printf("splits %d %d %d\n", T_, R, kmeans_splits(R, T_));
    return 0;
}
