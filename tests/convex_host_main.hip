// convex_host_main.hip - a program of its own (host code only) that runs what evc_convex_learn (csrc/evc_convex_plan.h)
// decides on the host and prints it: tests/test_convex_host.py builds it, once plainly and once under the address and
// undefined-behaviour sanitizers, and checks the lines.
//   carve <M R T S esize> shift <s> : <byte offsets of K, Np, Nn, Q1, Q2, part, rrpart, Sp, Sn, Wm, V, err2, trace, eprev, stop> bytes <b> query <q>
//   args <case> <status> <W> <S>   convex_args_check over a grid of bad and good arguments, and the plan it leaves
//   plan <T R> <W> <S> <workgroups> <Z>   convex_plan and convex_rr_splits over a grid of sizes
#include "../exemplars_vc_amd/csrc/evc_convex_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace evc;

static void carve_line(int M, int R, int T_, int S, int dtype, size_t shift) {
    std::vector<char> mem(4096);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~uintptr_t(255)) + shift;
    const ConvexWs w = carve_convex(base, M, R, T_, S, dtype);        // addresses only: nothing is dereferenced
    const char* arr[] = {w.K, w.Np, w.Nn, w.Q1, w.Q2, w.part, w.rrpart, w.Sp, w.Sn, w.Wm, w.V, reinterpret_cast<char*>(w.err2),
                         reinterpret_cast<char*>(w.trace), reinterpret_cast<char*>(w.eprev), reinterpret_cast<char*>(w.stop)};
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t TP = (size_t)round_up(T_, CONVEX_BN), tr = (size_t)T_ * R * es, rr = (size_t)R * R * es;
    const int Z = convex_rr_splits(T_, R);
    const size_t room[] = {TP * TP * es, tr, tr, tr, tr, S > 1 ? 2 * (size_t)S * tr : 0, Z > 1 ? (size_t)Z * rr : 0, rr, rr, (size_t)M * R * es,
                           (size_t)T_ * M * es, (size_t)T_ * 8, (size_t)CONVEX_MAX_SLOTS * 8, 8, 4};
    printf("carve %d %d %d %d %zu shift %zu :", M, R, T_, S, es, shift);
    for (int i = 0; i < 15; ++i) {
        const size_t off = (size_t)(arr[i] - base);
        const size_t end = i < 14 ? (size_t)(arr[i + 1] - base) : w.bytes;
        if ((reinterpret_cast<uintptr_t>(arr[i]) & 255) != 0 || off + room[i] > end) {
            printf(" BAD");
            exit(3);
        }
        printf(" %zu", off);
    }
    const size_t need = convex_workspace_bytes(M, R, T_, dtype, S);
    if (w.bytes > need) {
        printf(" BAD SIZE");
        exit(4);
    }
    printf(" bytes %zu query %zu\n", w.bytes, need);
}

static void args_lines() {
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
    auto opts = [] {
        evc_convex_opts o{};
        o.struct_bytes = (int)sizeof(o);
        o.dtype = EVC_F64; o.layout = EVC_FRAME_MAJOR; o.iters = 100;
        o.check_every = 1; o.update = EVC_CONVEX_BOTH; o.tol = 2.22e-16; o.eps = 1e-9;
        return o;
    };
    // frame-major: ldx >= M, ldh >= R, ldw >= M; ldg >= R always
    auto run = [&](const char* name, const evc_convex_opts& o, int M, int R, int T, size_t ws, bool with_w = true, int ldg = -1,
                   bool with_g = true) {
        ConvexPlan pl{0, 0};
        const int st = convex_args_check(p, M, with_g ? p : nullptr, ldg < 0 ? R : ldg, p, R, with_w ? p : nullptr, with_w ? M : 0, M,
                                         R, T, &o, p, ws, &pl);
        printf("args %s %d %d %d\n", name, st, pl.W, pl.S);
    };
    const size_t big = size_t(1) << 40;
    run("ok", opts(), 25, 17, 70, big);
    run("ok_exact", opts(), 25, 17, 70, convex_workspace_bytes(25, 17, 70, EVC_F64));
    run("short_by_one", opts(), 25, 17, 70, convex_workspace_bytes(25, 17, 70, EVC_F64) - 1);
    run("f32_ws", opts(), 25, 17, 70, convex_workspace_bytes(25, 17, 70, EVC_F32));
    run("no_w", opts(), 25, 17, 70, big, false);
    run("no_g", opts(), 25, 17, 70, big, true, -1, false);
    run("ldg_short", opts(), 25, 17, 70, big, true, 16);
    run("ldg_padded", opts(), 25, 17, 70, big, true, 40);
    { auto o = opts(); o.struct_bytes = 4; run("struct_bytes", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = -1; run("iters_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = 0; run("iters_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = CONVEX_MAX_SLOTS - 1; run("slots_4097", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = CONVEX_MAX_SLOTS; run("slots_4098", o, 25, 17, 70, big); }
    { auto o = opts(); o.check_every = -1; run("check_every_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.check_every = 0; run("check_every_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 1; run("reserved_low", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 1 << 24; run("reserved_high", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 7 << 8; run("forced_s7", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 7 << 8; run("forced_s7_plan_ws", o, 25, 17, 70, convex_workspace_bytes(25, 17, 70, EVC_F64)); }
    { auto o = opts(); o.reserved = 7 << 8; run("forced_s7_own_ws", o, 25, 17, 70, convex_workspace_bytes(25, 17, 70, EVC_F64, 7)); }
    { auto o = opts(); o.reserved = 16 << 8; run("forced_s16", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 17 << 8; run("forced_s17", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 8 << 16; run("forced_w8", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = (4 << 16) | (3 << 8); run("forced_w4_s3", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 3 << 16; run("forced_w3", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 1 << 16; run("forced_w1", o, 25, 17, 70, big); }
    { auto o = opts(); o.update = EVC_CONVEX_H_ONLY; run("h_only", o, 25, 17, 70, big); }
    { auto o = opts(); o.update = EVC_CONVEX_G_ONLY; run("g_only", o, 25, 17, 70, big); }
    { auto o = opts(); o.update = 3; run("update_3", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = -1e-9; run("tol_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = 0.0; run("tol_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.eps = -1e-9; run("eps_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.eps = 0.0; run("eps_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.eps = __builtin_nan(""); run("eps_nan", o, 25, 17, 70, big); }
    { auto o = opts(); o.eps = __builtin_inf(); run("eps_inf", o, 25, 17, 70, big); }
    { auto o = opts(); o.dtype = 7; run("dtype", o, 25, 17, 70, big); }
    { auto o = opts(); o.layout = 5; run("layout", o, 25, 17, 70, big); }
    run("M_0", opts(), 0, 17, 70, big);
    run("R_0", opts(), 25, 0, 70, big);
    run("T_0", opts(), 25, 17, 0, big);
    run("M_1056", opts(), CONVEX_MAX_M, 17, 70, big);
    run("M_1057", opts(), CONVEX_MAX_M + 1, 17, 70, big);
    run("M_1057_small_ws", opts(), CONVEX_MAX_M + 1, 17, 70, 16);
    run("T_16384", opts(), 25, 17, CONVEX_MAX_T, big);
    run("T_16384_small_ws", opts(), 25, 17, CONVEX_MAX_T, size_t(1) << 31);
    run("T_16385", opts(), 25, 17, CONVEX_MAX_T + 1, big);
    run("T_16385_small_ws", opts(), 25, 17, CONVEX_MAX_T + 1, 16);
    run("R_1024", opts(), 25, CONVEX_MAX_R, 4096, big);
    run("R_1025", opts(), 25, CONVEX_MAX_R + 1, 4096, big);
    run("R_eq_T", opts(), 25, 70, 70, big);
    run("R_above_T", opts(), 25, 71, 70, big);
    run("R_above_T_small_ws", opts(), 25, 71, 70, 16);
    { auto o = opts(); o.tol = __builtin_nan(""); run("nan_before_limits", o, CONVEX_MAX_M + 1, 17, 70, 16); }
    { auto o = opts(); o.reserved = 2; run("reserved_before_limits", o, 25, 17, CONVEX_MAX_T + 1, 16); }
}

int main() {
    for (size_t shift : {size_t(0), size_t(8)}) {
        carve_line(25, 8, 70, 1, EVC_F64, shift);
        carve_line(25, 17, 257, 4, EVC_F32, shift);
        carve_line(50, 256, 4096, 1, EVC_F64, shift);
        carve_line(1056, 1024, 16384, 1, EVC_F64, shift);
        carve_line(50, 64, 4096, 16, EVC_F64, shift);
        carve_line(1, 1, 1, 1, EVC_F32, shift);
    }
    args_lines();
    const int Ts[] = {1, 5, 16, 17, 63, 64, 65, 129, 130, 257, 300, 1000, 1024, 2048, 4095, 4096, 4097, 8192, 16383, 16384};
    const int Rs[] = {1, 2, 15, 16, 17, 33, 63, 64, 65, 128, 130, 256, 257, 512, 1024};
    for (int T_ : Ts)
        for (int R : Rs) {
            if (R > T_) continue;
            const ConvexPlan pl = convex_plan(T_, R);
            printf("plan %d %d %d %d %ld %d\n", T_, R, pl.W, pl.S, convex_workgroups(T_, R, pl.W) * pl.S, convex_rr_splits(T_, R));
        }
    return 0;
}
