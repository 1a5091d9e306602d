// prox_masked_learn_host_main.hip - a program of its own (host code only) that runs what evc_prox_masked_learn
// (csrc/evc_prox_masked_learn_plan.h) decides on the host and prints it: tests/test_prox_masked_learn_host.py builds it, once
// plainly and once under the address and undefined-behaviour sanitizers, and checks the lines.
//   carve <M N T bs esize> shift <s> : <byte offsets of the 8 arrays in carving order> bytes <b> query <q>
//   args <case> <status>     pmlearn_args_check over a grid of bad and good arguments
//   limit <M> <N> <0|1>      pmlearn_too_large
//   lasso <field> <value>    the options of a step's lasso
#include "../exemplars_vc_amd/csrc/evc_prox_masked_learn_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace evc;

static void carve_line(int M, int N, int T_, int bs, int dtype, size_t shift) {
    std::vector<char> mem(4096);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~uintptr_t(255)) + shift;
    const PMLearnWs w = carve_pmlearn(base, M, N, T_, bs, dtype);      // addresses only: nothing is dereferenced
    const char* arr[PMLEARN_WS_ARRAYS] = {w.Z, w.G, w.diag, w.Dt, reinterpret_cast<char*>(w.shares),
                                          reinterpret_cast<char*>(w.stat), reinterpret_cast<char*>(w.ord), w.prox_ws};
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t nm = (size_t)N * M * es;
    const size_t room[PMLEARN_WS_ARRAYS] = {((size_t)N + 2 * (size_t)M) * bs * es, nm, nm, nm, (size_t)N * 8, 8, (size_t)T_ * 4,
                                            prox_masked_workspace_bytes(M, N, bs, 1, dtype)};
    const char* first = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(base) + 255) & ~uintptr_t(255));
    printf("carve %d %d %d %d %zu shift %zu :", M, N, T_, bs, es, shift);
    for (int i = 0; i < PMLEARN_WS_ARRAYS; ++i) {
        const size_t off = (size_t)(arr[i] - base);
        const size_t end = i < PMLEARN_WS_ARRAYS - 1 ? (size_t)(arr[i + 1] - base) : w.bytes;
        if ((reinterpret_cast<uintptr_t>(arr[i]) & 255) != 0 || off + room[i] > end || arr[i] < first) {
            printf(" BAD");
            exit(3);
        }
        printf(" %zu", off);
    }
    const size_t need = prox_masked_learn_workspace_bytes(M, N, T_, bs, dtype);
    if (w.bytes > need || room[PMLEARN_WS_ARRAYS - 1] == 0 || w.prox_bytes != room[PMLEARN_WS_ARRAYS - 1]) {
        printf(" BAD SIZE");
        exit(4);
    }
    printf(" bytes %zu query %zu\n", w.bytes, need);
}

static evc_prox_masked_learn_opts good_opts() {
    evc_prox_masked_learn_opts o{};
    o.struct_bytes = (int)sizeof(o);
    o.dtype = EVC_F64; o.layout = EVC_FRAME_MAJOR; o.batch_size = 32; o.epochs = 3; o.lasso_iters = 10;
    o.lasso_check_every = 10; o.mode = EVC_PROX_POSITIVE; o.momentum = EVC_PROX_FISTA; o.alpha = 1e-3; o.lasso_tol = 1e-5;
    return o;
}

static const void* const P = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
struct Shape { int M = 25, N = 17, T = 70, ldx = 25, ldm = 25, ldd = 25, ldh = 17, lds = 17, ldq = 25; };
struct Ptrs { const void *X, *mask, *D, *H, *S, *Q, *ws; };
static const Ptrs all{P, P, P, P, P, P, P};

static void args_lines() {
    long long count = 0;
    const size_t big = (size_t)1 << 40;
    auto run = [&](const char* name, const evc_prox_masked_learn_opts* o, Shape s, size_t ws, const int* order = nullptr,
                   Ptrs q = all, const long long* cnt = nullptr) {
        printf("args %s %d\n", name, pmlearn_args_check(q.X, s.ldx, q.mask, s.ldm, q.D, s.ldd, q.H, s.ldh, q.S, s.lds, q.Q, s.ldq,
                                                       cnt ? cnt : &count, order, s.M, s.N, s.T, o, q.ws, ws));
    };
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    evc_prox_masked_learn_opts o = good_opts();
    Shape s;
    const size_t exact = prox_masked_learn_workspace_bytes(25, 17, 70, 32, EVC_F64);
    run("ok", &o, s, big);
    run("ok_exact", &o, s, exact);
    run("short_by_one", &o, s, exact - 1);
    run("no_opts", nullptr, s, big);
    { Ptrs q = all; q.X = nullptr; run("no_x", &o, s, big, nullptr, q); }
    { Ptrs q = all; q.mask = nullptr; run("no_mask", &o, s, big, nullptr, q); }
    { Ptrs q = all; q.D = nullptr; run("no_d", &o, s, big, nullptr, q); }
    { Ptrs q = all; q.H = nullptr; run("no_h", &o, s, big, nullptr, q); }
    { Ptrs q = all; q.S = nullptr; run("no_stats_s", &o, s, big, nullptr, q); }
    { Ptrs q = all; q.Q = nullptr; run("no_stats_q", &o, s, big, nullptr, q); }
    { Ptrs q = all; q.ws = nullptr; run("no_workspace", &o, s, big, nullptr, q); }
    o = good_opts(); o.struct_bytes -= 8; run("struct_bytes", &o, s, big);
    o = good_opts(); o.dtype = 2; run("dtype", &o, s, big);
    o = good_opts(); o.layout = 2; run("layout", &o, s, big);
    o = good_opts(); o.batch_size = 0; run("batch_0", &o, s, big);
    o = good_opts(); o.batch_size = 70; run("batch_T", &o, s, big);
    o = good_opts(); o.batch_size = 71; run("batch_T_plus_1", &o, s, big);
    o = good_opts(); o.epochs = -1; run("epochs_neg", &o, s, big);
    o = good_opts(); o.epochs = 0; run("epochs_0", &o, s, big);
    o = good_opts(); o.epochs = 0x7fffffff; o.batch_size = 1; run("steps_beyond_int", &o, s, big);
    o = good_opts(); o.lasso_iters = -1; run("lasso_iters_neg", &o, s, big);
    o = good_opts(); o.lasso_iters = 0; run("lasso_iters_0", &o, s, big);
    o = good_opts(); o.lasso_iters = 4098; o.lasso_check_every = 1; run("slots_4098", &o, s, big);
    o = good_opts(); o.lasso_iters = 4097; o.lasso_check_every = 1; run("slots_4097", &o, s, big);
    o = good_opts(); o.lasso_check_every = -1; run("check_every_neg", &o, s, big);
    o = good_opts(); o.mode = 2; run("mode", &o, s, big);
    o = good_opts(); o.mode = EVC_PROX_SIGNED; run("mode_signed", &o, s, big);
    o = good_opts(); o.momentum = 3; run("momentum", &o, s, big);
    o = good_opts(); o.momentum = EVC_PROX_NESTEROV; run("momentum_nesterov", &o, s, big);
    o = good_opts(); o.resume = 2; run("resume_2", &o, s, big);
    o = good_opts(); o.resume = 1; run("resume_1", &o, s, big);
    { const long long neg = -1; o = good_opts(); o.resume = 1; run("resume_count_neg", &o, s, big, nullptr, all, &neg);
      o = good_opts(); run("fresh_count_neg", &o, s, big, nullptr, all, &neg); }
    o = good_opts(); o.reserved = 8; run("reserved", &o, s, big);
    o = good_opts(); o.reserved = 7; run("reserved_halves_off", &o, s, big);
    o = good_opts(); o.reserved2 = 1; run("reserved2", &o, s, big);
    o = good_opts(); o.alpha = -1; run("alpha_neg", &o, s, big);
    o = good_opts(); o.alpha = nan; run("alpha_nan", &o, s, big);
    o = good_opts(); o.alpha = 0; run("alpha_0", &o, s, big);
    o = good_opts(); o.tol = -1; run("tol_neg", &o, s, big);
    o = good_opts(); o.tol = inf; run("tol_inf", &o, s, big);
    o = good_opts(); o.tol = 1e-3; run("tol_set", &o, s, big);
    o = good_opts(); o.lasso_tol = nan; run("lasso_tol_nan", &o, s, big);
    o = good_opts(); o.lasso_tol = 0; run("lasso_tol_0", &o, s, big);
    o = good_opts();
    s = Shape(); s.ldx = 24; run("ldx_short", &o, s, big);
    s = Shape(); s.ldm = 24; run("ldm_short", &o, s, big);
    s = Shape(); s.ldd = 24; run("ldd_short", &o, s, big);
    s = Shape(); s.ldh = 16; run("ldh_short", &o, s, big);
    s = Shape(); s.lds = 16; run("ld_s_short", &o, s, big);
    s = Shape(); s.ldq = 24; run("ld_q_short", &o, s, big);
    s = Shape(); s.ldx = 30; s.ldm = 31; s.ldd = 29; s.ldh = 20; s.lds = 19; s.ldq = 28; run("padded", &o, s, big);
    o.layout = EVC_BIN_MAJOR;
    s = Shape(); s.ldx = 70; s.ldm = 70; s.ldd = 17; s.ldh = 70; run("bin_major", &o, s, big);
    s = Shape(); s.ldx = 70; s.ldm = 69; s.ldd = 17; s.ldh = 70; run("bin_major_ldm_short", &o, s, big);
    s = Shape(); s.ldx = 70; s.ldm = 70; s.ldd = 16; s.ldh = 70; run("bin_major_ldd_short", &o, s, big);
    o = good_opts();
    s = Shape(); s.M = 0; run("M_0", &o, s, big);
    s = Shape(); s.T = 0; run("T_0", &o, s, big);
    s = Shape(); s.M = 1056; s.ldx = s.ldm = s.ldd = s.ldq = 1056; run("M_1056", &o, s, big);
    s = Shape(); s.M = 1057; s.ldx = s.ldm = s.ldd = s.ldq = 1057; run("M_1057", &o, s, big);
    run("M_1057_small_ws", &o, s, 16);
    s = Shape(); s.N = 1024; s.ldh = s.lds = 1024; run("N_1024", &o, s, big);
    run("N_1024_small_ws", &o, s, 16);
    s = Shape(); s.N = 1025; s.ldh = s.lds = 1025; run("N_1025", &o, s, big);
    s = Shape(); s.M = 256; s.ldx = s.ldm = s.ldd = s.ldq = 256; s.N = 1024; s.ldh = s.lds = 1024; run("S_at_the_limit", &o, s, big);
    s = Shape(); s.M = 257; s.ldx = s.ldm = s.ldd = s.ldq = 257; s.N = 1024; s.ldh = s.lds = 1024; run("S_beyond", &o, s, big);
    o.alpha = nan; run("nan_before_limits", &o, s, big);
    // the frame orders: -1 before the limits and the workspace are looked at
    const int good[10] = {4, 3, 2, 1, 0, 0, 2, 4, 1, 3};
    const int twice[10] = {0, 1, 2, 3, 4, 0, 1, 2, 2, 4};
    o = good_opts(); o.batch_size = 2; o.epochs = 2;
    s = Shape(); s.M = 3; s.N = 4; s.T = 5; s.ldx = s.ldm = s.ldd = s.ldq = 3; s.ldh = s.lds = 4;
    run("order_good", &o, s, 16, good);
    run("order_twice", &o, s, 16, twice);
    o.epochs = 1; run("order_first_row_only", &o, s, 16, twice);
}

int main() {
    const int shapes[][4] = {{25, 17, 70, 32}, {1, 1, 1, 1}, {201, 48, 100, 48}, {25, 1024, 2048, 256}, {1056, 504, 600, 512},
                             {256, 1024, 1030, 1024}};
    for (const auto& sh : shapes)
        for (int dtype : {EVC_F64, EVC_F32})
            for (size_t shift : {(size_t)0, (size_t)8}) carve_line(sh[0], sh[1], sh[2], sh[3], dtype, shift);
    args_lines();
    const int limits[][2] = {{1, 1}, {1056, 504}, {1056, 505}, {256, 1024}, {257, 1024}, {25, 1024}, {25, 1025}, {1057, 1},
                             {2147483647, 2147483647}};
    for (const auto& l : limits) printf("limit %d %d %d\n", l[0], l[1], pmlearn_too_large(l[0], l[1]) ? 1 : 0);
    evc_prox_masked_learn_opts o = good_opts();
    o.layout = EVC_BIN_MAJOR; o.mode = EVC_PROX_SIGNED; o.momentum = EVC_PROX_ISTA; o.lasso_iters = 7; o.lasso_check_every = 3;
    const evc_prox_masked_opts po = pmlearn_lasso_opts(o);
    printf("lasso struct_bytes %d\nlasso layout %d\nlasso iters %d\nlasso mode %d\nlasso momentum %d\nlasso normalize %d\n",
           po.struct_bytes == (int)sizeof(po) ? 1 : 0, po.layout, po.iters, po.mode, po.momentum, po.normalize);
    printf("lasso check_every %d\nlasso stop_rule %d\nlasso init_mode %d\nlasso lip_weights %d\nlasso reserved %d\n",
           po.check_every, po.stop_rule, po.init_mode, po.lip_weights, po.reserved | po.reserved2 | po.reserved3);
    printf("lasso alpha %.17g\nlasso tol %.17g\nlasso lipschitz %.17g\n", po.alpha, po.tol, po.lipschitz);
    return 0;
}
