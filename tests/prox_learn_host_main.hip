// prox_learn_host_main.hip - a program of its own (host code only) that runs what evc_prox_learn
// (csrc/evc_prox_learn_plan.h) decides on the host and prints it: tests/test_prox_learn_host.py builds it, once plainly and once
// under the address and undefined-behaviour sanitizers, and checks the lines.
//   carve <M N T bs esize> shift <s> : <byte offsets of the 7 arrays in carving order> bytes <b> query <q>
//   args <case> <status>     plearn_args_check over a grid of bad and good arguments
//   block <M> <esize> <nb>   plearn_block, with the LDS bytes of k_plearn_block at that width
//   beta <count> <bs> <beta> plearn_beta, 17 significant digits
//   order <case> <status>    plearn_order_check
//   loop <case> n_epochs <e> n_steps <n> count <count_io afterwards> staged <epochs whose order row was staged> reads <calls
//        of read_stat> t0 <the steps' first frames> trace <trace_out>      plearn_loop driven by fake callables: no device
#include "../exemplars_vc_amd/csrc/evc_prox_learn_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace evc;

static void carve_line(int M, int N, int T_, int bs, int dtype, size_t shift) {
    std::vector<char> mem(4096);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~uintptr_t(255)) + shift;
    const PLearnWs w = carve_plearn(base, M, N, T_, bs, dtype);      // addresses only: nothing is dereferenced
    const char* arr[7] = {w.Z, w.Rm, w.Dw, reinterpret_cast<char*>(w.shares), reinterpret_cast<char*>(w.stat),
                          reinterpret_cast<char*>(w.ord), w.prox_ws};
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const int nb = plearn_block(M, dtype);
    const size_t room[7] = {((size_t)N + M) * bs * es, (size_t)N * M * es, (size_t)N * M * es, (size_t)((N + nb - 1) / nb) * 8, 8,
                            (size_t)T_ * 4, prox_workspace_bytes(M, N, bs, 1, dtype)};
    const char* first = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(base) + 255) & ~uintptr_t(255));
    printf("carve %d %d %d %d %zu shift %zu :", M, N, T_, bs, es, shift);
    for (int i = 0; i < 7; ++i) {
        const size_t off = (size_t)(arr[i] - base);
        const size_t end = i < 6 ? (size_t)(arr[i + 1] - base) : w.bytes;
        if ((reinterpret_cast<uintptr_t>(arr[i]) & 255) != 0 || off + room[i] > end || arr[i] < first) {
            printf(" BAD");
            exit(3);
        }
        printf(" %zu", off);
    }
    const size_t need = prox_learn_workspace_bytes(M, N, T_, bs, dtype);
    if (w.bytes > need || room[6] == 0) {
        printf(" BAD SIZE");
        exit(4);
    }
    printf(" bytes %zu query %zu\n", w.bytes, need);
}

static void args_lines() {
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
    long long count = 0;
    auto opts = [] {
        evc_prox_learn_opts o{};
        o.struct_bytes = (int)sizeof(o);
        o.dtype = EVC_F64; o.layout = EVC_FRAME_MAJOR; o.batch_size = 32; o.epochs = 3; o.lasso_iters = 10;
        o.lasso_check_every = 10; o.mode = EVC_PROX_POSITIVE; o.momentum = EVC_PROX_FISTA; o.alpha = 1e-3; o.lasso_tol = 1e-5;
        return o;
    };
    struct Shape { int M = 25, N = 17, T = 70, ldx = 25, ldd = 25, ldh = 17, lds = 42; };
    const size_t big = (size_t)1 << 40;
    auto run = [&](const char* name, const evc_prox_learn_opts* o, Shape s, size_t ws, const int* order = nullptr,
                   const void* X = reinterpret_cast<const void*>(uintptr_t(256)), const void* cnt = nullptr) {
        const long long* c = cnt ? static_cast<const long long*>(cnt) : &count;
        printf("args %s %d\n", name, plearn_args_check(X, s.ldx, p, s.ldd, p, s.ldh, p, s.lds, c, order, s.M, s.N, s.T, o, p, ws));
    };
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    evc_prox_learn_opts o = opts();
    Shape s;
    run("ok", &o, s, big);
    run("ok_exact", &o, s, prox_learn_workspace_bytes(25, 17, 70, 32, EVC_F64));
    run("short_by_one", &o, s, prox_learn_workspace_bytes(25, 17, 70, 32, EVC_F64) - 1);
    run("no_opts", nullptr, s, big);
    run("no_x", &o, s, big, nullptr, nullptr);
    o = opts(); o.struct_bytes -= 8; run("struct_bytes", &o, s, big);
    o = opts(); o.dtype = 2; run("dtype", &o, s, big);
    o = opts(); o.layout = 2; run("layout", &o, s, big);
    o = opts(); o.batch_size = 0; run("batch_0", &o, s, big);
    o = opts(); o.batch_size = 70; run("batch_T", &o, s, big);
    o = opts(); o.batch_size = 71; run("batch_T_plus_1", &o, s, big);
    o = opts(); o.epochs = -1; run("epochs_neg", &o, s, big);
    o = opts(); o.epochs = 0; run("epochs_0", &o, s, big);
    o = opts(); o.epochs = 0x7fffffff; o.batch_size = 1; run("steps_beyond_int", &o, s, big);
    o = opts(); o.lasso_iters = -1; run("lasso_iters_neg", &o, s, big);
    o = opts(); o.lasso_iters = 0; run("lasso_iters_0", &o, s, big);
    o = opts(); o.lasso_iters = 4098; o.lasso_check_every = 1; run("slots_4098", &o, s, big);
    o = opts(); o.lasso_iters = 4097; o.lasso_check_every = 1; run("slots_4097", &o, s, big);
    o = opts(); o.lasso_check_every = -1; run("check_every_neg", &o, s, big);
    o = opts(); o.mode = 2; run("mode", &o, s, big);
    o = opts(); o.mode = EVC_PROX_SIGNED; run("mode_signed", &o, s, big);
    o = opts(); o.momentum = 3; run("momentum", &o, s, big);
    o = opts(); o.momentum = EVC_PROX_NESTEROV; run("momentum_nesterov", &o, s, big);
    o = opts(); o.resume = 2; run("resume_2", &o, s, big);
    o = opts(); o.resume = 1; run("resume_1", &o, s, big);
    { long long neg = -1; o = opts(); o.resume = 1; run("resume_count_neg", &o, s, big, nullptr, p, &neg);
      o = opts(); run("fresh_count_neg", &o, s, big, nullptr, p, &neg); }
    o = opts(); o.reserved = 8; run("reserved", &o, s, big);
    o = opts(); o.reserved = 7; run("reserved_halves_off", &o, s, big);
    o = opts(); o.reserved2 = 1; run("reserved2", &o, s, big);
    o = opts(); o.alpha = -1; run("alpha_neg", &o, s, big);
    o = opts(); o.alpha = nan; run("alpha_nan", &o, s, big);
    o = opts(); o.alpha = 0; run("alpha_0", &o, s, big);
    o = opts(); o.tol = -1; run("tol_neg", &o, s, big);
    o = opts(); o.tol = inf; run("tol_inf", &o, s, big);
    o = opts(); o.tol = 1e-3; run("tol_set", &o, s, big);
    o = opts(); o.lasso_tol = nan; run("lasso_tol_nan", &o, s, big);
    o = opts(); o.lasso_tol = 0; run("lasso_tol_0", &o, s, big);
    o = opts();
    s = Shape(); s.ldx = 24; run("ldx_short", &o, s, big);
    s = Shape(); s.ldd = 24; run("ldd_short", &o, s, big);
    s = Shape(); s.ldh = 16; run("ldh_short", &o, s, big);
    s = Shape(); s.lds = 41; run("ld_stats_short", &o, s, big);
    s = Shape(); s.ldx = 30; s.ldd = 29; s.ldh = 20; s.lds = 50; run("padded", &o, s, big);
    o.layout = EVC_BIN_MAJOR;
    s = Shape(); s.ldx = 70; s.ldd = 17; s.ldh = 70; run("bin_major", &o, s, big);
    s = Shape(); s.ldx = 69; s.ldd = 17; s.ldh = 70; run("bin_major_ldx_short", &o, s, big);
    s = Shape(); s.ldx = 70; s.ldd = 16; s.ldh = 70; run("bin_major_ldd_short", &o, s, big);
    o = opts();
    s = Shape(); s.M = 0; run("M_0", &o, s, big);
    s = Shape(); s.T = 0; run("T_0", &o, s, big);
    s = Shape(); s.M = 1056; s.ldx = s.ldd = 1056; s.lds = 1056 + 17; run("M_1056", &o, s, big);
    s = Shape(); s.M = 1057; s.ldx = s.ldd = 1057; s.lds = 1057 + 17; run("M_1057", &o, s, big);
    run("M_1057_small_ws", &o, s, 16);
    s = Shape(); s.N = 4096; s.ldh = 4096; s.lds = 4096 + 25; run("N_4096", &o, s, big);
    run("N_4096_small_ws", &o, s, 16);
    s = Shape(); s.N = 4097; s.ldh = 4097; s.lds = 4097 + 25; run("N_4097", &o, s, big);
    o.alpha = nan; run("nan_before_limits", &o, s, big);
}

static void order_lines() {
    const int T_ = 5;
    const int good[10] = {4, 3, 2, 1, 0, 0, 2, 4, 1, 3};
    const int twice[10] = {0, 1, 2, 3, 4, 0, 1, 2, 2, 4};
    const int beyond[5] = {0, 1, 2, 3, 5};
    const int negative[5] = {0, -1, 2, 3, 4};
    printf("order null %d\n", plearn_order_check(nullptr, 2, T_));
    printf("order good %d\n", plearn_order_check(good, 2, T_));
    printf("order twice_in_second_row %d\n", plearn_order_check(twice, 2, T_));
    printf("order first_row_only %d\n", plearn_order_check(twice, 1, T_));
    printf("order beyond %d\n", plearn_order_check(beyond, 1, T_));
    printf("order negative %d\n", plearn_order_check(negative, 1, T_));
    printf("order no_epochs %d\n", plearn_order_check(beyond, 0, T_));
    // ... and through the argument check: -1 before the limits and the workspace are looked at
    evc_prox_learn_opts o{};
    o.struct_bytes = (int)sizeof(o);
    o.dtype = EVC_F64; o.layout = EVC_FRAME_MAJOR; o.batch_size = 2; o.epochs = 2; o.lasso_iters = 10; o.lasso_check_every = 10;
    o.alpha = 1e-3;
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));
    long long count = 0;
    printf("order args_good %d\n", plearn_args_check(p, 3, p, 3, p, 4, p, 7, &count, good, 3, 4, T_, &o, p, 16));
    printf("order args_twice %d\n", plearn_args_check(p, 3, p, 3, p, 4, p, 7, &count, twice, 3, 4, T_, &o, p, 16));
}

// plearn_loop with both events NULL makes no HIP call of its own: the callables below only record.  The statistic of the
// k-th read (1, 2, ...) is 1 + 1 / k, but 0 at read `stop_at`.  What only this program can see is checked here (the order
// pointer handed on, beta = plearn_beta of the running count to the bit, the element behind the trace untouched); the
// printed line is checked by tests/test_prox_learn_host.py.
static void loop_line(const char* name, int epochs, int nbat, int bs, double tol, bool has_stat, bool with_order, bool with_trace,
                      long long count0, int stop_at) {
    evc_prox_learn_opts o{};
    o.epochs = epochs; o.batch_size = bs; o.tol = tol;
    static const int device_row = 0;            // stands for the staged row: never dereferenced
    const int* ord = with_order ? &device_row : nullptr;
    const long total = (long)epochs * nbat;
    std::vector<double> trace((size_t)total + 1, -5.0);
    std::vector<int> staged, t0s;
    long long count = count0;
    int n_epochs = -1, n_steps = -1, reads = 0;
    bool ok = true;
    auto stage_order = [&](int e) -> int { staged.push_back(e); return ST_OK; };
    auto step = [&](const int* got, int t0, double beta) -> int {
        ok = ok && got == ord && beta == plearn_beta(count0 + (long long)t0s.size(), bs);
        t0s.push_back(t0);
        return ST_OK;
    };
    auto read_stat = [&](double* stat) -> int { ++reads; *stat = reads == stop_at ? 0.0 : 1.0 + 1.0 / reads; return ST_OK; };
    const int st = plearn_loop(o, nbat, has_stat, ord, &count, &n_epochs, &n_steps, with_trace ? trace.data() : nullptr, nullptr,
                               stage_order, step, read_stat);
    if (st != ST_OK || !ok || trace[(size_t)total] != -5.0) {
        printf("loop %s BAD\n", name);
        exit(5);
    }
    printf("loop %s n_epochs %d n_steps %d count %lld staged", name, n_epochs, n_steps, count);
    for (int e : staged) printf(" %d", e);
    printf(" reads %d t0", reads);
    for (int t : t0s) printf(" %d", t);
    printf(" trace");
    for (long i = 0; with_trace && i < total; ++i) printf(" %.17g", trace[(size_t)i]);
    printf("\n");
}

int main() {
    loop_line("stop_at_step_2_of_epoch_1", 4, 3, 8, 0.5, true, true, true, 0, 5);
    loop_line("tol_0_with_a_trace", 2, 2, 8, 0.0, true, false, true, 0, 3);
    loop_line("no_trace_no_tol", 2, 3, 8, 0.0, true, true, false, 0, 0);
    loop_line("tol_without_a_trace", 3, 2, 8, 0.5, true, false, false, 0, 2);
    loop_line("no_statistic", 2, 2, 8, 0.5, false, true, true, 0, 1);
    loop_line("epochs_0", 0, 3, 8, 0.5, true, true, true, 4, 0);
    loop_line("nbat_0", 3, 0, 8, 0.5, true, true, true, 4, 0);
    loop_line("resumed_count", 1, 2, 32, 0.0, true, true, true, 7, 0);
    const int shapes[][4] = {{25, 17, 70, 32}, {1, 1, 1, 1}, {201, 96, 150, 64}, {50, 4096, 2048, 1024}, {1056, 4096, 4096, 4096},
                             {402, 1024, 1030, 1024}};
    for (const auto& sh : shapes)
        for (int dtype : {EVC_F64, EVC_F32})
            for (size_t shift : {(size_t)0, (size_t)8}) carve_line(sh[0], sh[1], sh[2], sh[3], dtype, shift);
    args_lines();
    for (int M : {1, 25, 160, 161, 201, 320, 321, 402, 640, 641, 1056})
        for (int dtype : {EVC_F64, EVC_F32}) {
            const int nb = plearn_block(M, dtype);
            const size_t es = dtype == EVC_F64 ? 8 : 4;
            printf("block %d %zu %d %zu\n", M, es, nb, ((size_t)nb * M + (size_t)nb * nb + (size_t)PLEARN_ROWS * nb) * es);
        }
    for (long long count : {0LL, 1LL, 2LL, 217LL, 1000000LL})
        for (int bs : {1, 32, 1024}) printf("beta %lld %d %.17g\n", count, bs, plearn_beta(count, bs));
    order_lines();
    return 0;
}
