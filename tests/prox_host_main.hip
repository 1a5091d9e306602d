// prox_host_main.hip - a program of its own (host code only) that runs what evc_prox_solve (csrc/evc_prox_plan.h) decides on
// the host and prints it: tests/test_prox_host.py builds it, once plainly and once under the address and undefined-behaviour
// sanitizers, and checks the lines.
//   carve <M N T n_utt esize> shift <s> : <byte offsets of G, P, W0, W1, thr, tol, d, lip, partials, frame_utt, offs, stop, trace> bytes <b> query <q>
//   args <case> <status>    prox_args_check over a grid of bad and good arguments
//   waves <N T> <W>         prox_waves: the wavefronts per workgroup of k_prox_sweep, around its two thresholds
//   slots <iters check_every> <n>   prox_slots
//   mom <kind> <c_0 .. c_7>         ProxMomentum, 17 significant digits
//   loop <case> sweeps <n> checks <the iterations checked> c <c_0 ..>     prox_loop driven by fake callables: no device
#include "../exemplars_vc_amd/csrc/evc_prox_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace evc;

static void carve_line(int M, int N, int T_, int n_utt, int dtype, size_t shift) {
    std::vector<char> mem(4096);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~uintptr_t(255)) + shift;
    const ProxWs w = carve_prox(base, N, T_, n_utt, dtype);        // addresses only: nothing is dereferenced
    const char* arr[] = {w.G, w.P, w.W[0], w.W[1], w.thr, w.tolv, w.d, w.lip, reinterpret_cast<char*>(w.partials),
                         reinterpret_cast<char*>(w.frame_utt), reinterpret_cast<char*>(w.offs), reinterpret_cast<char*>(w.stop),
                         reinterpret_cast<char*>(w.trace)};
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t NP = (size_t)round_up(N, PROX_BN), nt = (size_t)N * T_ * es;
    const size_t room[] = {NP * NP * es, nt, nt, nt, (size_t)N * es, (size_t)N * es, (size_t)N * es, ((size_t)N + 1) * es,
                           NP / 64 * (size_t)T_ * 8, (size_t)T_ * 4, ((size_t)n_utt + 1) * 4, (size_t)n_utt * 4,
                           (size_t)n_utt * PROX_MAX_SLOTS * 8};
    constexpr int K = 13;
    printf("carve %d %d %d %d %zu shift %zu :", M, N, T_, n_utt, es, shift);
    for (int i = 0; i < K; ++i) {
        const size_t off = (size_t)(arr[i] - base);
        const size_t end = i < K - 1 ? (size_t)(arr[i + 1] - base) : w.bytes;
        if ((reinterpret_cast<uintptr_t>(arr[i]) & 255) != 0 || off + room[i] > end) {
            printf(" BAD");
            exit(3);
        }
        printf(" %zu", off);
    }
    const size_t need = prox_workspace_bytes(M, N, T_, n_utt, dtype);
    if (w.bytes > need) {
        printf(" BAD SIZE");
        exit(4);
    }
    printf(" bytes %zu query %zu\n", w.bytes, need);
}

static void args_lines() {
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
    auto opts = [] {
        evc_prox_opts o{};
        o.struct_bytes = (int)sizeof(o);
        o.dtype = EVC_F64; o.layout = EVC_FRAME_MAJOR; o.iters = 100;
        o.mode = EVC_PROX_POSITIVE; o.momentum = EVC_PROX_FISTA; o.normalize = 1; o.check_every = 10;
        o.stop_rule = EVC_STOP_DECOMP; o.init_mode = EVC_INIT_CONST; o.alpha = 1e-3; o.tol = 1e-3;
        return o;
    };
    const int offs_ok[] = {0, 30, 30, 70}, offs_bad[] = {0, 40, 30, 70};
    auto run = [&](const char* name, const evc_prox_opts& o, int M, int N, int T, size_t ws, const int* offs = nullptr,
                   int n_utt = 1, bool with_x = true) {
        const int st = prox_args_check(p, M, with_x ? p : nullptr, M, p, N, M, N, T, offs, n_utt, &o, p, ws);
        printf("args %s %d\n", name, st);
    };
    const size_t big = size_t(1) << 40;
    run("ok", opts(), 25, 17, 70, big);
    run("ok_exact", opts(), 25, 17, 70, prox_workspace_bytes(25, 17, 70, 1, EVC_F64));
    run("short_by_one", opts(), 25, 17, 70, prox_workspace_bytes(25, 17, 70, 1, EVC_F64) - 1);
    run("f32_ws", opts(), 25, 17, 70, prox_workspace_bytes(25, 17, 70, 1, EVC_F32));
    run("ok_utts", opts(), 25, 17, 70, big, offs_ok, 3);
    run("bad_utts", opts(), 25, 17, 70, big, offs_bad, 3);
    run("no_frames_no_x", opts(), 25, 17, 0, big, nullptr, 1, false);
    run("frames_no_x", opts(), 25, 17, 70, big, nullptr, 1, false);
    { auto o = opts(); o.struct_bytes = 4; run("struct_bytes", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = -1; run("iters_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = 0; run("iters_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = PROX_MAX_SLOTS; o.check_every = 1; run("slots_4097", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = PROX_MAX_SLOTS + 1; o.check_every = 1; run("slots_4098", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = 1000000; o.check_every = 0; run("no_checks_many_iters", o, 25, 17, 70, big); }
    { auto o = opts(); o.check_every = -1; run("check_every_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 1; run("reserved", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved2 = 1; run("reserved2", o, 25, 17, 70, big); }
    { auto o = opts(); o.mode = 2; run("mode", o, 25, 17, 70, big); }
    { auto o = opts(); o.mode = EVC_PROX_SIGNED; run("mode_signed", o, 25, 17, 70, big); }
    { auto o = opts(); o.momentum = 3; run("momentum", o, 25, 17, 70, big); }
    { auto o = opts(); o.momentum = EVC_PROX_NESTEROV; run("momentum_nesterov", o, 25, 17, 70, big); }
    { auto o = opts(); o.normalize = 2; run("normalize", o, 25, 17, 70, big); }
    { auto o = opts(); o.normalize = 0; run("normalize_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.init_mode = EVC_INIT_SKLEARN; run("init_sklearn", o, 25, 17, 70, big); }
    { auto o = opts(); o.init_mode = EVC_INIT_GIVEN; run("init_given", o, 25, 17, 70, big); }
    { auto o = opts(); o.stop_rule = EVC_STOP_SKLEARN; run("stop_sklearn", o, 25, 17, 70, big); }
    { auto o = opts(); o.stop_rule = EVC_STOP_PYMF; run("stop_pymf", o, 25, 17, 70, big); }
    { auto o = opts(); o.stop_rule = EVC_STOP_NONE; run("stop_none", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = -1e-9; run("tol_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = 0.0; run("tol_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = __builtin_inf(); run("tol_inf", o, 25, 17, 70, big); }
    { auto o = opts(); o.alpha = -1e-9; run("alpha_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.alpha = 0.0; run("alpha_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.alpha = __builtin_nan(""); run("alpha_nan", o, 25, 17, 70, big); }
    { auto o = opts(); o.lipschitz = -1.0; run("lipschitz_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.lipschitz = 3.5; run("lipschitz_set", o, 25, 17, 70, big); }
    { auto o = opts(); o.lipschitz = __builtin_inf(); run("lipschitz_inf", o, 25, 17, 70, big); }
    { auto o = opts(); o.init_value = __builtin_inf(); run("init_value_inf", o, 25, 17, 70, big); }
    { auto o = opts(); o.dtype = 7; run("dtype", o, 25, 17, 70, big); }
    { auto o = opts(); o.layout = 5; run("layout", o, 25, 17, 70, big); }
    run("M_1056", opts(), PROX_MAX_M, 17, 70, big);
    run("M_1057", opts(), PROX_MAX_M + 1, 17, 70, big);
    run("M_1057_small_ws", opts(), PROX_MAX_M + 1, 17, 70, 16);
    run("N_16384", opts(), 25, PROX_MAX_N, 70, big);
    run("N_16384_small_ws", opts(), 25, PROX_MAX_N, 70, size_t(1) << 31);
    run("N_16385", opts(), 25, PROX_MAX_N + 1, 70, big);
    run("N_16385_small_ws", opts(), 25, PROX_MAX_N + 1, 70, 16);
    { auto o = opts(); o.tol = __builtin_nan(""); run("nan_before_limits", o, PROX_MAX_M + 1, 17, 70, 16); }
    { auto o = opts(); o.reserved = 2; run("reserved_before_limits", o, 25, PROX_MAX_N + 1, 70, 16); }
}

// prox_loop with both events NULL makes no HIP call of its own: the callables below only record.  What only this program can
// see is checked here (the ping-pong of the two buffers, `partials` handed on at a check and NULL elsewhere, the check right
// behind its sweep with slot i / check_every after i + 1 updates); the printed line is checked by tests/test_prox_host.py.
template <typename Opts> static void loop_line(const char* name, int iters, int check_every, int momentum, bool live) {
    Opts o{};
    o.iters = iters; o.check_every = check_every; o.momentum = momentum;
    double w0 = 0, w1 = 0, shares = 0;
    double* Wb[2] = {&w0, &w1};
    std::vector<int> checked;
    std::vector<double> cs;
    int last = -1;
    bool ok = true;
    auto sweep = [&](int i, const double* Win, double* Wout, double* partials, double c) -> int {
        const bool due = check_every > 0 && i % check_every == 0;
        ok = ok && i == last + 1 && Win == Wb[i & 1] && Wout == Wb[(i + 1) & 1] && partials == (due ? &shares : nullptr);
        last = i;
        cs.push_back(c);
        return ST_OK;
    };
    auto check = [&](int slot, int applied) -> int {
        ok = ok && applied == last + 1 && slot * check_every == last;
        checked.push_back(last);
        return ST_OK;
    };
    const int st = prox_loop<double>(o, live, Wb, &shares, nullptr, sweep, check);
    if (st != ST_OK || !ok || (int)cs.size() != (live ? iters : 0)) {
        printf("loop %s BAD\n", name);
        exit(5);
    }
    printf("loop %s sweeps %zu checks", name, cs.size());
    for (int i : checked) printf(" %d", i);
    printf(" c");
    for (double c : cs) printf(" %.17g", c);
    printf("\n");
}

int main() {
    loop_line<evc_prox_opts>("fista_7_every_3", 7, 3, EVC_PROX_FISTA, true);
    loop_line<evc_prox_opts>("nesterov_5_every_1", 5, 1, EVC_PROX_NESTEROV, true);
    loop_line<evc_prox_opts>("ista_4_no_checks", 4, 0, EVC_PROX_ISTA, true);
    loop_line<evc_prox_masked_opts>("masked_fista_10_every_10", 10, 10, EVC_PROX_FISTA, true);
    loop_line<evc_prox_masked_opts>("masked_fista_11_every_10", 11, 10, EVC_PROX_FISTA, true);
    loop_line<evc_prox_opts>("nothing_live", 5, 1, EVC_PROX_FISTA, false);
    for (size_t shift : {size_t(0), size_t(8)}) {
        carve_line(25, 64, 32, 1, EVC_F64, shift);
        carve_line(25, 17, 70, 4, EVC_F32, shift);
        carve_line(25, 4096, 11008, 16, EVC_F64, shift);
        carve_line(1056, 16384, 688, 1, EVC_F64, shift);
        carve_line(40, 130, 0, 1, EVC_F64, shift);
        carve_line(1, 1, 1, 1, EVC_F32, shift);
    }
    args_lines();
    const int sizes[][2] = {{1, 1}, {64, 32}, {257, 5440}, {257, 5441}, {257, 10880}, {257, 10881}, {1024, 688}, {4096, 688},
                            {4096, 1024}, {4096, 11008}, {16384, 64}, {16384, 128}, {16384, 256}, {128, 2000000000}, {25, 0}};
    for (const auto& nt : sizes) printf("waves %d %d %d\n", nt[0], nt[1], prox_waves(nt[0], nt[1]));
    const int ic[][2] = {{0, 10}, {1, 10}, {10, 10}, {11, 10}, {300, 10}, {301, 10}, {5, 0}, {7, 1}, {2147483647, 1}, {2147483647, 2147483647}};
    for (const auto& c : ic) printf("slots %d %d %d\n", c[0], c[1], prox_slots(c[0], c[1]));
    for (int kind : {EVC_PROX_ISTA, EVC_PROX_FISTA, EVC_PROX_NESTEROV}) {
        ProxMomentum m(kind);
        printf("mom %d", kind);
        for (int i = 0; i < 8; ++i) printf(" %.17g", m.next(i));
        printf("\n");
    }
    return 0;
}
