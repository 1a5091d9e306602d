// prox_masked_host_main.hip - a program of its own (host code only) that runs what evc_prox_masked_solve
// (csrc/evc_prox_masked_plan.h) decides on the host and prints it: tests/test_prox_masked_host.py builds it, once plainly and
// once under the address and undefined-behaviour sanitizers, and checks the lines.
//   carve <M N T n_utt esize> shift <s> : <byte offsets of the 19 arrays in carving order> bytes <b> query <q>
//   args <case> <status>    prox_masked_args_check over a grid of bad and good arguments
//   waves <M N T> <W of k_prox_resid> <W of k_prox_back>
//   slots <iters check_every> <n>   the statistic slots (prox_slots, shared with evc_prox_solve)
//   pad <M N> <rows and columns of Dn> <rows and columns of Dm>
//   image <M N> ok          both images filled as k_pm_images fills them inside buffers of exactly the carved size, every slab
//                           load of both kernels replayed against them: in bounds, the dictionary where it belongs, zero elsewhere
#include "../exemplars_vc_amd/csrc/evc_prox_masked_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace evc;

static void carve_line(int M, int N, int T_, int n_utt, int dtype, size_t shift) {
    std::vector<char> mem(4096);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~uintptr_t(255)) + shift;
    const ProxMaskedWs w = carve_prox_masked(base, M, N, T_, n_utt, dtype);      // addresses only: nothing is dereferenced
    const char* arr[PROX_MASKED_WS_ARRAYS] = {
        w.Dn, w.Dm, w.P, w.W[0], w.W[1], w.R, w.Xm, w.lam, w.tolv, w.d, w.colsum, w.wbar, w.s, w.cf,
        reinterpret_cast<char*>(w.partials), reinterpret_cast<char*>(w.frame_utt), reinterpret_cast<char*>(w.offs),
        reinterpret_cast<char*>(w.stop), reinterpret_cast<char*>(w.trace)};
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t nt = (size_t)N * T_ * es, mt = (size_t)M * T_ * es;
    const size_t room[PROX_MASKED_WS_ARRAYS] = {
        (size_t)pm_nk(N) * pm_mp(M) * es, (size_t)pm_mk(M) * pm_np(N) * es, nt, nt, nt, mt, mt, (size_t)N * es, (size_t)N * es,
        (size_t)N * es, (size_t)n_utt * N * es, (size_t)n_utt * M * es, (size_t)n_utt * es, (size_t)T_ * es,
        (size_t)pm_np(N) / 64 * (size_t)T_ * 8, (size_t)T_ * 4, ((size_t)n_utt + 1) * 4, (size_t)n_utt * 4,
        (size_t)n_utt * PROX_MAX_SLOTS * 8};
    printf("carve %d %d %d %d %zu shift %zu :", M, N, T_, n_utt, es, shift);
    for (int i = 0; i < PROX_MASKED_WS_ARRAYS; ++i) {
        const size_t off = (size_t)(arr[i] - base);
        const size_t end = i < PROX_MASKED_WS_ARRAYS - 1 ? (size_t)(arr[i + 1] - base) : w.bytes;
        if ((reinterpret_cast<uintptr_t>(arr[i]) & 255) != 0 || off + room[i] > end) {
            printf(" BAD");
            exit(3);
        }
        printf(" %zu", off);
    }
    const size_t need = prox_masked_workspace_bytes(M, N, T_, n_utt, dtype);
    if (w.bytes > need) {
        printf(" BAD SIZE");
        exit(4);
    }
    printf(" bytes %zu query %zu\n", w.bytes, need);
}

static void args_lines() {
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
    auto opts = [] {
        evc_prox_masked_opts o{};
        o.struct_bytes = (int)sizeof(o);
        o.dtype = EVC_F64; o.layout = EVC_FRAME_MAJOR; o.iters = 100;
        o.mode = EVC_PROX_POSITIVE; o.momentum = EVC_PROX_FISTA; o.normalize = 1; o.check_every = 10;
        o.stop_rule = EVC_STOP_DECOMP; o.init_mode = EVC_INIT_CONST; o.lip_weights = EVC_PROX_LIP_MEAN; o.alpha = 1e-3;
        o.tol = 1e-3;
        return o;
    };
    const int offs_ok[] = {0, 30, 30, 70}, offs_bad[] = {0, 40, 30, 70};
    auto run = [&](const char* name, const evc_prox_masked_opts& o, int M, int N, int T, size_t ws, const int* offs = nullptr,
                   int n_utt = 1, bool with_x = true, bool with_mask = true, int ldm = -1) {
        const int st = prox_masked_args_check(p, M, with_x ? p : nullptr, M, with_mask ? p : nullptr, ldm < 0 ? M : ldm, p, N, M,
                                              N, T, offs, n_utt, &o, p, ws);
        printf("args %s %d\n", name, st);
    };
    const size_t big = size_t(1) << 40;
    run("ok", opts(), 25, 17, 70, big);
    run("ok_exact", opts(), 25, 17, 70, prox_masked_workspace_bytes(25, 17, 70, 1, EVC_F64));
    run("short_by_one", opts(), 25, 17, 70, prox_masked_workspace_bytes(25, 17, 70, 1, EVC_F64) - 1);
    run("f32_ws", opts(), 25, 17, 70, prox_masked_workspace_bytes(25, 17, 70, 1, EVC_F32));
    run("ok_utts", opts(), 25, 17, 70, big, offs_ok, 3);
    run("bad_utts", opts(), 25, 17, 70, big, offs_bad, 3);
    run("no_frames_no_x", opts(), 25, 17, 0, big, nullptr, 1, false);
    run("frames_no_x", opts(), 25, 17, 70, big, nullptr, 1, false);
    run("no_mask", opts(), 25, 17, 70, big, nullptr, 1, true, false);
    run("no_mask_any_ldm", opts(), 25, 17, 70, big, nullptr, 1, true, false, 0);
    run("ldm_short", opts(), 25, 17, 70, big, nullptr, 1, true, true, 24);
    run("ldm_padded", opts(), 25, 17, 70, big, nullptr, 1, true, true, 31);
    { auto o = opts(); o.layout = EVC_BIN_MAJOR; run("ldm_short_bin_major", o, 70, 70, 70, big, nullptr, 1, true, true, 69); }
    { auto o = opts(); o.struct_bytes = (int)sizeof(evc_prox_opts); run("struct_bytes", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = -1; run("iters_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = 0; run("iters_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = PROX_MAX_SLOTS; o.check_every = 1; run("slots_4097", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = PROX_MAX_SLOTS + 1; o.check_every = 1; run("slots_4098", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = 1000000; o.check_every = 0; run("no_checks_many_iters", o, 25, 17, 70, big); }
    { auto o = opts(); o.check_every = -1; run("check_every_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 1; run("reserved", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved2 = 1; run("reserved2", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved3 = 1; run("reserved3", o, 25, 17, 70, big); }
    { auto o = opts(); o.lip_weights = 2; run("lip_weights", o, 25, 17, 70, big); }
    { auto o = opts(); o.lip_weights = -1; run("lip_weights_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.lip_weights = EVC_PROX_LIP_MAX; run("lip_weights_max", o, 25, 17, 70, big); }
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
    run("N_16384_small_ws", opts(), 25, PROX_MAX_N, 70, size_t(1) << 20);
    run("N_16385", opts(), 25, PROX_MAX_N + 1, 70, big);
    run("N_16385_small_ws", opts(), 25, PROX_MAX_N + 1, 70, 16);
    { auto o = opts(); o.tol = __builtin_nan(""); run("nan_before_limits", o, PROX_MAX_M + 1, 17, 70, 16); }
    { auto o = opts(); o.reserved3 = 2; run("reserved_before_limits", o, 25, PROX_MAX_N + 1, 70, 16); }
    { auto o = opts(); o.lip_weights = 7; run("lip_weights_before_limits", o, PROX_MAX_M + 1, 17, 70, 16); }
    run("ldm_before_limits", opts(), PROX_MAX_M + 1, 17, 70, 16, nullptr, 1, true, true, 25);
}

// The two images as k_pm_images fills them (Dn[n][m] = Dm[m][n] = the dictionary, zero elsewhere), inside vectors of exactly
// the carved size: the sanitizer sees any slab load of k_prox_resid (rows k of Dn, columns of a 16 W-bin block) or k_prox_back
// (rows k of Dm, columns of a 16 W-exemplar block) that leaves them, for both workgroup widths.
static void image_line(int M, int N) {
    const int NK = pm_nk(N), MP = pm_mp(M), MK = pm_mk(M), NP = pm_np(N);
    std::vector<double> Dn((size_t)NK * MP, 0.0), Dm((size_t)MK * NP, 0.0);
    for (int n = 0; n < N; ++n)
        for (int m = 0; m < M; ++m) Dn.at((size_t)n * MP + m) = Dm.at((size_t)m * NP + n) = 1.0 + n + 1e-3 * m;
    auto replay = [&](const std::vector<double>& D, int ldd, int K, int rows, bool transposed) {
        for (int W : {4, 8}) {
            const int BN = 16 * W, blocks = (rows + BN - 1) / BN, NS = (K + PROX_KS - 1) / PROX_KS;
            for (int by = 0; by < blocks; ++by)
                for (int sl = 0; sl < NS; ++sl)
                    for (int tid = 0; tid < 64 * W; ++tid) {
                        const int g_row = tid / (4 * W), g_col = (tid % (4 * W)) * 4;
                        for (int e = 0; e < 4; ++e) {
                            const int k = sl * PROX_KS + g_row, r = by * BN + g_col + e;
                            const double v = D.at((size_t)k * ldd + r);           // throws when out of range
                            const double want = (k < K && r < rows) ? (transposed ? 1.0 + r + 1e-3 * k : 1.0 + k + 1e-3 * r) : 0.0;
                            if (v != want) {
                                printf("image %d %d BAD\n", M, N);
                                exit(5);
                            }
                        }
                    }
        }
    };
    replay(Dn, MP, N, M, false);       // k = n, row = m
    replay(Dm, NP, M, N, true);        // k = m, row = n
    printf("pad %d %d %d %d %d %d\n", M, N, NK, MP, MK, NP);
    printf("image %d %d ok\n", M, N);
}

int main() {
    for (size_t shift : {size_t(0), size_t(8)}) {
        carve_line(25, 64, 32, 1, EVC_F64, shift);
        carve_line(25, 17, 70, 4, EVC_F32, shift);
        carve_line(25, 4096, 11008, 16, EVC_F64, shift);
        carve_line(1056, 16384, 688, 1, EVC_F64, shift);
        carve_line(40, 130, 0, 1, EVC_F64, shift);
        carve_line(1, 1, 1, 1, EVC_F32, shift);
    }
    args_lines();
    const int sizes[][3] = {{1, 1, 1}, {25, 64, 32}, {25, 4096, 688}, {25, 4096, 11008}, {201, 4096, 11008}, {513, 4096, 11008},
                            {1056, 16384, 64}, {25, 257, 10881}, {25, 130, 0}};
    for (const auto& z : sizes) printf("waves %d %d %d %d %d\n", z[0], z[1], z[2], pm_resid_waves(z[0], z[2]), pm_back_waves(z[1], z[2]));
    const int ic[][2] = {{0, 10}, {1, 10}, {10, 10}, {11, 10}, {300, 10}, {301, 10}, {5, 0}, {7, 1}, {4097, 1}, {40970, 10}};
    for (const auto& c : ic) printf("slots %d %d %d\n", c[0], c[1], prox_slots(c[0], c[1]));
    for (int M : {1, 15, 16, 17, 128, 129})
        for (int N : {1, 15, 16, 17, 128, 129}) image_line(M, N);
    return 0;
}
