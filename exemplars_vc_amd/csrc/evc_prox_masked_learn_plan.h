// evc_prox_masked_learn_plan.h - what evc_prox_masked_learn decides on the host before and between its launches: the limits,
// the argument checks in the order of their statuses and the workspace carving.  The forgetting factor and the check of the
// frame orders are evc_prox_learn's (evc_prox_learn_plan.h), the lasso's workspace evc_prox_masked_solve's
// (evc_prox_masked_plan.h).  No device code: tests/prox_masked_learn_host_main.hip, a program of its own, includes it and runs
// it under the host sanitizers (tests/test_prox_masked_learn_host.py).
#pragma once
#include "evc_prox_learn_plan.h"
#include "evc_prox_masked_plan.h"

namespace evc {

constexpr int PMLEARN_MAX_M = 1056;                 // evc_prox_masked_solve's
constexpr int PMLEARN_MAX_N = 1024;                 // the statistics are M planes of N x N
constexpr long PMLEARN_MAX_S = 1L << 28;            // elements of those planes together, M N^2
constexpr int PMLEARN_MAX_BINS = (PMLEARN_MAX_M + PLEARN_THREADS - 1) / PLEARN_THREADS;     // bins per thread of k_pmlearn_atoms
// evc_prox_masked_learn_opts.reserved, measurement only (tools/bench_prox_masked_learn.py): evc_prox_learn's three bits, the
// third leaving the atom update out (and with it the stop statistic)
enum { PMLEARN_NO_LASSO = PLEARN_NO_LASSO, PMLEARN_NO_STATS = PLEARN_NO_STATS, PMLEARN_NO_ATOMS = PLEARN_NO_SWEEP };

inline bool pmlearn_too_large(int M, int N) {
    return M > PMLEARN_MAX_M || N > PMLEARN_MAX_N || (long)M * N * N > PMLEARN_MAX_S;
}

struct PMLearnWs : PLearnTail {
    char* Z;            // the batch, gathered: [bs][N + 2 M] (frame-major) or [N + 2 M][bs] (bin-major): H_F, X_F, then W_F
    char* G;            // [N][M] elements: G[k][m] = sum_j S_m[k][j] D_old[j][m]
    char* diag;         // [M][N] elements: S_m[k][k]
    char* Dt;           // [M][N] elements: the dictionary, a bin per row (what k_pmlearn_stats reads along j)
    size_t bytes;       // (PLearnTail: a share per atom; the lasso's workspace is evc_prox_masked_solve's)
};
constexpr int PMLEARN_WS_ARRAYS = 8;

// [Z | G | diag | Dt | shares | stat | ord | the lasso's workspace], each 256-byte aligned (ws == NULL: sizes only)
inline PMLearnWs carve_pmlearn(void* ws, int M, int N, int T_, int bs, int dtype) {
    PMLearnWs w;
    Carver c = Carver::rounded(ws);
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    w.Z = c.take<char>(((size_t)N + 2 * (size_t)M) * bs * es);
    w.G = c.take<char>((size_t)N * M * es);
    w.diag = c.take<char>((size_t)N * M * es);
    w.Dt = c.take<char>((size_t)N * M * es);
    static_cast<PLearnTail&>(w) = carve_plearn_tail(c, (size_t)N, T_, prox_masked_workspace_bytes(M, N, bs, 1, dtype));
    w.bytes = c.bytes();
    return w;
}

inline size_t prox_masked_learn_workspace_bytes(int M, int N, int T_, int batch_size, int dtype) {
    if (M < 1 || N < 1 || pmlearn_too_large(M, N) || T_ < 1 || batch_size < 1 || batch_size > T_) return 0;
    if (dtype != EVC_F64 && dtype != EVC_F32) return 0;
    return carve_pmlearn(nullptr, M, N, T_, batch_size, dtype).bytes + 256;
}

// the options of a step's lasso: evc_prox_masked_solve on the gathered batch as one utterance, deComP's step
inline evc_prox_masked_opts pmlearn_lasso_opts(const evc_prox_masked_learn_opts& o) {
    evc_prox_masked_opts p = plearn_lasso_opts<evc_prox_masked_opts>(o);
    p.lip_weights = EVC_PROX_LIP_MEAN;
    return p;
}

// evc_prox_masked_learn's argument checks, in the order of its statuses: ST_BADARG, ST_UNSUPPORTED, ST_WORKSPACE before any
// device work
inline int pmlearn_args_check(const void* X, int ldx, const void* mask, int ldm, const void* D, int ldd, const void* H, int ldh,
                              const void* stats_s, int ld_s, const void* stats_q, int ld_q, const long long* count_io,
                              const int* order, int M, int N, int T, const evc_prox_masked_learn_opts* opts,
                              const void* workspace, size_t workspace_bytes) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_prox_masked_learn_opts)) return ST_BADARG;
    const evc_prox_masked_learn_opts& o = *opts;
    if (M < 1 || N < 1 || T < 1 || !plearn_opts_ok(o, T)) return ST_BADARG;
    if (!X || !mask || !D || !H || !stats_s || !stats_q || !count_io || !workspace) return ST_BADARG;
    if (bad_ld(o.layout, ldx, T, M) || bad_ld(o.layout, ldm, T, M) || bad_ld(o.layout, ldd, N, M) || bad_ld(o.layout, ldh, T, N))
        return ST_BADARG;
    if (ld_s < N || ld_q < M) return ST_BADARG;
    if (o.resume && *count_io < 0) return ST_BADARG;
    HIP_TRY(plearn_order_check(order, o.epochs, T));
    if (pmlearn_too_large(M, N)) return ST_UNSUPPORTED;
    if (workspace_bytes < prox_masked_learn_workspace_bytes(M, N, T, o.batch_size, o.dtype)) return ST_WORKSPACE;
    return ST_OK;
}

}  // namespace evc
