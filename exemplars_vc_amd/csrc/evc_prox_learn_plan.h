// evc_prox_learn_plan.h - what evc_prox_learn decides on the host before and between its launches: the limits, the argument
// checks in the order of their statuses, the check of the frame orders, the block width of the atom sweep, the forgetting
// factor and the workspace carving.  No device code: tests/prox_learn_host_main.hip, a program of its own, includes it and
// runs it under the host sanitizers (tests/test_prox_learn_host.py).
#pragma once
#include "evc_prox_plan.h"

#include <stdlib.h>
#include <string.h>

namespace evc {

constexpr int PLEARN_MAX_M = 1056;         // evc_prox_solve's
constexpr int PLEARN_MAX_N = 4096;         // the statistics are N x (N + M)
constexpr int PLEARN_LDS_BYTES = 40 * 1024;        // what a block's atom changes may take of a workgroup's LDS
constexpr int PLEARN_ROWS = 32;            // rows of Rm a workgroup of k_plearn_block updates behind its block
constexpr int PLEARN_THREADS = 256;
// evc_prox_learn_opts.reserved, measurement only (tools/bench_prox_learn.py times a half of the step by leaving the others
// out): the step runs without its lasso, its statistics or its sweep.  Without the sweep there is no stop statistic.
enum { PLEARN_NO_LASSO = 1, PLEARN_NO_STATS = 2, PLEARN_NO_SWEEP = 4 };

// Block width of the right-looking atom sweep: the widest of 32, 16, 8, 4 whose atom changes (nb x M elements) stay within
// PLEARN_LDS_BYTES, so that k_plearn_block, with the block's corner of S and a tile of S beside them (8 KB each at most),
// stays inside the 64 KB of LDS a launch gets without asking for more.  float64: 32 up to M = 160, 16 up to 320, 8 up to 640,
// else 4; float32: 32 up to M = 320, 16 up to 640, else 8.  A function of M and the dtype alone: an output's bits may depend
// on it, never on the grid.
inline int plearn_block(int M, int dtype) {
    const long es = dtype == EVC_F64 ? 8 : 4;
    for (int nb = 32; nb > 4; nb >>= 1)
        if (nb * (long)M * es <= PLEARN_LDS_BYTES) return nb;
    return 4;
}

// Mairal's forgetting factor of step `count` (0, 1, ...) in double precision (dictionary_learning.py:143-144):
// theta = count bs + 1, beta = (theta - bs) / theta.  The first step's beta is negative (bs > 1) and multiplies zeros.
inline double plearn_beta(long long count, int bs) {
    const double theta = (double)count * (double)bs + 1.0;
    return (theta - (double)bs) / theta;
}

// every row of order[epochs][T] must be a permutation of 0 .. T - 1 (order == NULL: the identity, nothing to check);
// ST_OK, ST_BADARG, or hipErrorOutOfMemory when the scratch row cannot be had
inline int plearn_order_check(const int* order, int epochs, int T_) {
    if (!order || epochs == 0) return ST_OK;
    unsigned char* seen = static_cast<unsigned char*>(malloc((size_t)T_));
    if (!seen) return (int)hipErrorOutOfMemory;
    int st = ST_OK;
    for (int e = 0; e < epochs && st == ST_OK; ++e) {
        memset(seen, 0, (size_t)T_);
        const int* row = order + (size_t)e * T_;
        for (int t = 0; t < T_; ++t) {
            const int f = row[t];
            if (f < 0 || f >= T_ || seen[f]) { st = ST_BADARG; break; }
            seen[f] = 1;
        }
    }
    free(seen);
    return st;
}

struct PLearnWs {
    char* Z;            // the batch, gathered: [bs][N + M] (frame-major) or [N + M][bs] (bin-major): H_F, then X_F
    char* Rm;           // [N][M] elements: Q - S D^T, updated block by block
    char* Dw;           // [N][M] elements: the step's old dictionary, atoms as rows
    double* shares;     // [ceil(N / nb)]: a block's max |dD|
    double* stat;       // [1]
    int* ord;           // [T]: the epoch's row of `order`
    char* prox_ws;      // evc_prox_solve's workspace for a batch
    size_t prox_bytes, bytes;
};

// [Z | Rm | Dw | shares | stat | ord | the lasso's workspace], each 256-byte aligned (ws == NULL: sizes only)
inline PLearnWs carve_plearn(void* ws, int M, int N, int T_, int bs, int dtype) {
    PLearnWs w;
    Carver c = Carver::rounded(ws);
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const int nb = plearn_block(M, dtype);
    w.Z = c.take<char>(((size_t)N + M) * bs * es);
    w.Rm = c.take<char>((size_t)N * M * es);
    w.Dw = c.take<char>((size_t)N * M * es);
    w.shares = c.take<double>((size_t)(N + nb - 1) / nb);
    w.stat = c.take<double>(1);
    w.ord = c.take<int>((size_t)T_);
    w.prox_bytes = prox_workspace_bytes(M, N, bs, 1, dtype);
    w.prox_ws = c.take<char>(w.prox_bytes);
    w.bytes = c.bytes();
    return w;
}

inline size_t prox_learn_workspace_bytes(int M, int N, int T_, int batch_size, int dtype) {
    if (M < 1 || M > PLEARN_MAX_M || N < 1 || N > PLEARN_MAX_N || T_ < 1 || batch_size < 1 || batch_size > T_) return 0;
    if (dtype != EVC_F64 && dtype != EVC_F32) return 0;
    return carve_plearn(nullptr, M, N, T_, batch_size, dtype).bytes + 256;
}

// the options of a step's lasso: evc_prox_solve on the gathered batch as one utterance
inline evc_prox_opts plearn_lasso_opts(const evc_prox_learn_opts& o) {
    evc_prox_opts p;
    memset(&p, 0, sizeof(p));
    p.struct_bytes = (int)sizeof(evc_prox_opts);
    p.dtype = o.dtype; p.layout = o.layout; p.iters = o.lasso_iters; p.mode = o.mode; p.momentum = o.momentum;
    p.normalize = 1; p.check_every = o.lasso_check_every; p.stop_rule = EVC_STOP_DECOMP; p.init_mode = EVC_INIT_GIVEN;
    p.alpha = o.alpha; p.tol = o.lasso_tol;
    return p;
}

// evc_prox_learn's argument checks, in the order of its statuses: ST_BADARG, ST_UNSUPPORTED, ST_WORKSPACE before any device work
inline int plearn_args_check(const void* X, int ldx, const void* D, int ldd, const void* H, int ldh, const void* stats,
                             int ld_stats, const long long* count_io, const int* order, int M, int N, int T,
                             const evc_prox_learn_opts* opts, const void* workspace, size_t workspace_bytes) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_prox_learn_opts)) return ST_BADARG;
    const evc_prox_learn_opts& o = *opts;
    if (M < 1 || N < 1 || T < 1 || (o.dtype != EVC_F64 && o.dtype != EVC_F32)) return ST_BADARG;
    if (o.layout != EVC_FRAME_MAJOR && o.layout != EVC_BIN_MAJOR) return ST_BADARG;
    if (!X || !D || !H || !stats || !count_io || !workspace) return ST_BADARG;
    if (bad_ld(o.layout, ldx, T, M) || bad_ld(o.layout, ldd, N, M) || bad_ld(o.layout, ldh, T, N)) return ST_BADARG;
    if ((long)ld_stats < (long)N + M) return ST_BADARG;
    if (o.batch_size < 1 || o.batch_size > T || o.epochs < 0 || (o.resume != 0 && o.resume != 1)) return ST_BADARG;
    if (o.lasso_iters < 0 || o.lasso_check_every < 0 || (o.reserved & ~7) != 0 || o.reserved2 != 0) return ST_BADARG;
    if (o.mode != EVC_PROX_POSITIVE && o.mode != EVC_PROX_SIGNED) return ST_BADARG;
    if (o.momentum != EVC_PROX_ISTA && o.momentum != EVC_PROX_FISTA && o.momentum != EVC_PROX_NESTEROV) return ST_BADARG;
    if (!(o.alpha >= 0.0) || !(o.alpha - o.alpha == 0.0) || !(o.tol >= 0.0) || !(o.tol - o.tol == 0.0)) return ST_BADARG;
    if (!(o.lasso_tol >= 0.0) || !(o.lasso_tol - o.lasso_tol == 0.0)) return ST_BADARG;
    if (prox_slots(o.lasso_iters, o.lasso_check_every) > PROX_MAX_SLOTS) return ST_BADARG;
    if ((long)o.epochs * (T / o.batch_size) > 0x7fffffffL) return ST_BADARG;        // n_steps_out is an int
    if (o.resume && *count_io < 0) return ST_BADARG;
    HIP_TRY(plearn_order_check(order, o.epochs, T));
    if (M > PLEARN_MAX_M || N > PLEARN_MAX_N) return ST_UNSUPPORTED;
    if (workspace_bytes < prox_learn_workspace_bytes(M, N, T, o.batch_size, o.dtype)) return ST_WORKSPACE;
    return ST_OK;
}

}  // namespace evc
