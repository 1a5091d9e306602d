// evc_prox_learn_plan.h - what evc_prox_learn decides on the host before and between its launches: the limits, the argument
// checks in the order of their statuses, the check of the frame orders, the block width of the atom sweep, the forgetting
// factor, the workspace carving and the epoch loop.  What evc_prox_masked_learn decides alike is here once (DESIGN.md
// §5.17a): plearn_opts_ok, plearn_lasso_opts, carve_plearn_tail, plearn_loop.  No device code: tests/prox_learn_host_main.hip,
// a program of its own, includes it and runs it under the host sanitizers (tests/test_prox_learn_host.py).
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

// The epoch / batch loop of the two sparse dictionary-learning drivers, between its two events.  An epoch is `nbat` steps
// of `bs` frames in the order of its row of the caller's `order`: stage_order(e) brings that row to `ord` on the device
// (ord == NULL: the frames as they lie, nothing to stage), step(ord, t0, beta) enqueues the step on frames t0 .. t0 + bs - 1
// of that order with the forgetting factor of the running step count, which starts at *count_io and is left there.
// read_stat(&stat) evaluates max |D_new - D| of the step just enqueued and waits for it - the only synchronisation of a
// step, asked for only when somebody reads it: trace_out (NaN where not evaluated) or tol > 0, and only if the step leaves a
// statistic at all (has_stat).  stat < tol stops the call within its epoch: n_epochs is the epochs begun; a NaN compares
// false and never stops.  With both events NULL every device action is the callables'.
template <typename Opts, typename StageOrder, typename Step, typename ReadStat>
int plearn_loop(const Opts& o, int nbat, bool has_stat, const int* ord, long long* count_io, int* n_epochs_out, int* n_steps_out,
                double* trace_out, hipStream_t s, StageOrder stage_order, Step step, ReadStat read_stat) {
    const long total = (long)o.epochs * nbat;
    const bool reads = has_stat && (o.tol > 0.0 || trace_out);
    if (trace_out) for (long i = 0; i < total; ++i) trace_out[i] = __builtin_nan("");
    long long count = *count_io;
    long n_steps = 0;
    int n_epochs = o.epochs;
    bool stopped = false;
    if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
    for (int e = 0; e < o.epochs && !stopped; ++e) {
        if (ord && nbat > 0) HIP_TRY(stage_order(e));
        for (int b = 0; b < nbat && !stopped; ++b) {
            HIP_TRY(step(ord, b * o.batch_size, plearn_beta(count, o.batch_size)));
            ++count;
            ++n_steps;
            if (!reads) continue;
            double stat;
            HIP_TRY(read_stat(&stat));
            if (trace_out) trace_out[n_steps - 1] = stat;
            if (stat < o.tol) {
                stopped = true;
                n_epochs = e + 1;
            }
        }
    }
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    *count_io = count;
    if (n_steps_out) *n_steps_out = (int)n_steps;
    if (n_epochs_out) *n_epochs_out = n_epochs;
    return ST_OK;
}

// the last four arrays of both drivers' workspaces
struct PLearnTail {
    double* shares;     // [n_shares]: a block's (evc_prox_masked_learn: an atom's) max |dD|
    double* stat;       // [1]
    int* ord;           // [T]: the epoch's row of `order`
    char* prox_ws;      // the workspace of the step's lasso for a batch
    size_t prox_bytes;
};

// [shares | stat | ord | the lasso's workspace] behind what `c` has given out so far
inline PLearnTail carve_plearn_tail(Carver& c, size_t n_shares, int T_, size_t lasso_bytes) {
    PLearnTail t;
    t.shares = c.take<double>(n_shares);
    t.stat = c.take<double>(1);
    t.ord = c.take<int>((size_t)T_);
    t.prox_bytes = lasso_bytes;
    t.prox_ws = c.take<char>(lasso_bytes);
    return t;
}

struct PLearnWs : PLearnTail {
    char* Z;            // the batch, gathered: [bs][N + M] (frame-major) or [N + M][bs] (bin-major): H_F, then X_F
    char* Rm;           // [N][M] elements: Q - S D^T, updated block by block
    char* Dw;           // [N][M] elements: the step's old dictionary, atoms as rows
    size_t bytes;
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
    static_cast<PLearnTail&>(w) = carve_plearn_tail(c, (size_t)(N + nb - 1) / nb, T_, prox_workspace_bytes(M, N, bs, 1, dtype));
    w.bytes = c.bytes();
    return w;
}

inline size_t prox_learn_workspace_bytes(int M, int N, int T_, int batch_size, int dtype) {
    if (M < 1 || M > PLEARN_MAX_M || N < 1 || N > PLEARN_MAX_N || T_ < 1 || batch_size < 1 || batch_size > T_) return 0;
    if (dtype != EVC_F64 && dtype != EVC_F32) return 0;
    return carve_plearn(nullptr, M, N, T_, batch_size, dtype).bytes + 256;
}

// the options of a step's lasso: evc_prox_solve (LassoOpts = evc_prox_opts) or evc_prox_masked_solve on the gathered batch
// as one utterance
template <typename LassoOpts, typename Opts> LassoOpts plearn_lasso_opts(const Opts& o) {
    LassoOpts p;
    memset(&p, 0, sizeof(p));
    p.struct_bytes = (int)sizeof(LassoOpts);
    p.dtype = o.dtype; p.layout = o.layout; p.iters = o.lasso_iters; p.mode = o.mode; p.momentum = o.momentum;
    p.normalize = 1; p.check_every = o.lasso_check_every; p.stop_rule = EVC_STOP_DECOMP; p.init_mode = EVC_INIT_GIVEN;
    p.alpha = o.alpha; p.tol = o.lasso_tol;
    return p;
}

// the option ranges evc_prox_learn_opts and evc_prox_masked_learn_opts share, field for field, for T >= 1 frames: true, or
// false for ST_BADARG
template <typename Opts> bool plearn_opts_ok(const Opts& o, int T) {
    if ((o.dtype != EVC_F64 && o.dtype != EVC_F32) || (o.layout != EVC_FRAME_MAJOR && o.layout != EVC_BIN_MAJOR)) return false;
    if (o.batch_size < 1 || o.batch_size > T || o.epochs < 0 || (o.resume != 0 && o.resume != 1)) return false;
    if (o.lasso_iters < 0 || o.lasso_check_every < 0 || (o.reserved & ~7) != 0 || o.reserved2 != 0) return false;
    if (o.mode != EVC_PROX_POSITIVE && o.mode != EVC_PROX_SIGNED) return false;
    if (o.momentum != EVC_PROX_ISTA && o.momentum != EVC_PROX_FISTA && o.momentum != EVC_PROX_NESTEROV) return false;
    if (!(o.alpha >= 0.0) || !(o.alpha - o.alpha == 0.0) || !(o.tol >= 0.0) || !(o.tol - o.tol == 0.0)) return false;
    if (!(o.lasso_tol >= 0.0) || !(o.lasso_tol - o.lasso_tol == 0.0)) return false;
    if (prox_slots(o.lasso_iters, o.lasso_check_every) > PROX_MAX_SLOTS) return false;
    return (long)o.epochs * (T / o.batch_size) <= 0x7fffffffL;                       // n_steps_out is an int
}

// evc_prox_learn's argument checks, in the order of its statuses: ST_BADARG, ST_UNSUPPORTED, ST_WORKSPACE before any device work
inline int plearn_args_check(const void* X, int ldx, const void* D, int ldd, const void* H, int ldh, const void* stats,
                             int ld_stats, const long long* count_io, const int* order, int M, int N, int T,
                             const evc_prox_learn_opts* opts, const void* workspace, size_t workspace_bytes) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_prox_learn_opts)) return ST_BADARG;
    const evc_prox_learn_opts& o = *opts;
    if (M < 1 || N < 1 || T < 1 || !plearn_opts_ok(o, T)) return ST_BADARG;
    if (!X || !D || !H || !stats || !count_io || !workspace) return ST_BADARG;
    if (bad_ld(o.layout, ldx, T, M) || bad_ld(o.layout, ldd, N, M) || bad_ld(o.layout, ldh, T, N)) return ST_BADARG;
    if ((long)ld_stats < (long)N + M) return ST_BADARG;
    if (o.resume && *count_io < 0) return ST_BADARG;
    HIP_TRY(plearn_order_check(order, o.epochs, T));
    if (M > PLEARN_MAX_M || N > PLEARN_MAX_N) return ST_UNSUPPORTED;
    if (workspace_bytes < prox_learn_workspace_bytes(M, N, T, o.batch_size, o.dtype)) return ST_WORKSPACE;
    return ST_OK;
}

}  // namespace evc
