// evc_prox_plan.h - what evc_prox_solve decides on the host before and between its launches: the limits, the argument checks
// in the order of their statuses, the workspace carving, the momentum schedule and the iteration loop.  What
// evc_prox_masked_solve decides alike is here once: prox_opts_ok, carve_prox_tail, prox_loop.  No device
// code: tests/prox_host_main.hip, a program of its own, includes it and runs it under the host sanitizers
// (tests/test_prox_host.py).
#pragma once
#include "evc_internal.h"

#include <cmath>

namespace evc {

constexpr int PROX_MAX_M = 1056;       // as evc_semi_solve: M is only a contraction length here
constexpr int PROX_MAX_N = 16384;      // the Gram matrix is N x N: 2 GiB in float64 at this N
constexpr int PROX_MAX_SLOTS = 4097;   // statistic slots per utterance (evc_semi_solve's cap)
constexpr int PROX_MAX_WAVES = 8;      // wavefronts per workgroup of k_prox_sweep, each owning 16 exemplar rows
constexpr int PROX_BN = 128;           // exemplar rows of the widest workgroup; G is padded to a multiple in both directions
constexpr int PROX_BT = 64;            // frame columns per workgroup
constexpr int PROX_KS = 16;            // exemplars per k-slab

// Wavefronts (row tiles of 16) per workgroup of k_prox_sweep: 8 where that already gives the chip two workgroups per compute
// unit (512 on 256), else 4 - k_semi_sweep's rule (evc_semi_plan.h), whose geometry this kernel shares.  A function of the
// sizes alone, never of the device; an output's sum does not depend on it (every wavefront runs the same k-ascending chain
// over all of N).
constexpr int PROX_FILL_WGS = 512;
inline int prox_waves(int N, int T_) {
    const long frame_blocks = ((long)T_ + PROX_BT - 1) / PROX_BT, NP = round_up(N, PROX_BN);
    return frame_blocks * (NP / PROX_BN) >= PROX_FILL_WGS ? PROX_MAX_WAVES : PROX_MAX_WAVES / 2;
}

// the checks run at iterations 0, check_every, 2 check_every, ... < iters: one statistic slot each
inline int prox_slots(int iters, int check_every) { return (check_every > 0 && iters > 0) ? (iters - 1) / check_every + 1 : 0; }

// The momentum schedule, in double precision on the host: c_i of W' = X_new + c_i (X_new - X_old).
//   ISTA      0
//   FISTA     beta_(i+1) = (1 + sqrt(1 + 4 beta_i^2)) / 2, c_i = (beta_i - 1) / beta_(i+1), beta_0 = 1   (lasso.py:411-412)
//   NESTEROV  i / (i + 3)                                                                                (lasso.py:353)
struct ProxMomentum {
    int kind;
    double beta = 1.0;
    explicit ProxMomentum(int k) : kind(k) {}
    double next(int i) {                   // call with i = 0, 1, 2, ... in order
        if (kind == EVC_PROX_NESTEROV) return (double)i / ((double)i + 3.0);
        if (kind != EVC_PROX_FISTA) return 0.0;
        const double beta_new = 0.5 * (1.0 + std::sqrt(1.0 + 4.0 * beta * beta));
        const double c = (beta - 1.0) / beta_new;
        beta = beta_new;
        return c;
    }
};

// The iteration loop of the two proximal-gradient drivers, between its two events (recorded also when nothing is `live`: no
// frames or no iterations).  Iteration i reads Wb[i & 1] and writes the other; the checks run at i = 0, check_every,
// 2 check_every, ...  sweep(i, Win, Wout, partials, c) enqueues the driver's update with the momentum coefficient c_i, and
// leaves the shares of the stop statistic in `partials` on a check iteration, where it is not NULL; check(slot, applied) then
// enqueues k_prox_check after applied = i + 1 updates.  Apart from the events every device action is the callables'.
template <typename T, typename Opts, typename Sweep, typename Check>
int prox_loop(const Opts& o, bool live, T* const Wb[2], double* partials, hipStream_t s, Sweep sweep, Check check) {
    if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
    if (live) {
        ProxMomentum mom(o.momentum);
        for (int i = 0; i < o.iters; ++i) {
            const bool checked = o.check_every > 0 && i % o.check_every == 0;
            HIP_TRY(sweep(i, (const T*)Wb[i & 1], Wb[(i + 1) & 1], checked ? partials : nullptr, (T)mom.next(i)));
            if (checked) HIP_TRY(check(i / o.check_every, i + 1));
        }
    }
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    return ST_OK;
}

// the last five arrays of both drivers' workspaces
struct ProxTail {
    double* partials;   // [NP / 64][T], NP = round_up(N, PROX_BN): max over a row block of |X_new - X_old| - tol_n, per frame
    int* frame_utt;     // [T]
    int* offs;          // [n_utt + 1]
    int* stop;          // [n_utt]: 0 running, else the updates applied when the utterance stopped
    double* trace;      // [n_utt][PROX_MAX_SLOTS]
};

// [partials | frame_utt | offs | stop | trace] behind what `c` has given out so far
inline ProxTail carve_prox_tail(Carver& c, int N, int T_, int n_utt) {
    ProxTail t;
    t.partials = c.take<double>((size_t)round_up(N, PROX_BN) / 64 * (size_t)T_);
    t.frame_utt = c.take<int>((size_t)T_);
    t.offs = c.take<int>((size_t)n_utt + 1);
    t.stop = c.take<int>((size_t)n_utt);
    t.trace = c.take<double>((size_t)n_utt * PROX_MAX_SLOTS);
    return t;
}

struct ProxWs : ProxTail {
    char* G;            // [NP][NP] elements, NP = round_up(N, PROX_BN): A^T A (scaled), zero in the padding
    char* P;            // [N][T] elements: A^T X (scaled)
    char* W[2];         // [N][T] elements each: the extrapolated point, read from one and written to the other
    char* thr;          // [N] elements: s lambda_n
    char* tolv;         // [N] elements: tol_n
    char* d;            // [N] elements: sqrt(G_nn), or 1
    char* lip;          // [1 + N] elements: s = 1 / L, then the Gershgorin column sums
    size_t bytes;
};

// [G | P | W0 | W1 | thr | tol | d | lip | partials | frame_utt | offs | stop | trace], each 256-byte aligned
// (ws == NULL: sizes only)
inline ProxWs carve_prox(void* ws, int N, int T_, int n_utt, int dtype) {
    ProxWs w;
    Carver c = Carver::rounded(ws);
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t NP = (size_t)round_up(N, PROX_BN);
    w.G = c.take<char>(NP * NP * es);
    w.P = c.take<char>((size_t)N * T_ * es);
    w.W[0] = c.take<char>((size_t)N * T_ * es);
    w.W[1] = c.take<char>((size_t)N * T_ * es);
    w.thr = c.take<char>((size_t)N * es);
    w.tolv = c.take<char>((size_t)N * es);
    w.d = c.take<char>((size_t)N * es);
    w.lip = c.take<char>(((size_t)N + 1) * es);
    static_cast<ProxTail&>(w) = carve_prox_tail(c, N, T_, n_utt);
    w.bytes = c.bytes();
    return w;
}

inline size_t prox_workspace_bytes(int M, int N, int T_, int n_utt, int dtype) {
    if (M < 1 || M > PROX_MAX_M || N < 1 || N > PROX_MAX_N || T_ < 0 || n_utt < 1) return 0;
    if (dtype != EVC_F64 && dtype != EVC_F32) return 0;
    return carve_prox(nullptr, N, T_, n_utt, dtype).bytes + 256;
}

// the option ranges evc_prox_opts and evc_prox_masked_opts share, field for field: true, or false for ST_BADARG
template <typename Opts> bool prox_opts_ok(const Opts& o) {
    if (o.iters < 0 || o.check_every < 0 || o.reserved != 0 || o.reserved2 != 0) return false;
    if (o.mode != EVC_PROX_POSITIVE && o.mode != EVC_PROX_SIGNED) return false;
    if (o.momentum != EVC_PROX_ISTA && o.momentum != EVC_PROX_FISTA && o.momentum != EVC_PROX_NESTEROV) return false;
    if (o.normalize != 0 && o.normalize != 1) return false;
    if (o.init_mode != EVC_INIT_GIVEN && o.init_mode != EVC_INIT_CONST) return false;
    if (o.stop_rule != EVC_STOP_NONE && o.stop_rule != EVC_STOP_DECOMP) return false;
    if (!(o.alpha >= 0.0) || !(o.alpha - o.alpha == 0.0) || !(o.tol >= 0.0) || !(o.tol - o.tol == 0.0)) return false;
    if (!(o.lipschitz >= 0.0) || !(o.lipschitz - o.lipschitz == 0.0) || !(o.init_value - o.init_value == 0.0)) return false;
    return prox_slots(o.iters, o.check_every) <= PROX_MAX_SLOTS;
}

// evc_prox_solve's argument checks, in the order of its statuses: ST_BADARG, ST_UNSUPPORTED, ST_WORKSPACE before any device work
inline int prox_args_check(const void* A, int lda, const void* X, int ldx, const void* H, int ldh, int M, int N, int T,
                           const int* utt_offsets, int n_utt, const evc_prox_opts* opts, const void* workspace,
                           size_t workspace_bytes) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_prox_opts)) return ST_BADARG;
    const evc_prox_opts& o = *opts;
    HIP_TRY(solve_args_ok(M, N, T, n_utt, o.dtype, o.layout, A, workspace, lda, ldx, ldh, utt_offsets));
    if (!prox_opts_ok(o)) return ST_BADARG;
    if (T > 0 && (!X || !H)) return ST_BADARG;                             // no frames: X and H are never touched
    if (M > PROX_MAX_M || N > PROX_MAX_N) return ST_UNSUPPORTED;
    if (workspace_bytes < prox_workspace_bytes(M, N, T, n_utt, o.dtype)) return ST_WORKSPACE;
    return ST_OK;
}

}  // namespace evc
