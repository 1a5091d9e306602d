// evc_semi_plan.h - what evc_semi_solve decides on the host before its launches: the limits, the argument checks in the order
// of their statuses and the workspace carving.  No device code: tests/semi_host_main.hip, a program of its own, includes it
// and runs it under the host sanitizers (tests/test_semi_host.py).
#pragma once
#include "evc_internal.h"

namespace evc {

constexpr int SEMI_MAX_M = 1056;       // LEARN_MAX_M: stacked WORLD spectra; M is only a contraction length here
constexpr int SEMI_MAX_N = 16384;      // the Gram matrix is N x N: 2 GiB in float64 at this N
constexpr int SEMI_MAX_SLOTS = 4097;   // error slots per utterance (evc_beta_solve's cap)
constexpr int SEMI_MAX_WAVES = 8;      // wavefronts per workgroup of k_semi_sweep, each owning 16 exemplar rows
constexpr int SEMI_BN = 128;           // exemplar rows of the widest workgroup; G is padded to a multiple in both directions
constexpr int SEMI_BT = 64;            // frame columns per workgroup
constexpr int SEMI_KS = 16;            // exemplars per k-slab

// Wavefronts (row tiles of 16) per workgroup of k_semi_sweep: 8 where that already gives the chip two workgroups per compute
// unit (512 on 256), else 4 - a lone utterance gets twice as many, narrower workgroups (measured: DESIGN.md §5.16; 2 lost to
// both).  A function of the sizes alone, never of the device; an output's sums do not depend on it (every wavefront runs
// the same k-ascending chain over all of N).
constexpr int SEMI_FILL_WGS = 512;
inline int semi_waves(int N, int T_) {
#if defined(EVC_DIAG_SEMI_WAVES)           // diagnostic builds: one width for every size (A/B timing)
    return EVC_DIAG_SEMI_WAVES == SEMI_MAX_WAVES ? SEMI_MAX_WAVES : SEMI_MAX_WAVES / 2;
#endif
    const long frame_blocks = ((long)T_ + SEMI_BT - 1) / SEMI_BT, NP = round_up(N, SEMI_BN);
    return frame_blocks * (NP / SEMI_BN) >= SEMI_FILL_WGS ? SEMI_MAX_WAVES : SEMI_MAX_WAVES / 2;
}

struct SemiWs {
    char* G;            // [NP][NP] elements, NP = round_up(N, SEMI_BN): A^T A, zero in the padding
    char* P;            // [N][T] elements: A^T X
    char* H2;           // [T][N] (frame-major) or [N][T] elements: the second activation buffer, packed
    char* V;            // [T][M] elements: A H at a check
    double* err2;       // [T]: every frame's squared residual
    int* frame_utt;     // [T]
    int* offs;          // [n_utt + 1]
    int* stop;          // [n_utt]: 0 running, else the iteration the utterance stopped at
    double* eprev;      // [n_utt]
    double* trace;      // [n_utt][SEMI_MAX_SLOTS]
    size_t bytes;
};

// [G | P | H2 | V | err2 | frame_utt | offs | stop | eprev | trace], each 256-byte aligned (ws == NULL: sizes only)
inline SemiWs carve_semi(void* ws, int M, int N, int T_, int n_utt, int dtype) {
    SemiWs w;
    Carver c = Carver::rounded(ws);
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t NP = (size_t)round_up(N, SEMI_BN);
    w.G = c.take<char>(NP * NP * es);
    w.P = c.take<char>((size_t)N * T_ * es);
    w.H2 = c.take<char>((size_t)N * T_ * es);
    w.V = c.take<char>((size_t)T_ * M * es);
    w.err2 = c.take<double>((size_t)T_);
    w.frame_utt = c.take<int>((size_t)T_);
    w.offs = c.take<int>((size_t)n_utt + 1);
    w.stop = c.take<int>((size_t)n_utt);
    w.eprev = c.take<double>((size_t)n_utt);
    w.trace = c.take<double>((size_t)n_utt * SEMI_MAX_SLOTS);
    w.bytes = c.bytes();
    return w;
}

inline size_t semi_workspace_bytes(int M, int N, int T_, int n_utt, int dtype) {
    if (M < 1 || M > SEMI_MAX_M || N < 1 || N > SEMI_MAX_N || T_ < 0 || n_utt < 1) return 0;
    if (dtype != EVC_F64 && dtype != EVC_F32) return 0;
    return carve_semi(nullptr, M, N, T_, n_utt, dtype).bytes + 256;
}

// evc_semi_solve's argument checks, in the order of its statuses: ST_BADARG, ST_UNSUPPORTED, ST_WORKSPACE before any device work
inline int semi_args_check(const void* A, int lda, const void* X, int ldx, const void* H, int ldh, int M, int N, int T,
                           const int* utt_offsets, int n_utt, const evc_semi_opts* opts, const void* workspace,
                           size_t workspace_bytes) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_semi_opts)) return ST_BADARG;
    const evc_semi_opts& o = *opts;
    HIP_TRY(solve_args_ok(M, N, T, n_utt, o.dtype, o.layout, A, workspace, lda, ldx, ldh, utt_offsets));
    if (o.iters < 0 || o.check_every < 0 || o.reserved != 0) return ST_BADARG;
    if (o.init_mode != EVC_INIT_GIVEN && o.init_mode != EVC_INIT_CONST) return ST_BADARG;
    if (o.stop_rule != EVC_STOP_NONE && o.stop_rule != EVC_STOP_PYMF) return ST_BADARG;
    if (!(o.tol >= 0.0) || !(o.eps >= 0.0) || !(o.eps - o.eps == 0.0) || !(o.init_value - o.init_value == 0.0)) return ST_BADARG;
    if (T > 0 && (!X || !H)) return ST_BADARG;                             // no frames: X and H are never touched
    if (o.check_every > 0 && o.iters / o.check_every + 1 > SEMI_MAX_SLOTS) return ST_BADARG;
    if (M > SEMI_MAX_M || N > SEMI_MAX_N) return ST_UNSUPPORTED;
    if (workspace_bytes < semi_workspace_bytes(M, N, T, n_utt, o.dtype)) return ST_WORKSPACE;
    return ST_OK;
}

}  // namespace evc
