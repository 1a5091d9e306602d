// evc_prox_masked_plan.h - what evc_prox_masked_solve decides on the host before its launches: the padded sizes of the two
// dictionary images, the wavefronts per workgroup of its two kernels, the argument checks in the order of their statuses
// and the workspace carving.  The limits, the statistic slots and the momentum schedule are evc_prox_solve's
// (evc_prox_plan.h).  No device code: tests/prox_masked_host_main.hip, a program of its own, includes it and runs it under
// the host sanitizers (tests/test_prox_masked_host.py).
#pragma once
#include "evc_prox_plan.h"

namespace evc {

// The scaled dictionary is kept twice, zero-padded so that the slab loads of the two kernels need no bounds checks:
//   Dn [pm_nk(N)][pm_mp(M)]   exemplar-major (a row is an exemplar, bins contiguous): k_prox_resid streams it over n
//   Dm [pm_mk(M)][pm_np(N)]   bin-major (a row is a bin, exemplars contiguous): k_prox_back streams it over m
// rows padded to whole k-slabs (PROX_KS), columns to the widest workgroup's row block (PROX_BN), as G is in evc_prox_solve
inline int pm_nk(int N) { return round_up(N, PROX_KS); }
inline int pm_mp(int M) { return round_up(M, PROX_BN); }
inline int pm_mk(int M) { return round_up(M, PROX_KS); }
inline int pm_np(int N) { return round_up(N, PROX_BN); }

// Wavefronts (row tiles of 16) per workgroup, prox_waves' rule on each kernel's own rows: k_prox_resid owns bins x frames,
// k_prox_back exemplars x frames.  A function of the sizes alone; no output's bits depend on it.
inline int pm_resid_waves(int M, int T_) { return prox_waves(M, T_); }
inline int pm_back_waves(int N, int T_) { return prox_waves(N, T_); }

struct ProxMaskedWs : ProxTail {
    char* Dn;           // [pm_nk(N)][pm_mp(M)] elements: A / d, exemplar-major, zero in the padding
    char* Dm;           // [pm_mk(M)][pm_np(N)] elements: A / d, bin-major, zero in the padding
    char* P;            // [N][T] elements: A^T (mask . X) in the scaled dictionary
    char* W[2];         // [N][T] elements each: the extrapolated point, read from one and written to the other
    char* R;            // [M][T] elements: mask . (A W)
    char* Xm;           // [M][T] elements: mask . X
    char* lam;          // [N] elements: alpha / d_n | alpha
    char* tolv;         // [N] elements: tol_n
    char* d;            // [N] elements: the exemplars' norms, or 1
    char* colsum;       // [n_utt][N] elements: the Gershgorin column sums of A diag(wbar_u) A^T
    char* wbar;         // [n_utt][M] elements: the per-bin weights of the bound
    char* s;            // [n_utt] elements: 1 / L_u
    char* cf;           // [T] elements: cnt_t = sum_m mask_tm | 1 (normalize == 0)
    size_t bytes;
};
constexpr int PROX_MASKED_WS_ARRAYS = 19;

// [Dn | Dm | P | W0 | W1 | R | Xm | lam | tol | d | colsum | wbar | s | cf | partials | frame_utt | offs | stop | trace], each
// 256-byte aligned (ws == NULL: sizes only); the last five are carve_prox_tail's (pm_np(N) is evc_prox_solve's NP).  Nothing is N x N: the bound is formed in panels of 16 rows that live in registers.
inline ProxMaskedWs carve_prox_masked(void* ws, int M, int N, int T_, int n_utt, int dtype) {
    ProxMaskedWs w;
    Carver c = Carver::rounded(ws);
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t nt = (size_t)N * T_ * es, mt = (size_t)M * T_ * es;
    w.Dn = c.take<char>((size_t)pm_nk(N) * pm_mp(M) * es);
    w.Dm = c.take<char>((size_t)pm_mk(M) * pm_np(N) * es);
    w.P = c.take<char>(nt);
    w.W[0] = c.take<char>(nt);
    w.W[1] = c.take<char>(nt);
    w.R = c.take<char>(mt);
    w.Xm = c.take<char>(mt);
    w.lam = c.take<char>((size_t)N * es);
    w.tolv = c.take<char>((size_t)N * es);
    w.d = c.take<char>((size_t)N * es);
    w.colsum = c.take<char>((size_t)n_utt * N * es);
    w.wbar = c.take<char>((size_t)n_utt * M * es);
    w.s = c.take<char>((size_t)n_utt * es);
    w.cf = c.take<char>((size_t)T_ * es);
    static_cast<ProxTail&>(w) = carve_prox_tail(c, N, T_, n_utt);
    w.bytes = c.bytes();
    return w;
}

inline size_t prox_masked_workspace_bytes(int M, int N, int T_, int n_utt, int dtype) {
    if (M < 1 || M > PROX_MAX_M || N < 1 || N > PROX_MAX_N || T_ < 0 || n_utt < 1) return 0;
    if (dtype != EVC_F64 && dtype != EVC_F32) return 0;
    return carve_prox_masked(nullptr, M, N, T_, n_utt, dtype).bytes + 256;
}

// evc_prox_masked_solve's argument checks, in the order of evc_prox_solve's statuses: ST_BADARG, ST_UNSUPPORTED, ST_WORKSPACE
// before any device work
inline int prox_masked_args_check(const void* A, int lda, const void* X, int ldx, const void* mask, int ldm, const void* H,
                                  int ldh, int M, int N, int T, const int* utt_offsets, int n_utt,
                                  const evc_prox_masked_opts* opts, const void* workspace, size_t workspace_bytes) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_prox_masked_opts)) return ST_BADARG;
    const evc_prox_masked_opts& o = *opts;
    HIP_TRY(solve_args_ok(M, N, T, n_utt, o.dtype, o.layout, A, workspace, lda, ldx, ldh, utt_offsets));
    if (mask && bad_ld(o.layout, ldm, T, M)) return ST_BADARG;
    if (!prox_opts_ok(o) || o.reserved3 != 0) return ST_BADARG;
    if (o.lip_weights != EVC_PROX_LIP_MEAN && o.lip_weights != EVC_PROX_LIP_MAX) return ST_BADARG;
    if (T > 0 && (!X || !H)) return ST_BADARG;                             // no frames: X, mask and H are never touched
    if (M > PROX_MAX_M || N > PROX_MAX_N) return ST_UNSUPPORTED;
    if (workspace_bytes < prox_masked_workspace_bytes(M, N, T, n_utt, o.dtype)) return ST_WORKSPACE;
    return ST_OK;
}

}  // namespace evc
