// evc_mu_masked_plan.h - what evc_mu_masked_solve and evc_mu_masked_learn decide on the host before their launches: the limits,
// the argument checks in the order of their statuses and the workspace carving.  The tile geometry and the limits are evc_beta_solve's
// (evc_beta_common.h; evc_mu_masked.hip asserts that they agree).  No device code: tests/mu_masked_host_main.hip, a program of
// its own, includes it and runs it under the host sanitizers (tests/test_mu_masked_host.py).
#pragma once
#include "evc_internal.h"

namespace evc {

constexpr int MUM_F = 16;             // frames per tile (BT_F)
constexpr int MUM_MAX_M = 528;        // two LDS images of 528 x 16 float64 (BETA_MAX_M)
constexpr int MUM_MAX_SLOTS = 4097;   // error slots per utterance (BETA_MAX_SLOTS)
constexpr double MUM_J = 1.0e-15;     // deComP's _JITTER, in both element types

inline int mum_slots(int iters, int check_every) { return n_slots_for(iters, check_every); }

struct MumWs {
    char* Ap1;          // [NP][MP] elements: exemplars as rows, bins contiguous, zero-padded (NP, MP: N, M rounded up to 16)
    char* Ap3;          // [NP][MP] elements: the same with the bins of every chunk of 16 permuted (BetaArgs.Ap3)
    char* Xp;           // [tiles][MP][16] elements: X in the tile's order, zero-padded (read by the error only)
    char* XMp;          // [tiles][MP][16] elements: mask . X
    char* Mp;           // [tiles][MP][16] elements: mask (1 without one), zero in the padding
    double* errf;       // [tiles * 16]: the frames' shares of the error
    int4* tiles;        // [tiles]
    int* utt_tile0;     // [n_utt + 1]
    int* stop;          // [n_utt]
    double* einit;      // [n_utt]
    double* eprev;      // [n_utt]
    double* trace;      // [n_utt][MUM_MAX_SLOTS]
    size_t bytes;
};
constexpr int MUM_WS_ARRAYS = 12;

// [Ap1 | Ap3 | Xp | XMp | Mp | errf | tiles | utt_tile0 | stop | einit | eprev | trace], each 256-byte
// aligned (ws == NULL: sizes only)
inline MumWs carve_mum(void* ws, int M, int N, int T_, int n_utt, int dtype) {
    MumWs w;
    Carver c = Carver::rounded(ws);
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t MP = (size_t)round_up(M, 16), NP = (size_t)round_up(N, 16);
    const size_t nt = (size_t)frame_tile_cap(T_, MUM_F, n_utt);
    w.Ap1 = c.take<char>(NP * MP * es);
    w.Ap3 = c.take<char>(NP * MP * es);
    w.Xp = c.take<char>(nt * MP * MUM_F * es);
    w.XMp = c.take<char>(nt * MP * MUM_F * es);
    w.Mp = c.take<char>(nt * MP * MUM_F * es);
    w.errf = c.take<double>(nt * MUM_F);
    w.tiles = c.take<int4>(nt);
    w.utt_tile0 = c.take<int>((size_t)n_utt + 1);
    w.stop = c.take<int>((size_t)n_utt);
    w.einit = c.take<double>((size_t)n_utt);
    w.eprev = c.take<double>((size_t)n_utt);
    w.trace = c.take<double>((size_t)n_utt * MUM_MAX_SLOTS);
    w.bytes = c.bytes();
    return w;
}

inline size_t mum_workspace_bytes(int M, int N, int T_, int n_utt, int dtype) {
    if (M < 1 || M > MUM_MAX_M || N < 1 || T_ < 0 || n_utt < 1) return 0;
    if (dtype != EVC_F64 && dtype != EVC_F32) return 0;
    return carve_mum(nullptr, M, N, T_, n_utt, dtype).bytes + 256;
}

// evc_mu_masked_solve's argument checks: ST_BADARG, then ST_UNSUPPORTED, then ST_WORKSPACE, before any device work
inline int mum_args_check(const void* A, int lda, const void* X, int ldx, const void* mask, int ldm, const void* H, int ldh,
                          int M, int N, int T, const int* utt_offsets, int n_utt, const evc_mu_masked_opts* opts,
                          const void* workspace, size_t workspace_bytes) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_mu_masked_opts)) return ST_BADARG;
    const evc_mu_masked_opts& o = *opts;
    HIP_TRY(solve_args_ok(M, N, T, n_utt, o.dtype, o.layout, A, workspace, lda, ldx, ldh, utt_offsets));
    if (mask && bad_ld(o.layout, ldm, T, M)) return ST_BADARG;
    if (o.loss != EVC_LOSS_FROBENIUS && o.loss != EVC_LOSS_KL) return ST_BADARG;
    if (o.iters < 0 || o.check_every < 0 || o.reserved != 0 || o.reserved2 != 0) return ST_BADARG;
    if (o.init_mode != EVC_INIT_GIVEN && o.init_mode != EVC_INIT_CONST) return ST_BADARG;
    if (o.stop_rule != EVC_STOP_NONE && o.stop_rule != EVC_STOP_SKLEARN) return ST_BADARG;
    if (!(o.tol >= 0.0) || !(o.tol - o.tol == 0.0) || !(o.init_value - o.init_value == 0.0)) return ST_BADARG;
    if (T > 0 && (!X || !H)) return ST_BADARG;                             // no frames: X, mask and H are never touched
    if (o.check_every > 0 && mum_slots(o.iters, o.check_every) > MUM_MAX_SLOTS) return ST_BADARG;
    if (M > MUM_MAX_M) return ST_UNSUPPORTED;
    if (workspace_bytes < mum_workspace_bytes(M, N, T, n_utt, o.dtype)) return ST_WORKSPACE;
    return ST_OK;
}

// ----- evc_mu_masked_learn -----
constexpr int MUM_LEARN_MAX_R = LEARN_MAX_R;

struct MumLearnWs {
    char* Am;           // [Mj][Np] elements: W with the bins as rows, zero-padded (make_dims)
    char* Ht;           // [Tp][Np] elements: H with the frames as rows
    char* Vt;           // [Tp][Mj] elements: (W H)^T
    char* Q1t;          // [Tp][Mj] elements: the left operand of Num
    char* Q2t;          // [Tp][Mj] elements: the left operand of Den
    char* part;         // [LEARN_MAX_SPLITS][2][learn_bin_tiles(M) * 16][Np] elements: the slabs of partial sums
    double* astat;      // [R]: every atom's share of max |D - D_new|
    double* stat;       // [1]
    char* solve_ws;     // the activation half's workspace (carve_mum with one utterance)
    size_t solve_bytes, bytes;
};
constexpr int MUM_LEARN_WS_ARRAYS = 9;

// [Am | Ht | Vt | Q1t | Q2t | part | astat | stat | the activation half's workspace], each 256-byte aligned (ws == NULL: sizes only)
inline MumLearnWs carve_mum_learn(void* ws, int M, int R, int T_, int dtype) {
    MumLearnWs w;
    Carver c = Carver::rounded(ws);
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const Dims d = make_dims((int)es, M, R, T_, 1);
    w.Am = c.take<char>((size_t)d.Mj * d.Np * es);
    w.Ht = c.take<char>((size_t)d.Tp * d.Np * es);
    w.Vt = c.take<char>((size_t)d.Tp * d.Mj * es);
    w.Q1t = c.take<char>((size_t)d.Tp * d.Mj * es);
    w.Q2t = c.take<char>((size_t)d.Tp * d.Mj * es);
    w.part = c.take<char>((size_t)LEARN_MAX_SPLITS * 2 * learn_bin_tiles(M) * 16 * d.Np * es);
    w.astat = c.take<double>((size_t)R);
    w.stat = c.take<double>(1);
    w.solve_bytes = mum_workspace_bytes(M, R, T_, 1, dtype);
    w.solve_ws = c.take<char>(w.solve_bytes);
    w.bytes = c.bytes();
    return w;
}

inline size_t mum_learn_workspace_bytes(int M, int R, int T_, int dtype) {
    if (M < 1 || M > MUM_MAX_M || R < 1 || R > MUM_LEARN_MAX_R || T_ < 1) return 0;
    if (dtype != EVC_F64 && dtype != EVC_F32) return 0;
    return carve_mum_learn(nullptr, M, R, T_, dtype).bytes + 256;
}

// evc_mu_masked_learn's argument checks: ST_BADARG, then ST_UNSUPPORTED, then ST_WORKSPACE, before any device work; *forced:
// the frame ranges bits 8..15 of `reserved` ask for (0: learn_splits decides)
inline int mum_learn_args_check(const void* X, int ldx, const void* mask, int ldm, const void* W, int ldw, const void* H, int ldh,
                                int M, int R, int T, const evc_mu_masked_learn_opts* opts, const void* workspace,
                                size_t workspace_bytes, int* forced) {
    *forced = 0;
    if (!opts || opts->struct_bytes != (int)sizeof(evc_mu_masked_learn_opts)) return ST_BADARG;
    const evc_mu_masked_learn_opts& o = *opts;
    HIP_TRY(learn_args_ok(M, R, T, o.dtype, o.layout, X, W, H, workspace, ldx, ldw, ldh, o.reserved, 0xff00, forced));
    if (mask && bad_ld(o.layout, ldm, T, M)) return ST_BADARG;
    if (o.loss != EVC_LOSS_FROBENIUS && o.loss != EVC_LOSS_KL) return ST_BADARG;
    if (o.iters < 0 || o.check_every < 0 || o.reserved2 != 0) return ST_BADARG;
    if (!(o.tol >= 0.0) || !(o.tol - o.tol == 0.0)) return ST_BADARG;
    if (o.check_every > 0 && mum_slots(o.iters, o.check_every) > MUM_MAX_SLOTS) return ST_BADARG;
    if (M > MUM_MAX_M || R > MUM_LEARN_MAX_R) return ST_UNSUPPORTED;
    if (workspace_bytes < mum_learn_workspace_bytes(M, R, T, o.dtype)) return ST_WORKSPACE;
    return ST_OK;
}

}  // namespace evc
