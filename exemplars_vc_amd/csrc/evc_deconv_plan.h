// evc_deconv_plan.h - what evc_deconv_solve and evc_deconv_synthesize decide on the host before their launches: the limits,
// the argument checks in the order of their statuses and the workspace carving.  No device code: tests/deconv_host_main.hip,
// a program of its own, includes it and runs it under the host sanitizers (tests/test_deconv_host.py).
#pragma once
#include "evc_beta_common.h"

namespace evc {

constexpr int DC_MAX_M = 256;         // k_deconv_update: two LDS images of 256 x 32 float64 are 131 072 of 163 840 bytes
constexpr int DC_MAX_TAPS = 16;       // a tile of 16 frames and the next one: 32 frame columns, so a tap reaches at most 15 on
constexpr int DC_MAX_MB = 1056;       // evc_deconv_synthesize's bins (LEARN_MAX_M: stacked WORLD spectra)
constexpr int DC_COLS = 2 * BT_F;     // frame columns of the update's LDS images

struct DcWs {
    char *Ap1, *Ap3;        // [taps][NP][MP] elements each: the two packed images of every tap (as BetaArgs has them)
    char *Qn, *Qd;          // [frame_tile_cap][MP][16] elements each: the images k_deconv_v leaves for k_deconv_update
    char* beta_ws;          // the tile table, the packed X, the stop state and the trace: evc_beta_solve's carving
    size_t beta_bytes, bytes;
};

// [Ap1 | Ap3 | Qn | Qd | the activation half's workspace], each 256-byte aligned (ws == NULL: sizes only)
inline DcWs carve_deconv(void* ws, int M, int N, int T_, int n_utt, int taps, int dtype) {
    DcWs w;
    Carver c = Carver::rounded(ws);
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t MP = (size_t)round_up(M, 16), NP = (size_t)round_up(N, 16);
    const size_t nt = (size_t)frame_tile_cap(T_, BT_F, n_utt);
    w.Ap1 = c.take<char>((size_t)taps * NP * MP * es);
    w.Ap3 = c.take<char>((size_t)taps * NP * MP * es);
    w.Qn = c.take<char>(nt * MP * BT_F * es);
    w.Qd = c.take<char>(nt * MP * BT_F * es);
    w.beta_bytes = beta_workspace_bytes(M, N, T_, n_utt, dtype);
    w.beta_ws = c.take<char>(w.beta_bytes);
    w.bytes = c.bytes();
    return w;
}

inline size_t deconv_workspace_bytes(int M, int N, int T_, int n_utt, int taps, int dtype) {
    if (M < 1 || M > DC_MAX_M || N < 1 || T_ < 0 || n_utt < 1 || taps < 1 || taps > DC_MAX_TAPS) return 0;
    if (dtype != EVC_F64 && dtype != EVC_F32) return 0;
    return carve_deconv(nullptr, M, N, T_, n_utt, taps, dtype).bytes + 256;
}

// evc_deconv_solve's argument checks, in the order of its statuses: ST_BADARG, ST_UNSUPPORTED, ST_WORKSPACE before any
// device work
inline int deconv_args_check(const void* A, int lda, long tap_stride, const void* X, int ldx, const void* H, int ldh, int M,
                             int N, int T, const int* utt_offsets, int n_utt, const evc_deconv_opts* opts,
                             const void* workspace, size_t workspace_bytes) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_deconv_opts)) return ST_BADARG;
    const evc_deconv_opts& o = *opts;
    HIP_TRY(solve_args_ok(M, N, T, n_utt, o.dtype, o.layout, A, workspace, lda, ldx, ldh, utt_offsets));
    if (o.taps < 1 || tap_stride < 0) return ST_BADARG;
    if (o.loss != EVC_LOSS_FROBENIUS && o.loss != EVC_LOSS_KL) return ST_BADARG;
    if (o.iters < 0 || o.check_every < 0 || o.reserved != 0) return ST_BADARG;
    if (o.init_mode != EVC_INIT_GIVEN && o.init_mode != EVC_INIT_SKLEARN && o.init_mode != EVC_INIT_CONST) return ST_BADARG;
    if (o.stop_rule != EVC_STOP_NONE && o.stop_rule != EVC_STOP_SKLEARN) return ST_BADARG;
    if (!(o.tol >= 0.0) || !(o.l1 >= 0.0) || !(o.l2 >= 0.0) || !(o.init_value - o.init_value == 0.0)) return ST_BADARG;
    if (T > 0 && (!X || !H)) return ST_BADARG;                             // no frames: X and H are never touched
    if (o.check_every > 0 && o.iters / o.check_every + 1 > BETA_MAX_SLOTS) return ST_BADARG;
    if (M > DC_MAX_M || o.taps > DC_MAX_TAPS) return ST_UNSUPPORTED;
    if (workspace_bytes < deconv_workspace_bytes(M, N, T, n_utt, o.taps, o.dtype)) return ST_WORKSPACE;
    return ST_OK;
}

// evc_deconv_synthesize's: ST_BADARG, then ST_UNSUPPORTED (it takes no workspace)
inline int deconv_synth_args_check(const void* B, int ldb, long tap_stride, const void* H, int ldh, const void* Y, int ldy,
                                   int Mb, int N, int T, const int* utt_offsets, int n_utt, int taps, int layout, int dtype) {
    if (Mb < 1 || N < 1 || T < 0 || n_utt < 1 || taps < 1 || tap_stride < 0) return ST_BADARG;
    if ((dtype != EVC_F64 && dtype != EVC_F32) || (layout != EVC_FRAME_MAJOR && layout != EVC_BIN_MAJOR)) return ST_BADARG;
    if (!B || (T > 0 && (!H || !Y))) return ST_BADARG;
    if (bad_ld(layout, ldb, N, Mb) || bad_ld(layout, ldh, T, N) || bad_ld(layout, ldy, T, Mb)) return ST_BADARG;
    if (!utt_offsets_ok(utt_offsets, n_utt, T)) return ST_BADARG;
    if (Mb > DC_MAX_MB || taps > DC_MAX_TAPS) return ST_UNSUPPORTED;
    return ST_OK;
}

}  // namespace evc
