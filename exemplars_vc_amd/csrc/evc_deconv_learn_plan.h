// evc_deconv_learn_plan.h - what evc_deconv_learn decides on the host before its launches: the limits, the frame ranges and
// tap chunks of the dictionary half, the argument checks in the order of their statuses and the workspace carving.  No
// device code: tests/deconv_learn_host_main.hip, a program of its own, includes it and runs it under the host sanitizers
// (tests/test_deconv_learn_host.py).
#pragma once
#include "evc_deconv_plan.h"

namespace evc {

constexpr size_t DCL_SLAB_CAP = size_t(128) << 20;      // bytes the slabs of one k_deconv_dict_grad launch may take
constexpr int DCL_RING = 64;                             // error words in flight (one per check, read back at once)

// one slab pair (Num | Den of one tap and one frame range): 2 x learn_bin_tiles(M) * 16 rows x round_up(R, 128) columns
inline size_t dcl_pair_elems(int M, int R) { return (size_t)2 * learn_bin_tiles(M) * 16 * round_up(R, 128); }

inline bool dcl_sizes_ok(int M, int R, int T_, int n_utt, int taps, int update) {
    if (M < 1 || R < 1 || T_ < 1 || n_utt < 1 || taps < 1) return false;
    if (update != EVC_DCL_BOTH && update != EVC_DCL_DICT_ONLY) return false;
    return taps <= DC_MAX_TAPS && R <= LEARN_MAX_R && M <= (update == EVC_DCL_BOTH ? DC_MAX_M : DC_MAX_MB);
}

// The frame ranges S and the taps contracted per launch (`chunk`), from the sizes alone; the slab pairs are counted at 8
// bytes an element whatever the type, so that neither depends on it.  S: about four workgroups per compute unit of a
// 256-CU device over ranges of at least 256 frames, as learn_splits; then lowered until S * taps pairs fit the cap, and
// where one range of all taps does not, the taps go a chunk at a time.  forced (1..64): S as asked, lowered likewise.
// Sizes within the limits only (dcl_sizes_ok): a pair is then at most 68 * 16 * 4096 * 2 * 8 = 71 303 168 bytes.
struct DclPlan {
    int S, chunk;
};
inline DclPlan dcl_plan(int M, int R, int T_, int taps, int forced) {
    const size_t pair = dcl_pair_elems(M, R) * 8;
    const int blocks = (round_up(R, 128) / 128) * (2 * learn_bin_tiles(M) / DG_MB) * taps;
    int S = forced;
    if (S < 1) {
        S = (1024 + blocks - 1) / blocks;
        S = S < T_ / 256 ? S : T_ / 256;
    }
    S = S > LEARN_MAX_SPLITS ? LEARN_MAX_SPLITS : S;
    const size_t fit = DCL_SLAB_CAP / (pair * (size_t)taps);        // ranges of all taps the cap holds
    if ((size_t)S > fit) S = (int)fit;
    S = S < 1 ? 1 : S;
    size_t chunk = DCL_SLAB_CAP / (pair * (size_t)S);
    chunk = chunk > (size_t)taps ? (size_t)taps : chunk;
    DclPlan p;
    p.S = S;
    p.chunk = chunk < 1 ? 1 : (int)chunk;
    return p;
}

struct DclWs {
    char* tiles;            // int4 [frame_tile_cap]: the frame-tile table (evc_internal.h)
    char* tpos;             // int4 [frame_tile_cap]: per tile {first frame, frames, frames of the utterance before it, 0}
    char* utt_tile0;        // int [n_utt + 1]
    char* stop;             // int [n_utt]: zeros (k_deconv_v and k_deconv_update read it; nothing stops per utterance here)
    char *Xp, *Qn, *Qd;     // [frame_tile_cap][MP][16] elements each: the packed X and k_deconv_v's two images
    char *Ap1, *Ap3;        // [taps][RP][MP] elements each: the activation half's packed taps (EVC_DCL_BOTH only)
    char* errf;             // double [bin groups][frame_tile_cap * 16]: per-frame shares of the error
    char* ring;             // double [DCL_RING]
    char* part;             // the slabs: min(cap, 64 ranges x taps) pairs' worth
    size_t bytes;
};

// bin groups of k_deconv_learn_v (EVC_DCL_DICT_ONLY): BT_GT bin tiles each; k_deconv_v (EVC_DCL_BOTH) holds all bins: 1
inline int dcl_bin_groups(int M, int update) {
    return update == EVC_DCL_BOTH ? 1 : (round_up(M, 16) / 16 + BT_GT - 1) / BT_GT;
}

// every array 256-byte aligned (ws == NULL: sizes only)
inline DclWs carve_deconv_learn(void* ws, int M, int R, int T_, int n_utt, int taps, int update, int dtype) {
    DclWs w;
    Carver c = Carver::rounded(ws);
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t MP = (size_t)round_up(M, 16), RP = (size_t)round_up(R, 16);
    const size_t nt = (size_t)frame_tile_cap(T_, BT_F, n_utt);
    const size_t dict = update == EVC_DCL_BOTH ? (size_t)taps * RP * MP * es : 0;
    w.tiles = c.take<char>(nt * sizeof(int4));
    w.tpos = c.take<char>(nt * sizeof(int4));
    w.utt_tile0 = c.take<char>(((size_t)n_utt + 1) * sizeof(int));
    w.stop = c.take<char>((size_t)n_utt * sizeof(int));
    w.Xp = c.take<char>(nt * MP * BT_F * es);
    w.Qn = c.take<char>(nt * MP * BT_F * es);
    w.Qd = c.take<char>(nt * MP * BT_F * es);
    w.Ap1 = c.take<char>(dict);
    w.Ap3 = c.take<char>(dict);
    w.errf = c.take<char>((size_t)dcl_bin_groups(M, update) * nt * BT_F * sizeof(double));
    w.ring = c.take<char>(DCL_RING * sizeof(double));
    const size_t pair = dcl_pair_elems(M, R), all = (size_t)LEARN_MAX_SPLITS * taps * pair * es;
    // dcl_plan counts a pair at 8 bytes: what it admits never exceeds the cap in either type
    w.part = c.take<char>(all < DCL_SLAB_CAP ? all : DCL_SLAB_CAP);
    w.bytes = c.bytes();
    return w;
}

inline size_t deconv_learn_workspace_bytes(int M, int R, int T_, int n_utt, int taps, int update, int dtype) {
    if (!dcl_sizes_ok(M, R, T_, n_utt, taps, update) || (dtype != EVC_F64 && dtype != EVC_F32)) return 0;
    return carve_deconv_learn(nullptr, M, R, T_, n_utt, taps, update, dtype).bytes + 256;
}

inline int deconv_learn_splits(int M, int R, int T_, int n_utt, int taps) {
    // the wider of the two limits on M: the count is the same function under either update mode
    return dcl_sizes_ok(M, R, T_, n_utt, taps, EVC_DCL_DICT_ONLY) ? dcl_plan(M, R, T_, taps, 0).S : 0;
}

// evc_deconv_learn's argument checks, in the order of its statuses: ST_BADARG, ST_UNSUPPORTED, ST_WORKSPACE before any
// device work.  *forced: the frame ranges asked for in opts->reserved (0: none).
inline int deconv_learn_args_check(const void* X, int ldx, const void* W, int ldw, long tap_stride, const void* H, int ldh,
                                   int M, int R, int T, const int* utt_offsets, int n_utt,
                                   const evc_deconv_learn_opts* opts, const void* workspace, size_t workspace_bytes,
                                   int* forced) {
    *forced = 0;
    if (!opts || opts->struct_bytes != (int)sizeof(evc_deconv_learn_opts)) return ST_BADARG;
    const evc_deconv_learn_opts& o = *opts;
    HIP_TRY(learn_args_ok(M, R, T, o.dtype, o.layout, X, W, H, workspace, ldx, ldw, ldh, o.reserved, 0xff00, forced));
    if (n_utt < 1 || !utt_offsets_ok(utt_offsets, n_utt, T)) return ST_BADARG;
    if (o.taps < 1 || (o.loss != EVC_LOSS_FROBENIUS && o.loss != EVC_LOSS_KL)) return ST_BADARG;
    if (o.update != EVC_DCL_BOTH && o.update != EVC_DCL_DICT_ONLY) return ST_BADARG;
    if (o.iters < 0 || o.check_every < 0) return ST_BADARG;
    if (!(o.tol >= 0.0) || !(o.l1_h >= 0.0) || !(o.l2_h >= 0.0)) return ST_BADARG;
    if (o.check_every > 0 && o.iters / o.check_every + 1 > MAX_SLOTS) return ST_BADARG;
    // the taps are written: one tap's extent in the caller's memory must fit between two taps
    const long extent = o.layout == EVC_FRAME_MAJOR ? (long)(R - 1) * ldw + M : (long)(M - 1) * ldw + R;
    if (o.taps > 1 && tap_stride < extent) return ST_BADARG;
    if (o.taps > DC_MAX_TAPS || R > LEARN_MAX_R || M > (o.update == EVC_DCL_BOTH ? DC_MAX_M : DC_MAX_MB))
        return ST_UNSUPPORTED;
    if (workspace_bytes < deconv_learn_workspace_bytes(M, R, T, n_utt, o.taps, o.update, o.dtype)) return ST_WORKSPACE;
    return ST_OK;
}

}  // namespace evc
