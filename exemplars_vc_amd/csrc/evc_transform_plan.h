// evc_transform_plan.h - what evc_online_transform decides on the host before its launches: the argument checks and the
// workspace carving.  No device code: tests/transform_host_main.hip, a program of its own, includes it and runs it under
// the host sanitizers (tests/test_minibatch_host.py).
#pragma once
#include "evc_beta_common.h"

namespace evc {

struct TrWs {
    double* chg;            // [frame_tile_cap * 16][2] the change variant's per-frame shares
    char* beta_ws;
    size_t beta_bytes, bytes;
};

// [chg | the activation half's workspace], each 256-byte aligned (ws == NULL: sizes only)
inline TrWs carve_transform(void* ws, int M, int R, int T_, int n_utt, int dtype) {
    TrWs w;
    Carver c = Carver::rounded(ws);
    w.chg = c.take<double>((size_t)frame_tile_cap(T_, BT_F, n_utt) * BT_F * 2);
    w.beta_bytes = beta_workspace_bytes(M, R, T_, n_utt, dtype);
    w.beta_ws = c.take<char>(w.beta_bytes);
    w.bytes = c.bytes();
    return w;
}

inline size_t transform_workspace_bytes(int M, int R, int T_, int n_utt, int dtype) {
    if (M < 1 || M > BETA_MAX_M || R < 1 || T_ < 0 || n_utt < 1 || (dtype != EVC_F64 && dtype != EVC_F32)) return 0;
    return carve_transform(nullptr, M, R, T_, n_utt, dtype).bytes + 256;
}

// trace slots per utterance: one per iteration (at least one, so that the state kernels have something to launch over)
inline int transform_slots(int max_iter) { return max_iter > 0 ? max_iter : 1; }

// evc_online_transform's argument checks, in the order of its statuses: ST_BADARG, ST_UNSUPPORTED, ST_WORKSPACE before any
// device work
inline int transform_args_check(const void* W, int ldw, const void* X, int ldx, const void* H, int ldh, int M, int R, int T,
                                const int* utt_offsets, int n_utt, const evc_transform_opts* opts, const void* workspace,
                                size_t workspace_bytes) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_transform_opts)) return ST_BADARG;
    const evc_transform_opts& o = *opts;
    HIP_TRY(solve_args_ok(M, R, T, n_utt, o.dtype, o.layout, W, workspace, ldw, ldx, ldh, utt_offsets));
    if (o.max_iter < 0 || o.reserved != 0) return ST_BADARG;
    if (o.init_mode != EVC_INIT_GIVEN && o.init_mode != EVC_INIT_SKLEARN && o.init_mode != EVC_INIT_CONST) return ST_BADARG;
    if (!(o.beta - o.beta == 0.0)) return ST_BADARG;                      // NaN or infinite
    if (!(o.tol >= 0.0) || !(o.l1 >= 0.0) || !(o.l2 >= 0.0) || !(o.init_value - o.init_value == 0.0)) return ST_BADARG;
    if (T > 0 && (!X || !H)) return ST_BADARG;                             // no frames: X and H are never touched
    if (o.max_iter > BETA_MAX_SLOTS) return ST_BADARG;
    if (M > BETA_MAX_M) return ST_UNSUPPORTED;
    if (workspace_bytes < transform_workspace_bytes(M, R, T, n_utt, o.dtype)) return ST_WORKSPACE;
    return ST_OK;
}

}  // namespace evc
