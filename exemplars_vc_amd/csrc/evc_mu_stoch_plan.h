// evc_mu_stoch_plan.h - what evc_mu_stoch_learn decides on the host before its launches: the limits, the argument checks in
// the order of their statuses, the check of the frame orders and the workspace carving.  No device code:
// tests/mu_stoch_host_main.hip, a program of its own, includes it and runs it under the host sanitizers
// (tests/test_mu_stoch_host.py).  DESIGN.md §5.23.
#pragma once
#include "evc_mu_masked_plan.h"

#include <cstdlib>
#include <cstring>

namespace evc {

constexpr int MUS_MAX_R = LEARN_MAX_R;                  // 4096 atoms
constexpr int MUS_FUSED_MAX_R = 256;                    // k_mus_dict_grad holds W's tile rows in LDS (BDG_MAX_R)
constexpr int MUS_ROUTE_R = 256;                        // ROUTE_AUTO takes the fused dictionary half up to this R: measured, DESIGN.md §5.23
                                                        // (evc_beta_learn's BDG_ROUTE_R = 64 does not carry over: a step here is launch-bound)
constexpr size_t MUS_MAX_PREV_BYTES = size_t(1) << 40;  // svrmu's prev+-[n_loop]: beyond this the call is refused with -3

inline int mus_n_loop(int T_, int bs) { return bs > 0 ? T_ / bs : 0; }
// dictionary updates of a call = trace slots: one per step, gsag one per epoch
inline long mus_updates(int method, int epochs, int n_loop) {
    return method == EVC_STOCH_GSAG ? (long)epochs : (long)epochs * n_loop;
}
// bytes of prev+-[n_loop][2][R][M] (svrmu only); 0 when they pass MUS_MAX_PREV_BYTES or are not needed
inline bool mus_prev_bytes(int M, int R, int n_loop, int method, size_t es, size_t* bytes) {
    *bytes = 0;
    if (method != EVC_STOCH_SVRMU) return true;
    const size_t per = (size_t)2 * (size_t)M * (size_t)R * es;       // <= 2 x 528 x 4096 x 8: no overflow
    if ((size_t)n_loop > MUS_MAX_PREV_BYTES / per) return false;
    *bytes = per * (size_t)n_loop;
    return true;
}

struct MusWs {
    int* ord;           // [T]: the epoch's row of `order`
    char* HF;           // [Tb][Np] elements: the batch's activations, frames as rows, zero-padded (Tb = frame_pad(bs))
    char* Xt;           // [Tb][Mk] elements: the batch's frames of X as rows, zero-padded
    char* Mt;           // [Tb][Mk] elements: the batch's frames of the mask
    char* Am;           // [Mj][Np] elements: W with the bins as rows (unfused route)
    char* Vt;           // [Tb][Mj] elements: (W H_F)^T (unfused route)
    char* Q1t;          // [Tb][Mj] elements
    char* Q2t;          // [Tb][Mj] elements
    char* part;         // [LEARN_MAX_SPLITS][2][learn_bin_tiles(M) * 16][Np] elements: the gradient slabs
    char* acc;          // [2][R][M] elements: a+- (asag, gsag) or full+- (svrmu)
    char* prev;         // [n_loop][2][R][M] elements (svrmu)
    char* cand;         // [R][M] elements: the candidate dictionary
    double* astat;      // [R]: every atom's share of max |W - W_new|
    double* trace;      // [n_loop]: the statistics of one epoch's updates (gsag: slot 0), copied out after every epoch
    int* stop;          // [1]: 0 running, else the step (from 1) whose update stopped the call
    char* solve_ws;     // the activation half's workspace (carve_mum with one utterance of bs frames)
    size_t solve_bytes, bytes;
};
constexpr int MUS_WS_ARRAYS = 16;

// each array 256-byte aligned (ws == NULL: sizes only); the sizes must have passed mus_sizes_status
inline MusWs carve_mus(void* ws, int M, int R, int T_, int bs, int method, int dtype) {
    MusWs w;
    Carver c = Carver::rounded(ws);
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const Dims d = make_dims((int)es, M, R, bs, 1);
    const int n_loop = mus_n_loop(T_, bs);
    size_t prev = 0;
    mus_prev_bytes(M, R, n_loop, method, es, &prev);
    w.ord = c.take<int>((size_t)T_);
    w.HF = c.take<char>((size_t)d.Tp * d.Np * es);
    w.Xt = c.take<char>((size_t)d.Tp * d.Mk * es);
    w.Mt = c.take<char>((size_t)d.Tp * d.Mk * es);
    w.Am = c.take<char>((size_t)d.Mj * d.Np * es);
    w.Vt = c.take<char>((size_t)d.Tp * d.Mj * es);
    w.Q1t = c.take<char>((size_t)d.Tp * d.Mj * es);
    w.Q2t = c.take<char>((size_t)d.Tp * d.Mj * es);
    w.part = c.take<char>((size_t)LEARN_MAX_SPLITS * 2 * learn_bin_tiles(M) * 16 * d.Np * es);
    w.acc = c.take<char>((size_t)2 * R * M * es);
    w.prev = c.take<char>(prev);
    w.cand = c.take<char>((size_t)R * M * es);
    w.astat = c.take<double>((size_t)R);
    w.trace = c.take<double>((size_t)n_loop);
    w.stop = c.take<int>(1);
    w.solve_bytes = mum_workspace_bytes(M, R, bs, 1, dtype);
    w.solve_ws = c.take<char>(w.solve_bytes);
    w.bytes = c.bytes();
    return w;
}

// 0: fine; ST_BADARG or ST_UNSUPPORTED
inline int mus_sizes_status(int M, int R, int T_, int bs, int method, int dtype) {
    if (M < 1 || R < 1 || T_ < 1 || bs < 1 || bs > T_) return ST_BADARG;
    if (dtype != EVC_F64 && dtype != EVC_F32) return ST_BADARG;
    if (method < EVC_STOCH_ASG || method > EVC_STOCH_SVRMU) return ST_BADARG;
    if (M > MUM_MAX_M || R > MUS_MAX_R) return ST_UNSUPPORTED;
    size_t prev;
    if (!mus_prev_bytes(M, R, mus_n_loop(T_, bs), method, dtype == EVC_F64 ? 8 : 4, &prev)) return ST_UNSUPPORTED;
    return ST_OK;
}

inline size_t mus_workspace_bytes(int M, int R, int T_, int bs, int method, int dtype) {
    if (mus_sizes_status(M, R, T_, bs, method, dtype) != ST_OK) return 0;
    return carve_mus(nullptr, M, R, T_, bs, method, dtype).bytes + 256;
}

// every row of order[rows][T] must be a permutation of 0 .. T - 1; ST_OK, ST_BADARG, or hipErrorOutOfMemory
inline int mus_order_check(const int* order, int rows, int T_) {
    if (!order || rows == 0) return ST_OK;
    unsigned char* seen = static_cast<unsigned char*>(malloc((size_t)T_));
    if (!seen) return (int)hipErrorOutOfMemory;
    int st = ST_OK;
    for (int e = 0; e < rows && st == ST_OK; ++e) {
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

// ROUTE_* of the dictionary half: 1 fused (k_mus_dict_grad), 2 unfused (evc_mu_masked_learn's kernels); 0: route invalid
inline int mus_route(int route, int R) {
    if (route == 0) return R <= MUS_ROUTE_R ? 1 : 2;
    return route == 1 || route == 2 ? route : 0;
}

// evc_mu_stoch_learn's argument checks: ST_BADARG, then ST_UNSUPPORTED, then ST_WORKSPACE, before any device work
inline int mus_args_check(const void* X, int ldx, const void* mask, int ldm, const void* W, int ldw, const void* H, int ldh,
                          const int* order, int M, int R, int T, const evc_mu_stoch_opts* opts, const void* workspace,
                          size_t workspace_bytes) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_mu_stoch_opts)) return ST_BADARG;
    const evc_mu_stoch_opts& o = *opts;
    int forced;
    HIP_TRY(learn_args_ok(M, R, T, o.dtype, o.layout, X, W, H, workspace, ldx, ldw, ldh, 0, 0, &forced));
    if (mask && bad_ld(o.layout, ldm, T, M)) return ST_BADARG;
    if (o.loss != EVC_LOSS_FROBENIUS && o.loss != EVC_LOSS_KL) return ST_BADARG;
    if (o.method < EVC_STOCH_ASG || o.method > EVC_STOCH_SVRMU) return ST_BADARG;
    if (o.batch_size < 1 || o.batch_size > T || o.epochs < 0 || o.reserved != 0 || o.reserved2 != 0) return ST_BADARG;
    if (o.inner_iters < 1 || (o.inner_iters != 1 && o.method != EVC_STOCH_SVRMU)) return ST_BADARG;
    if (o.route < 0 || o.route > 2) return ST_BADARG;
    if ((long)o.epochs * mus_n_loop(T, o.batch_size) > (long)0x7fffffff) return ST_BADARG;      // n_steps_out is an int
    if (!(o.tol >= 0.0) || !(o.tol - o.tol == 0.0)) return ST_BADARG;
    if (!(o.forget_rate > 0.0 && o.forget_rate <= 1.0) || !(o.alpha - o.alpha == 0.0)) return ST_BADARG;
    if (order ? (o.order_rows != 1 && o.order_rows != o.epochs) : o.order_rows != 0) return ST_BADARG;
    const int sz = mus_sizes_status(M, R, T, o.batch_size, o.method, o.dtype);
    if (sz == ST_BADARG) return ST_BADARG;
    HIP_TRY(mus_order_check(order, o.order_rows, T));
    if (sz != ST_OK) return sz;
    if (o.route == 1 && R > MUS_FUSED_MAX_R) return ST_UNSUPPORTED;
    if (workspace_bytes < mus_workspace_bytes(M, R, T, o.batch_size, o.method, o.dtype)) return ST_WORKSPACE;
    return ST_OK;
}

}  // namespace evc
