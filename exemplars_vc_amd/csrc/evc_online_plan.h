// evc_online_plan.h - what evc_online_learn and evc_online_learn_fresh decide on the host before and between their launches:
// the argument checks, the workspace carving and the convergence rule.  No device code: tests/online_host_main.hip, a program of its own,
// includes it and runs it under the host sanitizers (tests/test_online_host.py).
#pragma once
#include "evc_beta_common.h"

namespace evc {

inline int online_blocks(int M, int R) { return (int)(((long)M * R + 255) / 256); }

template <typename T> struct OnWs {
    T *Xt, *Am, *Ht, *Vt, *Q2t, *part;
    double *sums, *stats;
    char* beta_ws;
    size_t beta_bytes, bytes;
};

// [Xt | Am | Ht | Vt | Q2t | part | sums | stats | the activation half's workspace], each 256-byte aligned (ws == NULL:
// sizes only).  Xt holds every frame; Ht, Vt and Q2t one batch.
template <typename T> OnWs<T> carve_online(void* ws, int M, int R, int T_, int bs, int n_batches) {
    OnWs<T> w;
    const int esize = (int)sizeof(T);
    const Dims d = make_dims(esize, M, R, T_, 1), db = make_dims(esize, M, R, bs, 1);
    Carver c = Carver::rounded(ws);
    w.Xt = c.take<T>((size_t)d.Tp * d.Mk);
    w.Am = c.take<T>((size_t)d.Mj * d.Np);
    w.Ht = c.take<T>((size_t)db.Tp * d.Np);
    w.Vt = c.take<T>((size_t)db.Tp * d.Mj);
    w.Q2t = c.take<T>((size_t)db.Tp * d.Mj);
    w.part = c.take<T>((size_t)LEARN_MAX_SPLITS * 2 * learn_bin_tiles(M) * 16 * d.Np);
    w.sums = c.take<double>((size_t)2 * online_blocks(M, R));
    w.stats = c.take<double>(4);
    w.beta_bytes = beta_workspace_bytes(M, R, T_, n_batches, esize == 8 ? EVC_F64 : EVC_F32);
    w.beta_ws = c.take<char>(w.beta_bytes);
    w.bytes = c.bytes();
    return w;
}

inline bool online_sizes_ok(int M, int R, int T_, int dtype) {
    return M >= 1 && R >= 1 && T_ >= 1 && M <= BETA_MAX_M && R <= LEARN_MAX_R && (dtype == EVC_F64 || dtype == EVC_F32);
}

inline size_t online_workspace_bytes(int M, int R, int T_, int batch_size, int dtype) {
    if (!online_sizes_ok(M, R, T_, dtype) || batch_size < 1) return 0;
    const int bs = batch_size < T_ ? batch_size : T_, nb = (T_ + bs - 1) / bs;
    return (dtype == EVC_F64 ? carve_online<double>(nullptr, M, R, T_, bs, nb).bytes
                             : carve_online<float>(nullptr, M, R, T_, bs, nb).bytes) + 256;
}

// _minibatch_convergence on the host: step() takes one step's figures and says whether the loop ends with it
struct OnlineStop {
    double tol;
    int max_no_improvement;     // < 0: off
    int T_;
    bool have_ewa = false, have_min = false;
    double ewa = 0.0, ewa_min = 0.0;
    int no_improvement = 0;
    bool step(long k, int frames, double cost, double change) {        // k = 1, 2, ...
        if (k == 1) return false;
        if (!have_ewa) {
            ewa = cost;
            have_ewa = true;
        } else {
            double alpha = (double)frames / ((double)T_ + 1.0);
            alpha = alpha < 1.0 ? alpha : 1.0;
            ewa = ewa * (1.0 - alpha) + cost * alpha;
        }
        if (tol > 0.0 && change <= tol) return true;
        if (!have_min || ewa < ewa_min) {
            no_improvement = 0;
            ewa_min = ewa;
            have_min = true;
        } else {
            ++no_improvement;
        }
        return max_no_improvement >= 0 && no_improvement >= max_no_improvement;
    }
};

inline int online_splits(int M, int R, int batch_frames) {
    return online_sizes_ok(M, R, batch_frames, EVC_F64) ? learn_splits(M, R, batch_frames) : 0;
}

// evc_online_learn's argument checks, in the order of its statuses: ST_BADARG, ST_UNSUPPORTED, ST_WORKSPACE before any device
// work.  *forced: the frame ranges bits 8..15 of `reserved` ask for (0: learn_splits decides); *fused: the dictionary route.
inline int online_args_check(const void* X, int ldx, const void* W, int ldw, const void* H, int ldh, const void* acc_a,
                             const void* acc_b, int ld_acc, int M, int R, int T, const evc_online_opts* opts,
                             const void* workspace, size_t workspace_bytes, int* forced, bool* fused) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_online_opts)) return ST_BADARG;
    const evc_online_opts& o = *opts;
    HIP_TRY(learn_args_ok(M, R, T, o.dtype, o.layout, X, W, H, workspace, ldx, ldw, ldh, o.reserved, 0x3ff00, forced));
    const int route = (o.reserved >> 16) & 3;
    if (!acc_a || !acc_b || bad_ld(o.layout, ld_acc, R, M)) return ST_BADARG;
    if (o.batch_size < 1 || o.max_iter < 0 || route == 3 || (o.resume != 0 && o.resume != 1)) return ST_BADARG;
    if (!(o.beta - o.beta == 0.0)) return ST_BADARG;               // NaN or infinite
    if (!(o.tol >= 0.0) || !(o.l1_h >= 0.0) || !(o.l2_h >= 0.0) || !(o.l1_w >= 0.0) || !(o.l2_w >= 0.0)) return ST_BADARG;
    if (!(o.forget_factor > 0.0 && o.forget_factor <= 1.0)) return ST_BADARG;
    const int bs = o.batch_size < T ? o.batch_size : T, nb = (T + bs - 1) / bs;
    if ((long)o.max_iter * nb > 0x7fffffffL) return ST_BADARG;      // n_steps_out is an int
    if (M > BETA_MAX_M || R > LEARN_MAX_R) return ST_UNSUPPORTED;
    if (route == ROUTE_FUSED && R > BDG_MAX_R) return ST_UNSUPPORTED;
    if (workspace_bytes < online_workspace_bytes(M, R, T, o.batch_size, o.dtype)) return ST_WORKSPACE;
    *fused = route == ROUTE_FUSED || (route == ROUTE_AUTO && R <= BDG_ROUTE_R);
    return ST_OK;
}

// ----- evc_online_learn_fresh: the same learner with MiniBatchNMF's fresh restarts -----
// what the fresh-restart entry adds to the step (NULL for evc_online_learn): the iterations of a step's activation solve and
// of the solve over all frames that ends the fit (0: none)
struct FreshPlan {
    int fresh_max_iter, final_max_iter;
    int slots() const { const int k = fresh_max_iter > final_max_iter ? fresh_max_iter : final_max_iter; return k > 0 ? k : 1; }
};

struct FreshWs {
    char *online_ws, *final_ws;
    double* chg;            // [tiles * 16][2] the change variant's per-frame shares: the batches' table or the final solve's
    size_t online_bytes, final_bytes, bytes;
};

// [evc_online_learn's workspace | chg | the final solve's activation half], each 256-byte aligned (ws == NULL: sizes only).
// Batches start at tile boundaries, so the final solve over all frames as one utterance has a tile table of its own: it
// gets a second activation half (n_utt = 1) rather than a second table squeezed into the first.
inline FreshWs carve_fresh(void* ws, int M, int R, int T_, int batch_size, int dtype) {
    FreshWs w;
    const int bs = batch_size < T_ ? batch_size : T_, nb = (T_ + bs - 1) / bs;
    Carver c = Carver::rounded(ws);
    w.online_bytes = online_workspace_bytes(M, R, T_, batch_size, dtype);
    w.online_ws = c.take<char>(w.online_bytes);
    w.chg = c.take<double>((size_t)frame_tile_cap(T_, BT_F, nb) * BT_F * 2);
    w.final_bytes = beta_workspace_bytes(M, R, T_, 1, dtype);
    w.final_ws = c.take<char>(w.final_bytes);
    w.bytes = c.bytes();
    return w;
}

inline size_t online_fresh_workspace_bytes(int M, int R, int T_, int batch_size, int dtype) {
    if (!online_sizes_ok(M, R, T_, dtype) || batch_size < 1) return 0;
    return carve_fresh(nullptr, M, R, T_, batch_size, dtype).bytes + 256;
}

// the fields evc_online_fresh_opts shares with evc_online_opts, as one of those
inline evc_online_opts online_opts_of(const evc_online_fresh_opts& f) {
    evc_online_opts o;
    o.struct_bytes = (int)sizeof(evc_online_opts);
    o.dtype = f.dtype; o.layout = f.layout; o.batch_size = f.batch_size; o.max_iter = f.max_iter;
    o.max_no_improvement = f.max_no_improvement; o.resume = f.resume; o.reserved = f.reserved;
    o.beta = f.beta; o.tol = f.tol; o.forget_factor = f.forget_factor;
    o.l1_h = f.l1_h; o.l2_h = f.l2_h; o.l1_w = f.l1_w; o.l2_w = f.l2_w;
    o.ev_loop_start = f.ev_loop_start; o.ev_loop_stop = f.ev_loop_stop;
    return o;
}

// evc_online_learn_fresh's argument checks: its own two counts, then evc_online_learn's in their order (ST_BADARG,
// ST_UNSUPPORTED, ST_WORKSPACE against the larger workspace); *o: the shared options, *plan: the two counts
inline int online_fresh_args_check(const void* X, int ldx, const void* W, int ldw, const void* H, int ldh, const void* acc_a,
                                   const void* acc_b, int ld_acc, int M, int R, int T, const evc_online_fresh_opts* opts,
                                   const void* workspace, size_t workspace_bytes, evc_online_opts* o, FreshPlan* plan,
                                   int* forced, bool* fused) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_online_fresh_opts)) return ST_BADARG;
    if (opts->fresh_max_iter < 1 || opts->fresh_max_iter > BETA_MAX_SLOTS) return ST_BADARG;
    if (opts->final_max_iter < 0 || opts->final_max_iter > BETA_MAX_SLOTS) return ST_BADARG;
    *o = online_opts_of(*opts);
    plan->fresh_max_iter = opts->fresh_max_iter;
    plan->final_max_iter = opts->final_max_iter;
    const int st = online_args_check(X, ldx, W, ldw, H, ldh, acc_a, acc_b, ld_acc, M, R, T, o, workspace, (size_t)-1, forced, fused);
    if (st != ST_OK) return st;
    if (workspace_bytes < online_fresh_workspace_bytes(M, R, T, o->batch_size, o->dtype)) return ST_WORKSPACE;
    return ST_OK;
}

}  // namespace evc
