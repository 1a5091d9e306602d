// evc_online.hip - evc_online_learn: mini-batch dictionary learning under any beta-divergence: scikit-learn's
// MiniBatchNMF._fit_transform with init='custom' and fresh_restarts=False (_nmf.py: _minibatch_step,
// _multiplicative_update_h(..., A, B, rho), _minibatch_convergence).  DESIGN.md §5.12.
//
// Batches are contiguous ranges of bs = min(batch_size, T) frames, in order and cycled (the last of a pass may be short).
// They are handed to beta_begin as utterances: a frame tile never straddles two batches, and a step launches the
// activation kernels over its batch's tiles only (BetaArgs.tile0).  Step k on batch b of T_b frames:
//   activations  one k_beta_sweep on the batch's columns of H with the current W (its packed images are rebuilt every
//                step); H_b[H_b < 2^-52] = 0 at the store when beta < 1
//   cost         k_beta_err leaves every frame's share of the divergence; k_online_stats sums the batch's shares and the
//                penalty terms: cost = (res + l1_h sum H_b + T_b l1_w sum W + l2_h sum H_b^2 + T_b l2_w sum W^2) / T_b
//   dictionary   Num and Den over the batch's frames in learn_splits(M, R, T_b) ranges by evc_beta_learn's kernels
//                (beta_dict_sums, either route); k_online_apply sums the slabs in ascending order and, per element,
//                  Den += T_b l1_w + T_b l2_w W, 0 -> EPS;  P = W^(1/gamma);  A <- rho A + Num P;  B <- rho B + Den;
//                  W <- (A / B)^gamma;  W[W < 2^-52] = 0 if beta <= 1
//                and leaves per-workgroup partial sums of (W_new - W_old)^2 and W_new^2 in float64
//   convergence  k_online_stats adds those partial sums in index order; the host reads {cost, sum dW^2, sum W^2} and
//                decides as _minibatch_convergence does (OnlineStop)
// The argument checks, the workspace carving and OnlineStop are host-only code in evc_online_plan.h, which a stand-alone
// program runs under the host sanitizers (tests/online_host_main.hip).
// With the stop rules off and nothing asked back, the cost kernels are not launched and the call is a pure enqueue.
// evc_online_learn_fresh is the same driver with MiniBatchNMF's fresh_restarts=True (`fresh` below): a step's activations
// are not one carried update but a whole _solve_W on the batch - the stop word cleared, the batch's columns of H refilled
// with sqrt(mean(X_b) / R), up to fresh_max_iter change-variant sweeps stopped on the device by tol (beta_sweep_change,
// evc_beta.hip), then the flush as a pass of its own - and the fit ends with one such solve over all frames as one
// utterance (final_max_iter), which has an activation half of its own because batches start at tile boundaries.  DESIGN.md
// §5.13.
// Nothing here exchanges data between workgroups inside a launch, uses float atomics or assumes residency: the same call
// gives bitwise the same W, H, A and B every time.
#include "evc_online_plan.h"

#include <math.h>

namespace evc {

namespace {

// sums a slab pair in the order s = 0 .. S-1 and applies the online update to the caller's W, A and B (all addressed
// alike: bin_major W[m ld + r], else W[r ld + m]); sums[2 block], sums[2 block + 1] = the block's share of
// sum (W_new - W_old)^2 and sum W_new^2, added in a fixed order
template <typename T>
__global__ __launch_bounds__(256) void k_online_apply(const T* __restrict__ part, int S, long slab, int ldp,
                                                      T* __restrict__ W, long ldw, T* __restrict__ A, T* __restrict__ B,
                                                      long ldacc, int bin_major, int M, int R, T l1, T l2, T rho,
                                                      int gamma_one, PowSpec pgi, PowSpec pg, T flush,
                                                      double* __restrict__ sums) {
    __shared__ double red[2][256];
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    double d2 = 0.0, w2 = 0.0;
    if (idx < (long)M * R) {
        // the caller's inner index is the fastest one here
        const int m = bin_major ? (int)(idx / R) : (int)(idx % M);
        const int r = bin_major ? (int)(idx % R) : (int)(idx / M);
        const T* __restrict__ p = part + (long)m * ldp + r;
        T num = T(0), den = T(0);
        for (int s = 0; s < S; ++s) {
            num += p[(long)s * 2 * slab];
            den += p[((long)s * 2 + 1) * slab];
        }
        T* wp = W + (bin_major ? m * ldw + r : r * ldw + m);
        const long oa = bin_major ? m * ldacc + r : r * ldacc + m;
        const T w = *wp;
        T d = den + l1;
        d = d + l2 * w;
        d = d == T(0) ? (T)BETA_EPS : d;
        const T pw_ = gamma_one ? w : pw(w, pgi);
        const T a = rho * A[oa] + num * pw_;
        const T b = rho * B[oa] + d;
        T wn = a / b;
        if (!gamma_one) wn = pw(wn, pg);
        if (flush > T(0) && wn < flush) wn = T(0);
        A[oa] = a;
        B[oa] = b;
        *wp = wn;
        const double dw = (double)wn - (double)w;
        d2 = dw * dw;
        w2 = (double)wn * (double)wn;
    }
    red[0][threadIdx.x] = d2;
    red[1][threadIdx.x] = w2;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
            red[0][threadIdx.x] += red[0][threadIdx.x + h];
            red[1][threadIdx.x] += red[1][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sums[2 * (long)blockIdx.x] = red[0][0];
        sums[2 * (long)blockIdx.x + 1] = red[1][0];
    }
}

// a fresh start: A = W, B = 1
template <typename T>
__global__ __launch_bounds__(256) void k_online_init(const T* __restrict__ W, long ldw, T* __restrict__ A,
                                                     T* __restrict__ B, long ldacc, int bin_major, int M, int R) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)M * R) return;
    const int m = bin_major ? (int)(idx / R) : (int)(idx % M);
    const int r = bin_major ? (int)(idx % R) : (int)(idx / M);
    const long oa = bin_major ? m * ldacc + r : r * ldacc + m;
    A[oa] = W[bin_major ? m * ldw + r : r * ldw + m];
    B[oa] = T(1);
}

struct OnlineStatsArgs {
    const double* errf;     // per-frame shares of the divergence; the batch's are [e0, e1)
    long e0, e1;
    const double* sums;     // k_online_apply's [n_blocks][2]
    int n_blocks;
    int rows_h, rows_w, R;  // the batch's frames, M, R: the frames-as-rows copy of H_b and the bins-as-rows copy of W_old
    int ld;                 // row length of both copies
    double l1_h, l2_h, l1_w, l2_w;      // l1_w, l2_w already multiplied by the batch's frames
    double frames;
    double* out;            // {cost, sum (W_new - W_old)^2, sum W_new^2}
};

// one workgroup: every sum in float64, each thread over its stride in ascending order, then a tree over the threads
template <typename T>
__global__ __launch_bounds__(256) void k_online_stats(OnlineStatsArgs a, const T* __restrict__ Ht, const T* __restrict__ Wm) {
    __shared__ double red[7][256];
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long i = a.e0 + threadIdx.x; i < a.e1; i += 256) v[0] += a.errf[i];
    for (int i = threadIdx.x; i < a.n_blocks; i += 256) {
        v[1] += a.sums[2 * (long)i];
        v[2] += a.sums[2 * (long)i + 1];
    }
    if (a.l1_h > 0.0 || a.l2_h > 0.0)
        for (long i = threadIdx.x; i < (long)a.rows_h * a.R; i += 256) {
            const double h = (double)Ht[(i / a.R) * a.ld + i % a.R];
            v[3] += h;
            v[4] += h * h;
        }
    if (a.l1_w > 0.0 || a.l2_w > 0.0)
        for (long i = threadIdx.x; i < (long)a.rows_w * a.R; i += 256) {
            const double w = (double)Wm[(i / a.R) * a.ld + i % a.R];
            v[5] += w;
            v[6] += w * w;
        }
#pragma unroll
    for (int j = 0; j < 7; ++j) red[j][threadIdx.x] = v[j];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int j = 0; j < 7; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double cost = red[0][0];
    if (a.l1_h > 0.0) cost += a.l1_h * red[3][0];
    if (a.l1_w > 0.0) cost += a.l1_w * red[5][0];
    if (a.l2_h > 0.0) cost += a.l2_h * red[4][0];
    if (a.l2_w > 0.0) cost += a.l2_w * red[6][0];
    a.out[0] = cost / a.frames;
    a.out[1] = red[1][0];
    a.out[2] = red[2][0];
}

// arguments already validated by the entry; returns ST_OK, ST_WORKSPACE or a hipError_t.  fresh: NULL for evc_online_learn,
// else evc_online_learn_fresh's counts, with fw its two extra pieces of workspace
template <typename T>
int online_learn(const void* X_, int ldx, void* W_, int ldw, void* H_, int ldh, void* A_, void* B_, int ldacc, int M, int R,
                 int T_, const evc_online_opts& o, int forced, bool fused, void* ws, size_t ws_bytes, int* n_iter_out,
                 int* n_steps_out, double* trace_out, hipStream_t s, const FreshPlan* fresh, const FreshWs* fw) {
    const int bs = o.batch_size < T_ ? o.batch_size : T_, nb = (T_ + bs - 1) / bs;
    const OnWs<T> w = carve_online<T>(ws, M, R, T_, bs, nb);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const Dims d = make_dims((int)sizeof(T), M, R, T_, 1);
    const int MTp = learn_bin_tiles(M);
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    const T* X = static_cast<const T*>(X_);
    T* W = static_cast<T*>(W_);
    T* H = static_cast<T*>(H_);
    T* A = static_cast<T*>(A_);
    T* B = static_cast<T*>(B_);
    const double beta = o.beta;
    const long total = (long)o.max_iter * nb;
    const bool reads = o.tol > 0.0 || o.max_no_improvement >= 0 || n_iter_out || n_steps_out || trace_out;
    if (trace_out) for (long i = 0; i < 2 * total; ++i) trace_out[i] = __builtin_nan("");

    if (!o.resume) {
        hipLaunchKernelGGL(k_online_init<T>, dim3(online_blocks(M, R)), dim3(256), 0, s, W, (long)ldw, A, B, (long)ldacc,
                           fm ? 0 : 1, M, R);
        HIP_TRY(hipGetLastError());
    }
    long n_steps = 0;
    if (total > 0) {
        int* offs = static_cast<int*>(malloc(sizeof(int) * ((size_t)nb + 1)));
        if (!offs) return (int)hipErrorOutOfMemory;
        for (int b = 0; b < nb; ++b) offs[b] = b * bs;
        offs[nb] = T_;
        BetaCtx<T> c;
        // a plain step flushes at the sweep's store; a fresh step's solve must not (an entry flushed mid-solve could never
        // recover): it flushes once, afterwards
        const int st = beta_begin<T>(c, X, ldx, H, ldh, M, R, T_, offs, nb, o.layout, beta, o.l1_h, o.l2_h,
                                     !fresh && beta < 1.0 ? BETA_E64 : 0.0, fresh ? fresh->slots() : 1, w.beta_ws,
                                     w.beta_bytes, s);
        free(offs);
        HIP_TRY(st);
        if (fresh) {
            c.a.chg = fw->chg;
            HIP_TRY(beta_h0<T>(c, s));      // the batches' means never change: once per call
        }
        HIP_TRY(copy2d<T>(X, ldx, T_, M, fm ? 0 : 1, w.Xt, d.Mk, d.Tp, d.Mk, 0, s));
        HIP_TRY(beta_dict_sums_prepare<T>(fused));
        const double gamma = beta_gamma(beta);
        const PowSpec pg = pow_spec(gamma), pgi = pow_spec(1.0 / gamma);
        const double rho = pow(o.forget_factor, (double)bs / (double)T_);
        const int tiles_full = (bs + BT_F - 1) / BT_F;      // tiles of every batch but a short last one
        OnlineStop stop{o.tol, o.max_no_improvement, T_};

        if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
        for (long k = 1; k <= total; ++k) {
            const int b = (int)((k - 1) % nb);
            const int t0 = b * bs, Tb = T_ - t0 < bs ? T_ - t0 : bs;
            BetaCtx<T> cb = c;
            cb.a.tile0 = b * tiles_full;
            cb.n_tiles = (Tb + BT_F - 1) / BT_F;
            HIP_TRY(beta_pack_dict<T>(c, W, ldw, s));
            if (!fresh) {
                HIP_TRY(beta_sweep<T>(cb, s));
            } else {
                cb.utt0 = b;
                cb.n_utt = 1;
                HIP_TRY(beta_restart<T>(cb, true, s));
                for (int it = 1; it <= fresh->fresh_max_iter; ++it) HIP_TRY(beta_sweep_change<T>(cb, it, o.tol, s));
                if (beta < 1.0) HIP_TRY(beta_flush<T>(cb, BETA_E64, s));
                if (reads) HIP_TRY(beta_restart<T>(cb, false, s));      // k_beta_err skips a stopped utterance
            }
            if (reads) HIP_TRY(beta_err<T>(cb, s));
            // frames-as-rows copies of the dictionary and of the batch's new activations
            const int Tpb = frame_pad((int)sizeof(T), Tb);
            HIP_TRY(copy2d<T>(W, ldw, M, R, fm ? 1 : 0, w.Am, d.Np, d.Mj, d.Np, 0, s));
            HIP_TRY(copy2d<T>(H + (fm ? (long)t0 * ldh : (long)t0), ldh, Tb, R, fm ? 0 : 1, w.Ht, d.Np, Tpb, d.Np, 0, s));
            BetaDictSums<T> q;
            q.Xt = w.Xt + (long)t0 * d.Mk; q.Ht = w.Ht; q.Am = w.Am; q.Vt = w.Vt; q.Q2t = w.Q2t; q.part = w.part;
            q.M = M; q.R = R; q.T_ = Tb; q.Tp = Tpb; q.S = forced ? forced : learn_splits(M, R, Tb); q.fused = fused;
            q.beta = beta;
            HIP_TRY(beta_dict_sums<T>(q, s));
            const double l1w = (double)Tb * o.l1_w, l2w = (double)Tb * o.l2_w;
            hipLaunchKernelGGL(k_online_apply<T>, dim3(online_blocks(M, R)), dim3(256), 0, s, w.part, q.S,
                               (long)MTp * 16 * d.Np, d.Np, W, (long)ldw, A, B, (long)ldacc, fm ? 0 : 1, M, R, (T)l1w, (T)l2w,
                               (T)rho, gamma == 1.0 ? 1 : 0, pgi, pg, (T)(beta <= 1.0 ? BETA_E64 : 0.0), w.sums);
            HIP_TRY(hipGetLastError());
            n_steps = k;
            if (!reads) continue;
            OnlineStatsArgs a;
            a.errf = c.w.errf; a.e0 = (long)cb.a.tile0 * BT_F; a.e1 = a.e0 + (long)cb.n_tiles * BT_F;
            a.sums = w.sums; a.n_blocks = online_blocks(M, R);
            a.rows_h = Tb; a.rows_w = M; a.R = R; a.ld = d.Np;
            a.l1_h = o.l1_h; a.l2_h = o.l2_h; a.l1_w = l1w; a.l2_w = l2w;
            a.frames = (double)Tb;
            a.out = w.stats;
            hipLaunchKernelGGL(k_online_stats<T>, dim3(1), dim3(256), 0, s, a, (const T*)w.Ht, (const T*)w.Am);
            HIP_TRY(hipGetLastError());
            double host[3];
            HIP_TRY(hipMemcpyAsync(host, w.stats, sizeof(host), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            const double change = sqrt(host[1]) / sqrt(host[2]);
            if (trace_out) {
                trace_out[2 * (k - 1)] = host[0];
                trace_out[2 * (k - 1) + 1] = change;
            }
            if (stop.step(k, Tb, host[0], change)) break;
        }
        if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    }
    if (fresh && fresh->final_max_iter > 0) {       // _fit_transform's last line: _solve_W over all frames, no flush
        BetaCtx<T> c2;
        HIP_TRY(beta_begin<T>(c2, X, ldx, H, ldh, M, R, T_, nullptr, 1, o.layout, beta, o.l1_h, o.l2_h, 0.0, fresh->slots(),
                              fw->final_ws, fw->final_bytes, s));
        c2.a.chg = fw->chg;
        HIP_TRY(beta_pack_dict<T>(c2, W, ldw, s));
        HIP_TRY(beta_start<T>(c2, EVC_INIT_SKLEARN, 0.0, s));
        for (int it = 1; it <= fresh->final_max_iter; ++it) HIP_TRY(beta_sweep_change<T>(c2, it, o.tol, s));
    }
    if (n_steps_out) *n_steps_out = (int)n_steps;
    if (n_iter_out) *n_iter_out = (int)((n_steps + nb - 1) / nb);
    return ST_OK;
}

}  // namespace

}  // namespace evc

extern "C" {

size_t evc_online_workspace_bytes(int M, int R, int T, int batch_size, int dtype) {
    return evc::online_workspace_bytes(M, R, T, batch_size, dtype);
}

int evc_online_splits(int M, int R, int batch_frames) { return evc::online_splits(M, R, batch_frames); }

int evc_online_learn(const void* X, int ldx, void* W, int ldw, void* H, int ldh, void* acc_a, void* acc_b, int ld_acc, int M,
                     int R, int T, const evc_online_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out,
                     int* n_steps_out, double* trace_out, evc_stream_t stream) {
    using namespace evc;
    int forced;
    bool fused;
    HIP_TRY(online_args_check(X, ldx, W, ldw, H, ldh, acc_a, acc_b, ld_acc, M, R, T, opts, workspace, workspace_bytes, &forced,
                              &fused));
    const evc_online_opts& o = *opts;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return (o.dtype == EVC_F64 ? online_learn<double> : online_learn<float>)(X, ldx, W, ldw, H, ldh, acc_a, acc_b, ld_acc, M,
                                                                              R, T, o, forced, fused, workspace,
                                                                              workspace_bytes, n_iter_out, n_steps_out,
                                                                              trace_out, s, nullptr, nullptr);
}

size_t evc_online_fresh_workspace_bytes(int M, int R, int T, int batch_size, int dtype) {
    return evc::online_fresh_workspace_bytes(M, R, T, batch_size, dtype);
}

int evc_online_learn_fresh(const void* X, int ldx, void* W, int ldw, void* H, int ldh, void* acc_a, void* acc_b, int ld_acc,
                           int M, int R, int T, const evc_online_fresh_opts* opts, void* workspace, size_t workspace_bytes,
                           int* n_iter_out, int* n_steps_out, double* trace_out, evc_stream_t stream) {
    using namespace evc;
    int forced;
    bool fused;
    evc_online_opts o;
    FreshPlan plan;
    HIP_TRY(online_fresh_args_check(X, ldx, W, ldw, H, ldh, acc_a, acc_b, ld_acc, M, R, T, opts, workspace, workspace_bytes, &o,
                                    &plan, &forced, &fused));
    const FreshWs fw = carve_fresh(workspace, M, R, T, o.batch_size, o.dtype);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return (o.dtype == EVC_F64 ? online_learn<double> : online_learn<float>)(X, ldx, W, ldw, H, ldh, acc_a, acc_b, ld_acc, M,
                                                                              R, T, o, forced, fused, fw.online_ws,
                                                                              fw.online_bytes, n_iter_out, n_steps_out,
                                                                              trace_out, s, &plan, &fw);
}

}  // extern "C"
