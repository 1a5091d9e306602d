// evc_nmf_learn.  Its dictionary update: W <- W (.) (X H^T) (/) ((W H) H^T), evaluated factored.
//
//   k_dict_grad   the split-T "TN" contraction C[m][r] = sum_t L[t][m] Ht[t][r] on the 16x16x4 MFMA, for the stacked left
//                 operand L = [X; V] (V = W H comes from the existing contraction).  A workgroup owns DG_MB bin tiles of
//                 one operand x 128 components x one contiguous frame range; its accumulators stay in registers for the
//                 whole range and leave as one slab of partial sums.  Operands go from global memory straight into the
//                 MFMA (frames as rows: 16 consecutive bins / components of one frame per quarter wavefront, 128-byte
//                 rows); the wavefronts of a workgroup share the bin tiles through the vector cache.
//                 Its one-operand form (Kullback-Leibler) contracts the quotient Q = X (/) max(V, eps) alone, with no
//                 `which` dimension in the grid, and its first row of workgroups also sums the right operand's rows over
//                 the range (s_r = sum_t H[r][t]) from the registers the MFMAs already read.
//   k_dict_quot   forms Q in V's place, once per dictionary step.
//   k_dict_apply  sums the slabs in the order s = 0 .. S-1 and applies the surface's update to the caller's W.
//   k_dict_colnorm  pymf: every column divided by its Euclidean norm (sum of squares over the bins in ascending order).
//   k_err_total   sqrt of the sum of the per-frame error terms (clamped at 0), in a fixed order.
// Nothing here exchanges data between workgroups inside a launch, uses atomics or assumes residency: the same call gives
// bitwise the same W every time.
// Below the kernels: evc_nmf_learn itself - its workspace, its steps for learn_loop (evc_internal.h) and its C entries.
#include "evc_internal.h"

#include <math.h>

namespace evc {

int learn_splits(int M, int R, int T_) {
    const int blocks = (round_up(R, 128) / 128) * (2 * learn_bin_tiles(M) / DG_MB);
    int S = (1024 + blocks - 1) / blocks;          // about four workgroups per compute unit of a 256-CU device
    S = S < T_ / 256 ? S : T_ / 256;               // ... of at least 256 frames each
    S = S > LEARN_MAX_SPLITS ? LEARN_MAX_SPLITS : S;
    return S < 1 ? 1 : S;
}

// V <- X (/) max(V, eps) in place (m < M; zero in the padding up to ldx columns), frames as rows
template <typename T>
__global__ __launch_bounds__(256) void k_dict_quot(const T* __restrict__ Xt, int ldx, T* __restrict__ Vt, int ldv, int M,
                                                   long rows, T eps) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= rows * ldx) return;
    const long t = gid / ldx;
    const int m = (int)(gid % ldx);
    T q = T(0);
    if (m < M) {
        T v = Vt[t * ldv + m];
        v = (v < eps) ? eps : v;
        q = Xt[t * ldx + m] / v;
    }
    Vt[t * ldv + m] = q;
}

// ONE: the left operand is Vt alone (Xt is not read), the grid has no `which` dimension, and the workgroups with
// blockIdx.y == 0 leave the sums of Ht's columns over the range in the first row of the range's second slab
template <typename T, bool ONE>
__global__ __launch_bounds__(64 * DG_WAVES) void k_dict_grad(const T* __restrict__ Xt, int ldx, const T* __restrict__ Vt,
                                                             int ldv, const T* __restrict__ Ht, int ldh, int MT, int MTp,
                                                             int T_, int S, T* __restrict__ part) {
    typedef typename Mma<T>::acc_t acc_t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bpo = MTp / DG_MB;                   // workgroups per operand along the bins
    const int which = ONE ? 1 : blockIdx.y / bpo;
    const int tile0 = (ONE ? blockIdx.y : blockIdx.y % bpo) * DG_MB;
    const bool sums = ONE && blockIdx.y == 0;
    const int r0 = (blockIdx.x * DG_WAVES + wave) * DG_RB * 16;
    const int sp = blockIdx.z;
    const int tb = (int)((long)sp * T_ / S), te = (int)((long)(sp + 1) * T_ / S);
    const T* __restrict__ L = which ? Vt : Xt;
    const int ldl = which ? ldv : ldx;
    int moff[DG_MB];
#pragma unroll
    for (int i = 0; i < DG_MB; ++i) {              // tiles past the last one repeat it: their sums land in padding
        const int tile = tile0 + i < MT ? tile0 + i : MT - 1;
        moff[i] = tile * 16 + (lane & 15);
    }
    acc_t acc[DG_MB][DG_RB];
#pragma unroll
    for (int i = 0; i < DG_MB; ++i)
#pragma unroll
        for (int j = 0; j < DG_RB; ++j) acc[i][j] = acc_t{0, 0, 0, 0};
    const int hoff = r0 + (lane & 15);
    // one step = 4 frames; the next step's operands are loaded before the current step's MFMAs are issued
    auto load = [&](int t, T (&a)[DG_MB], T (&b)[DG_RB]) {
        const int tt = t + (lane >> 4);
        const bool live = tt < te;                 // a ragged range: the frames past its end contribute zeros
        const long row = live ? tt : te - 1;
        const T* __restrict__ lrow = L + row * ldl;
        const T* __restrict__ hrow = Ht + row * ldh + hoff;
#pragma unroll
        for (int i = 0; i < DG_MB; ++i) a[i] = lrow[moff[i]];
#pragma unroll
        for (int j = 0; j < DG_RB; ++j) b[j] = hrow[16 * j];
#pragma unroll
        for (int i = 0; i < DG_MB; ++i) a[i] = live ? a[i] : T(0);
#pragma unroll
        for (int j = 0; j < DG_RB; ++j) b[j] = live ? b[j] : T(0);
    };
    T a[DG_MB], b[DG_RB], hs[DG_RB];
#pragma unroll
    for (int j = 0; j < DG_RB; ++j) hs[j] = T(0);
    if (tb < te) load(tb, a, b);
    for (int t = tb; t < te; t += 4) {
        T an[DG_MB], bn[DG_RB];
        load(t + 4, an, bn);                       // past the end: the clamped row, masked to zeros, never used
        if (sums) {                                // this lane's frames t + (lane >> 4), t + 4 + (lane >> 4), ...
#pragma unroll
            for (int j = 0; j < DG_RB; ++j) hs[j] += b[j];
        }
#pragma unroll
        for (int i = 0; i < DG_MB; ++i)
#pragma unroll
            for (int j = 0; j < DG_RB; ++j) acc[i][j] = Mma<T>::mma(a[i], b[j], acc[i][j]);
#pragma unroll
        for (int i = 0; i < DG_MB; ++i) a[i] = an[i];
#pragma unroll
        for (int j = 0; j < DG_RB; ++j) b[j] = bn[j];
    }
    const long slab = (long)MTp * 16 * ldh;
    T* __restrict__ out = part + ((long)sp * 2 + (ONE ? 0 : which)) * slab;
#pragma unroll
    for (int i = 0; i < DG_MB; ++i)
#pragma unroll
        for (int j = 0; j < DG_RB; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                out[(long)((tile0 + i) * 16 + Mma<T>::row(lane, r)) * ldh + hoff + 16 * j] = acc[i][j][r];
    if (sums) {                                    // the four lane groups of a component, added in ascending order
#pragma unroll
        for (int j = 0; j < DG_RB; ++j) {
            const int c = lane & 15;
            const T s01 = __shfl(hs[j], c, 64) + __shfl(hs[j], c + 16, 64);
            const T s = (s01 + __shfl(hs[j], c + 32, 64)) + __shfl(hs[j], c + 48, 64);
            if (lane < 16) out[slab + hoff + 16 * j] = s;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_dict_apply(const T* __restrict__ part, int S, long slab, int ldp, T* __restrict__ W,
                                                    long ldw, int bin_major, int M, int R, int surface, int loss) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)M * R) return;
    // the caller's inner index is the fastest one here
    const int m = bin_major ? (int)(idx / R) : (int)(idx % M);
    const int r = bin_major ? (int)(idx % R) : (int)(idx / M);
    const T* __restrict__ p = part + (long)m * ldp + r;
    T num = T(0), den = T(0);
    if (loss == EVC_LOSS_KL) {                     // sklearn _nmf.py:634-728 (beta 1) with the roles swapped
        for (int s = 0; s < S; ++s) {
            num += p[(long)s * 2 * slab];
            den += part[((long)s * 2 + 1) * slab + r];         // s_r: the first row of the range's second slab
        }
        den = den == T(0) ? T(1) : den;            // _nmf.py:679-680: an absent component divides by 1, not by eps
        T* w = W + (bin_major ? m * ldw + r : r * ldw + m);
        *w = *w * (num / den);
        return;
    }
    for (int s = 0; s < S; ++s) {
        num += p[(long)s * 2 * slab];
        den += p[((long)s * 2 + 1) * slab];
    }
    T* w = W + (bin_major ? m * ldw + r : r * ldw + m);
    if (surface == EVC_LEARN_PYMF) {               // pymf nmf.py:72-76: W *= num; W /= (den + 1e-9)
        *w = (*w * num) / (den + T(1e-9));
    } else {                                       // sklearn _nmf.py:620-629 with the roles swapped
        den = den == T(0) ? T(1.1920929e-7) : den;
        *w = *w * (num / den);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_dict_colnorm(T* __restrict__ W, long ldw, int bin_major, int M, int R) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const long sm = bin_major ? ldw : 1;
    T* __restrict__ col = W + (bin_major ? (long)r : r * ldw);
    T ss = T(0);
    for (int m = 0; m < M; ++m) {
        const T v = col[m * sm];
        ss += v * v;
    }
    const T n = sqrt(ss);                          // a zero column: 0 / 0 = NaN, as in pymf
    for (int m = 0; m < M; ++m) col[m * sm] = col[m * sm] / n;
}

__global__ __launch_bounds__(256) void k_err_total(const double* __restrict__ err2, int T_, double* __restrict__ out) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int t = threadIdx.x; t < T_; t += 256) acc += err2[t];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    // the Kullback-Leibler terms can sum to a rounding error below zero at an exact fit (k_utt_check clamps likewise)
    if (threadIdx.x == 0) *out = sqrt(red[0] < 0.0 ? 0.0 : red[0]);
}

template <typename T>
hipError_t dict_grad(const T* Xt, int ldx, const T* Vt, int ldv, const T* Ht, int ldh, int M, int T_, int S, T* part,
                     hipStream_t s) {
    const int MT = round_up(M, 16) / 16, MTp = learn_bin_tiles(M);
    const dim3 grid(ldh / (DG_WAVES * DG_RB * 16), 2 * MTp / DG_MB, S);
    hipLaunchKernelGGL((k_dict_grad<T, false>), grid, dim3(64 * DG_WAVES), 0, s, Xt, ldx, Vt, ldv, Ht, ldh, MT, MTp, T_, S,
                       part);
    return hipGetLastError();
}

template <typename T>
hipError_t dict_quot(const T* Xt, int ldx, T* Vt, int ldv, int M, int T_, double eps, hipStream_t s) {
    const long n = (long)T_ * ldx;
    hipLaunchKernelGGL(k_dict_quot<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Xt, ldx, Vt, ldv, M, (long)T_,
                       (T)eps);
    return hipGetLastError();
}

template <typename T>
hipError_t dict_grad_kl(const T* Qt, int ldq, const T* Ht, int ldh, int M, int T_, int S, T* part, hipStream_t s) {
    const int MT = round_up(M, 16) / 16, MTp = learn_bin_tiles(M);
    const dim3 grid(ldh / (DG_WAVES * DG_RB * 16), MTp / DG_MB, S);
    hipLaunchKernelGGL((k_dict_grad<T, true>), grid, dim3(64 * DG_WAVES), 0, s, (const T*)nullptr, 0, Qt, ldq, Ht, ldh, MT,
                       MTp, T_, S, part);
    return hipGetLastError();
}

template <typename T>
hipError_t dict_apply(const T* part, int S, int ldp, T* W, long ldw, int bin_major, int M, int R, int surface, int loss,
                      hipStream_t s) {
    const long slab = (long)learn_bin_tiles(M) * 16 * ldp;
    const long n = (long)M * R;
    hipLaunchKernelGGL(k_dict_apply<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, S, slab, ldp, W, ldw,
                       bin_major, M, R, surface, loss);
    if (surface == EVC_LEARN_PYMF)
        hipLaunchKernelGGL(k_dict_colnorm<T>, dim3((R + 255) / 256), dim3(256), 0, s, W, ldw, bin_major, M, R);
    return hipGetLastError();
}

hipError_t err_total(const double* err2, int T_, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_err_total, dim3(1), dim3(256), 0, s, err2, T_, out);
    return hipGetLastError();
}

template hipError_t dict_grad<double>(const double*, int, const double*, int, const double*, int, int, int, int, double*,
                                      hipStream_t);
template hipError_t dict_grad<float>(const float*, int, const float*, int, const float*, int, int, int, int, float*,
                                     hipStream_t);
template hipError_t dict_quot<double>(const double*, int, double*, int, int, int, double, hipStream_t);
template hipError_t dict_quot<float>(const float*, int, float*, int, int, int, double, hipStream_t);
template hipError_t dict_grad_kl<double>(const double*, int, const double*, int, int, int, int, double*, hipStream_t);
template hipError_t dict_grad_kl<float>(const float*, int, const float*, int, int, int, int, float*, hipStream_t);
template hipError_t dict_apply<double>(const double*, int, int, double*, long, int, int, int, int, int, hipStream_t);
template hipError_t dict_apply<float>(const float*, int, int, float*, long, int, int, int, int, int, hipStream_t);

// ---- evc_nmf_learn: the host driver.  The activation step is one update of evc_nmf_solve, the dictionary step the
// kernels above; learn_loop (evc_internal.h) alternates them and applies the surface's stop rule ----
namespace {

template <typename T> struct LearnWs {
    T *Xt, *Am, *Ht, *Vt, *part;
    double *err2, *ring;
    char* solve_ws;
    size_t solve_bytes, bytes;
};
constexpr int LEARN_RING = 64;

template <typename T> LearnWs<T> carve_learn(void* base, const Dims& d) {
    LearnWs<T> w;
    Carver c{static_cast<char*>(base), 0};
    w.Xt = c.take<T>((size_t)d.Tp * d.Mk);
    w.Am = c.take<T>((size_t)d.Mj * d.Np);
    w.Ht = c.take<T>((size_t)d.Tp * d.Np);
    w.Vt = c.take<T>((size_t)d.Tp * d.Mj);
    w.part = c.take<T>((size_t)LEARN_MAX_SPLITS * 2 * learn_bin_tiles(d.M) * 16 * d.Np);
    w.err2 = c.take<double>(d.Tp);
    w.ring = c.take<double>(LEARN_RING);
    w.solve_bytes = evc_workspace_bytes(d.M, 0, d.N, d.T_, 1, sizeof(T) == 8 ? EVC_F64 : EVC_F32, EVC_ALGO_AUTO);
    w.solve_ws = c.take<char>(w.solve_bytes);
    w.bytes = c.bytes();
    return w;
}

template <typename T>
int learn_typed(const void* X_, int ldx, void* W_, int ldw, void* H_, int ldh, int M, int R, int T_,
                const evc_learn_opts& o, int S, void* workspace, size_t workspace_bytes, int* n_iter_out, double* err_out,
                hipStream_t s) {
    const Dims d = make_dims((int)sizeof(T), M, R, T_, 1, 0);
    const LearnWs<T> w = carve_learn<T>(workspace, d);
    if (w.bytes > workspace_bytes) return ST_WORKSPACE;
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    const T* X = static_cast<const T*>(X_);
    T* W = static_cast<T*>(W_);
    T* H = static_cast<T*>(H_);
    const bool pymf = o.surface == EVC_LEARN_PYMF;
    const bool kl = o.loss == EVC_LOSS_KL;         // sklearn surface only (evc_nmf_learn rejects it with pymf)
    const double eps_kl = 1.1920929e-7;

    evc_solve_opts so{};                           // the activation step: one update of the existing solve, a pure enqueue
    so.struct_bytes = (int)sizeof(evc_solve_opts);
    so.dtype = o.dtype; so.layout = o.layout; so.algo = EVC_ALGO_AUTO; so.iters = 1;
    so.eps_mode = pymf ? EVC_EPS_ADD : EVC_EPS_ZERO_REPLACE;
    so.eps = pymf ? 1e-9 : 1.1920929e-7;
    so.init_mode = EVC_INIT_GIVEN; so.stop_rule = EVC_STOP_NONE; so.reserved = EVC_FLAG_NO_EXCHANGE;
    so.loss = kl ? EVC_LOSS_KL : EVC_LOSS_FROBENIUS;
    auto update_h = [&]() -> int {
        return evc_nmf_solve(W, ldw, X, ldx, H, ldh, M, R, T_, nullptr, 1, &so, w.solve_ws, w.solve_bytes, nullptr, nullptr,
                             reinterpret_cast<evc_stream_t>(s));
    };
    // V = W H on frames-as-rows copies of the current factors (Ht is the dictionary update's right operand too)
    auto form_v = [&]() -> int {
        HIP_TRY(copy2d<T>(W, ldw, M, R, fm ? 1 : 0, w.Am, d.Np, d.Mj, d.Np, 0, s));
        HIP_TRY(copy2d<T>(H, ldh, T_, R, fm ? 0 : 1, w.Ht, d.Np, d.Tp, d.Np, 0, s));
        HIP_TRY(gemm_nt<T>(w.Ht, d.Np, w.Am, d.Np, w.Vt, d.Mj, d.Tp, d.Mj, d.Np, s, nullptr, 0, nullptr, d.Mk));
        return ST_OK;
    };
    auto update_w = [&]() -> int {
        HIP_TRY(form_v());
        if (kl) {                                  // nothing below reads V again: the quotient takes its place
            HIP_TRY(dict_quot<T>(w.Xt, d.Mk, w.Vt, d.Mj, M, T_, eps_kl, s));
            HIP_TRY(dict_grad_kl<T>(w.Vt, d.Mj, w.Ht, d.Np, M, T_, S, w.part, s));
        } else {
            HIP_TRY(dict_grad<T>(w.Xt, d.Mk, w.Vt, d.Mj, w.Ht, d.Np, M, T_, S, w.part, s));
        }
        HIP_TRY(dict_apply<T>(w.part, S, d.Np, W, ldw, fm ? 0 : 1, M, R, o.surface, o.loss, s));
        return ST_OK;
    };
    auto step = [&]() -> int {                     // pymf: W, then H; scikit-learn: H, then W
        HIP_TRY(pymf ? update_w() : update_h());
        return pymf ? update_h() : update_w();
    };
    auto error_now = [&](int slot, double* host) -> int {
        HIP_TRY(form_v());
        if (kl) HIP_TRY(frame_err_kl<T>(w.Xt, d.Mk, w.Vt, d.Mj, M, T_, eps_kl, w.err2, s));
        else HIP_TRY(frame_err2<T>(w.Xt, d.Mk, w.Vt, d.Mj, M, T_, w.err2, s));
        double* dst = w.ring + slot % LEARN_RING;
        HIP_TRY(err_total(w.err2, T_, dst, s));
        HIP_TRY(hipMemcpyAsync(host, dst, sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return ST_OK;
    };
    auto stop = [&](int c, double err, double err_prev, double err_init) {
        return pymf ? (c >= 3 && fabs(err - err_prev) / T_ < o.tol) : ((err_prev - err) / err_init < o.tol);
    };

    HIP_TRY(copy2d<T>(X, ldx, T_, M, fm ? 0 : 1, w.Xt, d.Mk, d.Tp, d.Mk, 0, s));
    return learn_loop(o.iters, o.check_every, o.tol, err_out, n_iter_out, o.ev_loop_start, o.ev_loop_stop, s, step, error_now,
                      stop);
}

bool learn_sizes_ok(int M, int R, int T, int dtype) {
    return M >= 1 && R >= 1 && T >= 1 && M <= LEARN_MAX_M && R <= LEARN_MAX_R && (dtype == EVC_F64 || dtype == EVC_F32);
}

}  // namespace

}  // namespace evc

using namespace evc;

extern "C" {

size_t evc_learn_workspace_bytes(int M, int R, int T, int dtype) {
    if (!learn_sizes_ok(M, R, T, dtype)) return 0;
    if (dtype == EVC_F64) return carve_learn<double>(nullptr, make_dims(8, M, R, T, 1, 0)).bytes;
    return carve_learn<float>(nullptr, make_dims(4, M, R, T, 1, 0)).bytes;
}

int evc_learn_splits(int M, int R, int T) {
    return learn_sizes_ok(M, R, T, EVC_F64) ? learn_splits(M, R, T) : 0;
}

int evc_nmf_learn(const void* X, int ldx, void* W, int ldw, void* H, int ldh, int M, int R, int T,
                  const evc_learn_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out, double* err_out,
                  evc_stream_t stream) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_learn_opts)) return ST_BADARG;
    const evc_learn_opts& o = *opts;
    int forced;
    HIP_TRY(learn_args_ok(M, R, T, o.dtype, o.layout, X, W, H, workspace, ldx, ldw, ldh, o.reserved, 0xff00, &forced));
    if (o.iters < 0 || o.check_every < 0 || !(o.tol >= 0.0)) return ST_BADARG;
    if (o.surface != EVC_LEARN_SKLEARN && o.surface != EVC_LEARN_PYMF) return ST_BADARG;
    if (o.loss != EVC_LOSS_FROBENIUS && o.loss != EVC_LOSS_KL) return ST_BADARG;
    if (M > LEARN_MAX_M || R > LEARN_MAX_R) return ST_UNSUPPORTED;
    if (o.loss == EVC_LOSS_KL && o.surface == EVC_LEARN_PYMF) return ST_UNSUPPORTED;   // pymf has no KL update
    if (o.check_every > 0 && o.iters / o.check_every + 1 > MAX_SLOTS) return ST_BADARG;
    if (workspace_bytes < evc_learn_workspace_bytes(M, R, T, o.dtype)) return ST_WORKSPACE;
    const int S = forced ? forced : learn_splits(M, R, T);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return (o.dtype == EVC_F64 ? learn_typed<double> : learn_typed<float>)(X, ldx, W, ldw, H, ldh, M, R, T, o, S, workspace,
                                                                            workspace_bytes, n_iter_out, err_out, s);
}

}  // extern "C"
