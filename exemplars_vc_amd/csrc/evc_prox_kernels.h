// evc_prox_kernels.h - the small kernels the two proximal-gradient drivers share: the start, the
// finish and the per-utterance check of the stop statistic, with the helpers of their arithmetic (the per-call state is
// evc_solve_state.h's, which evc_semi.hip includes too) - and prox_solve_frame, the host frame of a call around the driver's
// own preparation and sweep.  Two translation units include this file, evc_prox.hip (evc_prox_solve) and
// evc_prox_masked.hip (evc_prox_masked_solve), each into an unnamed namespace of its own: both get the same device code from
// the same text.  The sweeps themselves stay with their drivers.
#pragma once
#include "evc_prox_plan.h"
#include "evc_solve_state.h"

namespace evc {

namespace {

template <typename T> struct PVec4;
template <> struct PVec4<double> { typedef f64x4 type; };
template <> struct PVec4<float> { typedef f32x4 type; };

__device__ __forceinline__ double pabs(double v) { return __builtin_fabs(v); }
__device__ __forceinline__ float pabs(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double psqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float psqrt(float v) { return sqrtf(v); }
// numpy's maximum: a NaN on either side wins
__device__ __forceinline__ double nanmax(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// over the N x T_ elements: P_n <- P_n / d_n (P == NULL: the caller's P is already in the scaled dictionary);  X_0 = (H | value) d_n,
// left in H and copied to W_0 (normalize == 0: no arithmetic)
template <typename T>
__global__ void k_prox_start(T* __restrict__ P, T* __restrict__ H, long hs_t, long hs_n, T* __restrict__ W0, const T* __restrict__ d,
                             int N, int T_, int n_fast, int normalize, int given, T value) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * T_) return;
    const long t = n_fast ? i / N : i % T_;
    const long n = n_fast ? i % N : i / T_;
    T* ph = H + t * hs_t + n * hs_n;
    T x = given ? *ph : value;
    if (normalize) {
        const T dn = d[n];
        if (P) P[n * T_ + t] = P[n * T_ + t] / dn;
        x = x * dn;
    }
    *ph = x;
    W0[n * T_ + t] = x;
}

// H(t, n) = value | H(t, n) / d_n over the N x T_ elements
template <typename T>
__global__ void k_prox_finish(T* __restrict__ H, long hs_t, long hs_n, const T* __restrict__ d, int N, int T_, int n_fast,
                              int fill, T value) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * T_) return;
    const long t = n_fast ? i / N : i % T_;
    const long n = n_fast ? i % N : i / T_;
    T* ph = H + t * hs_t + n * hs_n;
    *ph = fill ? value : *ph / d[n];
}

// one block per utterance: the maximum of its frames' shares over every row block, in an order that depends on the sizes
// only; a NaN wins and compares false, so the utterance runs on (lasso.py:293).  `applied` = i + 1 updates
__global__ __launch_bounds__(256) void k_prox_check(const double* __restrict__ partials, int n_blocks, int T_,
                                                    const int* __restrict__ offs, int* stop, double* trace, int n_slots, int slot,
                                                    int applied, int stop_rule) {
    __shared__ double red[256];
    const int u = blockIdx.x;
    const long i0 = offs[u], i1 = offs[u + 1];
    if (stop[u] != 0 || i0 == i1) return;       // uniform per block
    double m = -__builtin_inf();
    for (int rb = 0; rb < n_blocks; ++rb)
        for (long i = i0 + threadIdx.x; i < i1; i += 256) m = nanmax(m, partials[(long)rb * T_ + i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = nanmax(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    trace[(long)u * n_slots + slot] = red[0];
    if (stop_rule == EVC_STOP_DECOMP && red[0] < 0.0) stop[u] = applied;
}

unsigned prox_blocks_of(long n) { return (unsigned)((n + 255) / 256); }

// What a call of either driver does around its own part, in launch order: the state head; without iterations the constant
// start, if asked for (a given start stays as it is: nothing is scaled); with frames and iterations prepare() - the driver's
// once-per-call work, which ends with k_prox_start leaving X_0 in H and Wb[0] - then prox_loop over the driver's sweep with
// k_prox_check as its check, and the division of H by d under `normalize`; the read-back.  t: the tail of the driver's
// workspace; row_blocks: the row blocks of the sweep that writes t.partials; H(t, n) at t hs_t + n hs_n, n_fast: n is its
// contiguous direction.
template <typename T, typename Opts, typename Prepare, typename Sweep>
int prox_solve_frame(const Opts& o, const ProxTail& t, T* const Wb[2], const T* d, int row_blocks, T* H, long hs_t, long hs_n,
                     int n_fast, int N, int T_, const int* utt_offsets, int n_utt, int* n_iter_out, double* change_out,
                     hipStream_t s, Prepare prepare, Sweep sweep) {
    const int n_slots = prox_slots(o.iters, o.check_every);
    HIP_TRY(solve_state_head(utt_offsets, n_utt, T_, n_slots, t.offs, t.stop, t.trace, t.frame_utt, s));
    const unsigned nb = prox_blocks_of((long)N * T_);
    if (T_ > 0 && o.iters == 0 && o.init_mode == EVC_INIT_CONST) {
        hipLaunchKernelGGL(k_prox_finish<T>, dim3(nb), dim3(256), 0, s, H, hs_t, hs_n, (const T*)nullptr, N, T_, n_fast, 1,
                           (T)o.init_value);
        HIP_TRY(hipGetLastError());
    }
    const bool live = T_ > 0 && o.iters > 0;
    if (live) HIP_TRY(prepare());
    auto check = [&](int slot, int applied) -> int {
        hipLaunchKernelGGL(k_prox_check, dim3(n_utt), dim3(256), 0, s, (const double*)t.partials, row_blocks, T_,
                           (const int*)t.offs, t.stop, t.trace, n_slots, slot, applied, o.stop_rule);
        return (int)hipGetLastError();
    };
    HIP_TRY(prox_loop<T>(o, live, Wb, t.partials, s, sweep, check));
    if (live && o.normalize) {
        hipLaunchKernelGGL(k_prox_finish<T>, dim3(nb), dim3(256), 0, s, H, hs_t, hs_n, d, N, T_, n_fast, 0, T(0));
        HIP_TRY(hipGetLastError());
    }
    return solve_read_back(t.stop, t.trace, n_utt, n_slots, o.iters, n_iter_out, change_out, s);
}

}  // namespace

}  // namespace evc
