// evc_prox_kernels.h - the small kernels the two proximal-gradient drivers share: the per-call state,
// the start, the finish and the per-utterance check of the stop statistic, with the helpers of their arithmetic.  Two
// translation units include this file, evc_prox.hip (evc_prox_solve) and evc_prox_masked.hip (evc_prox_masked_solve), each into
// an unnamed namespace of its own: both get the same device code from the same text.  The sweeps themselves stay with their
// drivers.
#pragma once
#include "evc_prox_plan.h"

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

// stop = 0, trace = NaN, frame_utt[t] = the utterance of frame t (the largest u with offs[u] <= t)
__global__ void k_prox_state(const int* __restrict__ offs, int n_utt, int T_, int n_slots, int* stop, double* trace,
                             int* frame_utt) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_utt) stop[i] = 0;
    if (i < (long)n_utt * n_slots) trace[i] = __builtin_nan("");
    if (i < T_) {
        int lo = 0, hi = n_utt - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (offs[mid] <= i) lo = mid; else hi = mid - 1;
        }
        frame_utt[i] = lo;
    }
}

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

}  // namespace

}  // namespace evc
