// evc_prox_learn_kernels.h - the small kernels the two sparse dictionary learners share: the unit-norm
// start, the gather and scatter of a batch and the fixed-tree sum of a workgroup.  Two translation
// units include this file, evc_prox_learn.hip (evc_prox_learn) and evc_prox_masked_learn.hip (evc_prox_masked_learn), each into
// an unnamed namespace of its own: both get the same device code from the same text.  The statistics and atom kernels stay
// with their drivers.
#pragma once
#include "evc_prox_learn_plan.h"

namespace evc {

namespace {

__device__ __forceinline__ double plabs(double v) { return __builtin_fabs(v); }
__device__ __forceinline__ float plabs(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double plsqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float plsqrt(float v) { return sqrtf(v); }
// numpy's maximum: a NaN on either side wins
__device__ __forceinline__ double plmax(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// the sum of v over the workgroup's PLEARN_THREADS threads in one fixed tree: xor-shuffles inside a wavefront, then the
// wavefronts' sums in index order.  red: [PLEARN_THREADS / 64] of LDS that nobody else touches until the next barrier but one.
template <typename T>
__device__ __forceinline__ T plearn_sum(T v, T* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = red[0];
#pragma unroll
    for (int w = 1; w < PLEARN_THREADS / 64; ++w) s += red[w];
    return s;
}

// the unit-norm start: one workgroup per atom, d_n <- d_n / sqrt(sum_m d_mn^2)
template <typename T>
__global__ __launch_bounds__(PLEARN_THREADS) void k_plearn_unit(T* __restrict__ D, long ds_n, long ds_m, int M) {
    __shared__ T red[PLEARN_THREADS / 64];
    T* d = D + (long)blockIdx.x * ds_n;
    T ss = T(0);
    for (int m = threadIdx.x; m < M; m += PLEARN_THREADS) ss += d[m * ds_m] * d[m * ds_m];
    const T nrm = plsqrt(plearn_sum(ss, red));
    for (int m = threadIdx.x; m < M; m += PLEARN_THREADS) d[m * ds_m] = d[m * ds_m] / nrm;
}

// Z(t, r) = H(f_t, r) for r < N, X(f_t, r - N) else, over the bs x (N + M) elements; f_t = ord[t0 + t] (ord == NULL: t0 + t).
// r_fast: r is the contiguous direction of all three (frame-major)
template <typename T>
__global__ __launch_bounds__(256) void k_plearn_gather(const T* __restrict__ X, long xs_t, long xs_m, const T* __restrict__ H,
                                                       long hs_t, long hs_n, T* __restrict__ Z, long zs_t, long zs_r,
                                                       const int* __restrict__ ord, int t0, int bs, int N, int M, int r_fast) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int R = N + M;
    if (i >= (long)bs * R) return;
    const int t = r_fast ? (int)(i / R) : (int)(i % bs);
    const int r = r_fast ? (int)(i % R) : (int)(i / bs);
    const long f = ord ? ord[t0 + t] : t0 + t;
    Z[t * zs_t + r * zs_r] = r < N ? H[f * hs_t + r * hs_n] : X[f * xs_t + (r - N) * xs_m];
}

// H(f_t, n) = Z(t, n) over the bs x N activations of the batch
template <typename T>
__global__ __launch_bounds__(256) void k_plearn_scatter(T* __restrict__ H, long hs_t, long hs_n, const T* __restrict__ Z, long zs_t,
                                                        long zs_r, const int* __restrict__ ord, int t0, int bs, int N,
                                                        int r_fast) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)bs * N) return;
    const int t = r_fast ? (int)(i / N) : (int)(i % bs);
    const int n = r_fast ? (int)(i % N) : (int)(i / bs);
    const long f = ord ? ord[t0 + t] : t0 + t;
    H[f * hs_t + n * hs_n] = Z[t * zs_t + n * zs_r];
}

unsigned plearn_blocks_of(long n) { return (unsigned)((n + 255) / 256); }

// what both drivers hand plearn_loop (evc_prox_learn_plan.h) as stage_order: row e of the caller's order[epochs][T_] to `ord`
// (from pageable memory: HIP has copied the bytes by the time the call returns) ...
int plearn_stage_order(const int* order, int e, int T_, int* ord, hipStream_t s) {
    return (int)hipMemcpyAsync(ord, order + (size_t)e * T_, sizeof(int) * (size_t)T_, hipMemcpyHostToDevice, s);
}

// ... and the end of their read_stat: the statistic their own kernel has just left in `stat`, waited for
int plearn_fetch_stat(const double* stat, double* out, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(out, stat, sizeof(double), hipMemcpyDeviceToHost, s));
    return (int)hipStreamSynchronize(s);
}

}  // namespace

}  // namespace evc
