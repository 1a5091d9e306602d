// evc_kmeans.hip - evc_kmeans: k-means on the device (pymf kmeans.py:57-83, dist.py:54-127, base.py:238-270).  DESIGN.md §5.24.
//
// Once per call: xn[t] = ||x_t||^2 (k_km_norms).  Per assignment: wn[r] = ||w_r||^2 (k_km_norms), then
//   k_km_assign<T>   a workgroup of four wavefronts owns KM_BT = 64 samples (a wavefront 16) and one of S contiguous ranges of
//                    centre tiles.  Bins are staged in LDS in chunks of KM_KC = 64 as [bin][sample] and [bin][centre]; with
//                    M <= 64 the X tile is staged once and only the centres stream.  Per centre tile of KM_CT = 32 a wavefront
//                    issues two 16x16x4 MFMAs per k-step (A: 16 centres, B: its 16 samples), so a lane's eight accumulator
//                    values are eight centres of ONE sample: the scores ||w_r||^2 - 2 w_r^T x_t update the lane's best
//                    (score, index) and second-best score in registers, the four lane groups of a sample are merged by
//                    shuffles at the end.  S = 1: the kernel writes the label, the two scores and the flag; S > 1: the
//                    range's triple, and k_km_merge folds the ranges in ascending order and writes the same four.
//   k_km_refine<T>   one wavefront per FLAGGED sample: the direct form sum_m (x_m - w_m)^2 (bins ascending, no contraction
//                    into fused multiply-adds) against all R centres, a lane per centre, the lowest index of the least.
// Per round: k_km_centres (a workgroup per centre: the members, found in ascending sample order, are summed in that order;
// an empty cluster keeps its centre; also the counts), the assignment, k_km_err (every sample's squared distance to its
// centre in float64, and whether its label changed) and k_km_commit (one workgroup: the error summed in an order that
// depends on T only, the changed labels counted, the stop decided).  Once the loop has stopped every kernel that writes
// centres or labels returns at once.  No float atomics, no exchange between workgroups, no residency assumption.
#include "evc_kmeans_plan.h"

#include <limits.h>

namespace evc {

namespace {

constexpr int KM_LDX = KM_BT + 8;        // row strides of the two LDS images
constexpr int KM_LDW = KM_CT + 8;
constexpr int KM_CENTRE_E = (KM_MAX_M + 255) / 256;      // bins per thread of k_km_centres
static_assert(KM_BT == 64 && KM_CT == 32 && KM_KC == 64, "the staging maps below are written for 64 x 64 and 64 x 32 chunks");

template <typename T> struct KmNum;
template <> struct KmNum<double> {
    static __device__ __forceinline__ double inf() { return __builtin_inf(); }
    static __device__ __forceinline__ double unit() { return 1.1102230246251565e-16; }      // 2^-53
};
template <> struct KmNum<float> {
    static __device__ __forceinline__ float inf() { return __builtin_inff(); }
    static __device__ __forceinline__ float unit() { return 5.9604644775390625e-8f; }       // 2^-24
};

// out[c] = sum_m V(m, c)^2, bins ascending: one thread per column, so identical columns give identical norms
template <typename T>
__global__ __launch_bounds__(256) void k_km_norms(const T* __restrict__ V, long vs_m, long vs_c, int M, int C, T* __restrict__ out) {
    const long c = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    T acc = T(0);
    for (int m = 0; m < M; ++m) {
        const T v = V[m * vs_m + c * vs_c];
        acc += v * v;
    }
    out[c] = acc;
}

// the best (score, index) and the second-best score; the order is lexicographic on (score, index), so what a sequence of
// insertions and merges leaves does not depend on their order
template <typename T> struct KmTop {
    T s1, s2;
    int i1;
    __device__ __forceinline__ void clear() { s1 = s2 = KmNum<T>::inf(); i1 = INT_MAX; }
    __device__ __forceinline__ void insert(T s, int i) {
        if (s < s1 || (s == s1 && i < i1)) { s2 = s1; s1 = s; i1 = i; }
        else if (s < s2) s2 = s;
    }
    __device__ __forceinline__ void merge(T os1, int oi1, T os2) {
        insert(os1, oi1);
        if (os2 < s2) s2 = os2;
    }
};

// max_r wn[r] (NaN ignored) by the whole workgroup of 256; red: 256 elements of LDS
template <typename T>
__device__ __forceinline__ T km_block_wmax(const T* __restrict__ wn, int R, T* red) {
    T wm = T(0);
    for (int r = threadIdx.x; r < R; r += 256) {
        const T v = wn[r];
        if (v > wm) wm = v;
    }
    red[threadIdx.x] = wm;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w && red[threadIdx.x + w] > red[threadIdx.x]) red[threadIdx.x] = red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

template <typename T> struct KmOut {
    T* s1;              // [T]
    T* s2;              // [T]
    int* lab;           // [T]
    int* flag;          // [T]
    const T* xn;        // [T]
    int M, R, force;
};

// what the assignment leaves of sample t: its label, the two scores and whether the direct form has to decide again
template <typename T>
__device__ __forceinline__ void km_finish(const KmOut<T>& o, long t, const KmTop<T>& b, T wmax) {
    o.lab[t] = (b.i1 >= 0 && b.i1 < o.R) ? b.i1 : 0;
    o.s1[t] = b.s1;
    o.s2[t] = b.s2;
    const T g = T(4) * T(o.M + 4) * KmNum<T>::unit() * (o.xn[t] + wmax);
    o.flag[t] = (o.force || !(b.s2 - b.s1 >= g)) ? 1 : 0;      // NaN differences are flagged
}

template <typename T> struct KmAssignArgs {
    const T* X;         // element (m, t) at m xs_m + t xs_t
    const T* W;         // element (m, r) at m ws_m + r ws_r
    long xs_m, xs_t, ws_m, ws_r;
    const T* wn;        // [R]
    KmOut<T> out;       // S == 1
    T* ps1;             // S > 1: [S][T]
    T* ps2;
    int* pi1;
    const int* stop;
    int T_, S;
};

template <typename T>
__global__ __launch_bounds__(256) void k_km_assign(KmAssignArgs<T> a) {
    typedef typename Mma<T>::acc_t acc_t;
    __shared__ T Xs[KM_KC * KM_LDX];
    __shared__ T Ws[KM_KC * KM_LDW];
    __shared__ T red[256];
    if (*a.stop != 0) return;                 // uniform: the loop has stopped, the labels stay
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, q = lane >> 4;
    const int M = a.out.M, R = a.out.R;
    const long t0 = (long)blockIdx.x * KM_BT;
    const int NT = (R + KM_CT - 1) / KM_CT;
    const int ct_lo = (int)((long)blockIdx.y * NT / a.S), ct_hi = (int)((long)(blockIdx.y + 1) * NT / a.S);
    const int nchunks = (M + KM_KC - 1) / KM_KC;
    const bool x_tfast = a.xs_t == 1, w_rfast = a.ws_r == 1;

    // a chunk of 64 bins x 64 samples, zero outside the logical elements: 16 elements per thread, along the contiguous direction
    auto stage_x = [&](int m0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int s = x_tfast ? (tid & 63) : (tid >> 6) + 4 * e;
            const int k = x_tfast ? (tid >> 6) + 4 * e : (tid & 63);
            const long t = t0 + s;
            const int m = m0 + k;
            Xs[k * KM_LDX + s] = (m < M && t < a.T_) ? a.X[m * a.xs_m + t * a.xs_t] : T(0);
        }
    };
    // ... and of 64 bins x 32 centres: 8 per thread
    auto stage_w = [&](int c0, int m0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = w_rfast ? (tid & 31) : (tid >> 6) + 4 * e;
            const int k = w_rfast ? (tid >> 5) + 8 * e : (tid & 63);
            const int r = c0 + c;
            const int m = m0 + k;
            Ws[k * KM_LDW + c] = (m < M && r < R) ? a.W[m * a.ws_m + r * a.ws_r] : T(0);
        }
    };

    KmTop<T> best;
    best.clear();
    if (nchunks == 1 && ct_lo < ct_hi) stage_x(0);            // the loop's first barrier publishes it
#pragma unroll 1
    for (int ct = ct_lo; ct < ct_hi; ++ct) {
        acc_t acc[2];
        acc[0] = acc[1] = acc_t{0, 0, 0, 0};
#pragma unroll 1
        for (int ch = 0; ch < nchunks; ++ch) {
            const int m0 = ch * KM_KC;
            __syncthreads();                                  // the last chunk's reads are done
            if (nchunks > 1) stage_x(m0);
            stage_w(ct * KM_CT, m0);
            __syncthreads();
            const int left = M - m0;
            const int ksteps = ((left < KM_KC ? left : KM_KC) + 3) / 4;
            const T* xs = &Xs[q * KM_LDX + wave * 16 + i16];
            const T* ws = &Ws[q * KM_LDW + i16];
            for (int st = 0; st < ksteps; ++st) {
                const T x = xs[st * 4 * KM_LDX];
                const T w0 = ws[st * 4 * KM_LDW], w1 = ws[st * 4 * KM_LDW + 16];
                acc[0] = Mma<T>::mma(w0, x, acc[0]);
                acc[1] = Mma<T>::mma(w1, x, acc[1]);
            }
        }
        // rows of the accumulators are centres, the lane's column is its sample
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = ct * KM_CT + h * 16 + Mma<T>::row(lane, r);
                if (c < R) best.insert(a.wn[c] - T(2) * acc[h][r], c);
            }
    }
    // the four lane groups of a sample hold disjoint centres
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        const T os1 = __shfl_xor(best.s1, off, 64), os2 = __shfl_xor(best.s2, off, 64);
        const int oi1 = __shfl_xor(best.i1, off, 64);
        best.merge(os1, oi1, os2);
    }
    const long t = t0 + wave * 16 + i16;
    if (a.S > 1) {
        if (q == 0 && t < a.T_) {
            const long i = (long)blockIdx.y * a.T_ + t;
            a.ps1[i] = best.s1;
            a.ps2[i] = best.s2;
            a.pi1[i] = best.i1;
        }
        return;
    }
    const T wmax = km_block_wmax<T>(a.wn, R, red);
    if (q == 0 && t < a.T_) km_finish<T>(a.out, t, best, wmax);
}

// the S ranges' results, merged in ascending order
template <typename T>
__global__ __launch_bounds__(256) void k_km_merge(const T* __restrict__ ps1, const T* __restrict__ ps2, const int* __restrict__ pi1,
                                                  int S, int T_, const T* __restrict__ wn, KmOut<T> out,
                                                  const int* __restrict__ stop) {
    __shared__ T red[256];
    if (*stop != 0) return;
    const T wmax = km_block_wmax<T>(wn, out.R, red);
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T_) return;
    KmTop<T> best;
    best.clear();
    for (int z = 0; z < S; ++z) {
        const long i = (long)z * T_ + t;
        best.merge(ps1[i], pi1[i], ps2[i]);
    }
    km_finish<T>(out, t, best, wmax);
}

// the flagged samples again, by the direct form in the working type: a wavefront per sample, a lane per centre
template <typename T>
__global__ __launch_bounds__(256) void k_km_refine(const T* __restrict__ X, long xs_m, long xs_t, const T* __restrict__ W, long ws_m,
                                                   long ws_r, const int* __restrict__ flag, int* __restrict__ lab, int M, int R,
                                                   int T_, const int* __restrict__ stop) {
    if (*stop != 0) return;
    const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T_ || flag[t] == 0) return;      // uniform per wavefront
    const int lane = threadIdx.x & 63;
    T bd = KmNum<T>::inf();
    int bi = INT_MAX;
    for (int r = lane; r < R; r += 64) {
        T d = T(0);
        {
#pragma clang fp contract(off)
            for (int m = 0; m < M; ++m) {
                const T df = X[m * xs_m + t * xs_t] - W[m * ws_m + r * ws_r];
                const T sq = df * df;
                d = d + sq;
            }
        }
        if (d < bd) { bd = d; bi = r; }       // r ascends: the first of equals stays
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T od = __shfl_xor(bd, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    if (lane == 0) lab[t] = (bi >= 0 && bi < R) ? bi : 0;
}

// One workgroup per centre r: the samples are scanned 256 at a time, the members of a slice are listed in ascending order
// (ballot and prefix counts) and added in that order, thread j owning bins j, j + 256, ...  cnt[r] = the members;
// write_w: w_r = sum / members where there are any.
template <typename T>
__global__ __launch_bounds__(256) void k_km_centres(const T* __restrict__ X, long xs_m, long xs_t, T* W, long ws_m, long ws_r,
                                                    const int* __restrict__ lab, int* __restrict__ cnt, int M, int T_, int write_w,
                                                    const int* __restrict__ stop) {
    __shared__ int list[256];
    __shared__ int wtot[4];
    if (write_w && *stop != 0) return;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    T acc[KM_CENTRE_E];
#pragma unroll
    for (int e = 0; e < KM_CENTRE_E; ++e) acc[e] = T(0);
    int n = 0;
    for (long t0 = 0; t0 < T_; t0 += 256) {
        const long t = t0 + tid;
        const bool mine = t < T_ && lab[t] == r;
        const unsigned long long bal = __ballot(mine);
        if (lane == 0) wtot[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += wtot[w];
            total += wtot[w];
        }
        if (mine) list[before + __popcll(bal & ((1ull << lane) - 1ull))] = (int)(t - t0);
        __syncthreads();
        if (write_w)
            for (int j = 0; j < total; ++j) {
                const long tt = t0 + list[j];
#pragma unroll
                for (int e = 0; e < KM_CENTRE_E; ++e) {
                    const int m = tid + 256 * e;
                    if (m < M) acc[e] += X[m * xs_m + tt * xs_t];
                }
            }
        n += total;
        __syncthreads();                      // list and wtot are rewritten by the next slice
    }
    if (tid == 0) cnt[r] = n;
    if (!write_w || n == 0) return;
#pragma unroll
    for (int e = 0; e < KM_CENTRE_E; ++e) {
        const int m = tid + 256 * e;
        if (m < M) W[m * ws_m + r * ws_r] = acc[e] / T(n);
    }
}

// err2[t] = sum_m (X(m, t) - W(m, lab[t]))^2 in float64, one wavefront per sample; chg[t] = the label differs from the
// assignment before (first: 0), which it then replaces
template <typename T>
__global__ __launch_bounds__(256) void k_km_err(const T* __restrict__ X, long xs_m, long xs_t, const T* __restrict__ W, long ws_m,
                                                long ws_r, const int* __restrict__ lab, int* __restrict__ prev, int* __restrict__ chg,
                                                int M, int T_, int first, double* __restrict__ err2, const int* __restrict__ stop) {
    if (*stop != 0) return;
    const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T_) return;
    const int lane = threadIdx.x & 63;
    const int r = lab[t];
    double acc = 0.0;
    for (int m = lane; m < M; m += 64) {
        const double d = (double)X[m * xs_m + t * xs_t] - (double)W[m * ws_m + r * ws_r];
        acc += d * d;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) {
        err2[t] = acc;
        chg[t] = (!first && prev[t] != r) ? 1 : 0;
        prev[t] = r;
    }
}

// stop = 0, trace = NaN
__global__ void k_km_state(int n_slots, int* stop, double* eprev, double* trace) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { *stop = 0; *eprev = 0.0; }
    if (i < n_slots) trace[i] = __builtin_nan("");
}

// one workgroup: err = sqrt(sum of the samples' shares), summed in an order that depends on T only, and the labels that
// changed; round c (0: the first assignment).  EVC_KM_STOP_PYMF (base.py:189-206, 266-270): from the third round on,
// |err - err_prev| / T < tol stops; EVC_KM_STOP_LABELS: a round that changed no label stops
__global__ __launch_bounds__(256) void k_km_commit(const double* __restrict__ err2, const int* __restrict__ chg, int T_, int* stop,
                                                   double* eprev, double* trace, int c, int stop_rule, double tol) {
    __shared__ double red[256];
    __shared__ int redc[256];
    if (*stop != 0) return;                     // uniform
    double acc = 0.0;
    int changed = 0;
    for (int i = threadIdx.x; i < T_; i += 256) {
        acc += err2[i];
        changed += chg[i];
    }
    red[threadIdx.x] = acc;
    redc[threadIdx.x] = changed;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[threadIdx.x] += red[threadIdx.x + w];
            redc[threadIdx.x] += redc[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double err = sqrt(red[0]);
    trace[c] = err;
    if (stop_rule == EVC_KM_STOP_PYMF && c >= 3 && fabs(err - *eprev) / (double)T_ < tol) *stop = c;
    else if (stop_rule == EVC_KM_STOP_LABELS && c >= 1 && redc[0] == 0) *stop = c;
    else *eprev = err;
}

unsigned blocks_of(long n, int per) { return (unsigned)((n + per - 1) / per); }

// arguments already validated by kmeans_args_check; returns 0 or a hipError_t
template <typename T>
int kmeans_run(const T* X, int ldx, T* W, int ldw, int* labels, int* counts, int M, int R, int T_, const evc_kmeans_opts& o,
               int S, void* ws, int* n_iter_out, double* err_out, hipStream_t s) {
    const KmWs w = carve_kmeans(ws, R, T_, S, o.dtype);
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    const long xs_m = fm ? 1 : ldx, xs_t = fm ? ldx : 1, ws_m = fm ? 1 : ldw, ws_r = fm ? ldw : 1;
    const int n_slots = 1 + o.iters;
    T* xn = reinterpret_cast<T*>(w.xn);
    T* wn = reinterpret_cast<T*>(w.wn);

    hipLaunchKernelGGL(k_km_state, dim3(blocks_of(n_slots, 256)), dim3(256), 0, s, n_slots, w.stop, w.eprev, w.trace);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_km_norms<T>, dim3(blocks_of(T_, 256)), dim3(256), 0, s, X, xs_m, xs_t, M, T_, xn);
    HIP_TRY(hipGetLastError());

    KmAssignArgs<T> a;
    a.X = X; a.W = W; a.xs_m = xs_m; a.xs_t = xs_t; a.ws_m = ws_m; a.ws_r = ws_r; a.wn = wn;
    a.out.s1 = reinterpret_cast<T*>(w.s1); a.out.s2 = reinterpret_cast<T*>(w.s2); a.out.lab = w.lab; a.out.flag = w.flag;
    a.out.xn = xn; a.out.M = M; a.out.R = R; a.out.force = o.reserved & 1;
    a.ps1 = reinterpret_cast<T*>(w.ps1); a.ps2 = reinterpret_cast<T*>(w.ps2); a.pi1 = w.pi1;
    a.stop = w.stop; a.T_ = T_; a.S = S;
    // the assignment with the current centres, then the error and the stop of round c
    auto assign = [&](int c) -> int {
        hipLaunchKernelGGL(k_km_norms<T>, dim3(blocks_of(R, 256)), dim3(256), 0, s, (const T*)W, ws_m, ws_r, M, R, wn);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_km_assign<T>, dim3(blocks_of(T_, KM_BT), (unsigned)S), dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
        if (S > 1) {
            hipLaunchKernelGGL(k_km_merge<T>, dim3(blocks_of(T_, 256)), dim3(256), 0, s, (const T*)a.ps1, (const T*)a.ps2,
                               (const int*)a.pi1, S, T_, (const T*)wn, a.out, (const int*)w.stop);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_km_refine<T>, dim3(blocks_of(T_, 4)), dim3(256), 0, s, X, xs_m, xs_t, (const T*)W, ws_m, ws_r,
                           (const int*)w.flag, w.lab, M, R, T_, (const int*)w.stop);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_km_err<T>, dim3(blocks_of(T_, 4)), dim3(256), 0, s, X, xs_m, xs_t, (const T*)W, ws_m, ws_r,
                           (const int*)w.lab, w.prev, w.chg, M, T_, c == 0 ? 1 : 0, w.err2, (const int*)w.stop);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_km_commit, dim3(1), dim3(256), 0, s, (const double*)w.err2, (const int*)w.chg, T_, w.stop, w.eprev,
                           w.trace, c, o.stop_rule, o.tol);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    auto centres = [&](int write_w) -> int {
        hipLaunchKernelGGL(k_km_centres<T>, dim3((unsigned)R), dim3(256), 0, s, X, xs_m, xs_t, W, ws_m, ws_r, (const int*)w.lab,
                           w.cnt, M, T_, write_w, (const int*)w.stop);
        return (int)hipGetLastError();
    };
    HIP_TRY(assign(0));
    if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
    for (int it = 1; it <= o.iters; ++it) {
        if (o.update == EVC_KM_BOTH) HIP_TRY(centres(1));
        HIP_TRY(assign(it));
    }
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    if (counts) {
        HIP_TRY(centres(0));
        HIP_TRY(hipMemcpyAsync(counts, w.cnt, sizeof(int) * (size_t)R, hipMemcpyDeviceToDevice, s));
    }
    if (labels) HIP_TRY(hipMemcpyAsync(labels, w.lab, sizeof(int) * (size_t)T_, hipMemcpyDeviceToDevice, s));

    if (!n_iter_out && !err_out) return 0;
    int ni = 0;
    hipError_t e = hipMemcpyAsync(&ni, w.stop, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && err_out) e = hipMemcpyAsync(err_out, w.trace, sizeof(double) * n_slots, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    HIP_TRY(e);
    if (n_iter_out) *n_iter_out = ni ? ni : o.iters;
    return 0;
}

}  // namespace

}  // namespace evc

extern "C" {

size_t evc_kmeans_workspace_bytes(int M, int R, int T, int dtype) { return evc::kmeans_workspace_bytes(M, R, T, dtype); }

int evc_kmeans_splits(int R, int T) { return evc::kmeans_sizes_ok(1, R, T) ? evc::kmeans_splits(R, T) : 0; }

int evc_kmeans(const void* X, int ldx, void* W, int ldw, int* labels, int* counts, int M, int R, int T,
               const evc_kmeans_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out, double* err_out,
               evc_stream_t stream) {
    using namespace evc;
    int S = 1;
    HIP_TRY(kmeans_args_check(X, ldx, W, ldw, M, R, T, opts, workspace, workspace_bytes, &S));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (opts->dtype == EVC_F64)
        return kmeans_run<double>(static_cast<const double*>(X), ldx, static_cast<double*>(W), ldw, labels, counts, M, R, T, *opts,
                                  S, workspace, n_iter_out, err_out, s);
    return kmeans_run<float>(static_cast<const float*>(X), ldx, static_cast<float*>(W), ldw, labels, counts, M, R, T, *opts, S,
                             workspace, n_iter_out, err_out, s);
}

}  // extern "C"
