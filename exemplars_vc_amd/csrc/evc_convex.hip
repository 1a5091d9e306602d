// evc_convex.hip - evc_convex_learn: convex NMF, X ~ (X G) H with X signed and G, H >= 0 (Ding, Li and Jordan 2010; pymf
// cnmf.py:97-175).  DESIGN.md §5.21.
//
// Once per call:  K = X^T X (T x T, zero-padded to TP = round_up(T, 128) in both directions) by the bounds-checked strided
// contraction on the caller's X.  Per iteration, with pos(m) = (|m| + m) / 2 and neg(m) = (|m| - m) / 2 as written:
//     Np = pos(K) G;  Nn = neg(K) G                                                                       sweep 1
//     Sp = G^T Np;  Sn = G^T Nn;  Ha = Np + H^T Sn;  Hb = (Nn + H^T Sp) + eps;  H^T <- H^T * sqrt(Ha / Hb)
//     C = H H^T;  Wa = pos(K) H^T + Nn C;  Wb = (neg(K) H^T + Np C) + eps;  G <- G * sqrt(Wa / Wb)         sweep 2
//
// k_convex_sweep<T, W>: [pos(K) B, neg(K) B] for B = G or H^T (T x R, any strides).  This is k_semi_sweep's main loop on
// another shape: the right-hand side has R <= 1024 columns instead of thousands of frames, so blockIdx.z owns one of S
// contiguous ranges of k-slabs, and a workgroup of W = 8, 4 or 2 wavefronts owns 16 W rows x CONVEX_BR = 64 columns
// (convex_plan, evc_convex_plan.h, decides S and W from (T, R) alone: ranges first, narrower blocks where 16 ranges are not
// enough).  It streams K[k, rows] (K is symmetric: the rows of the block are read as columns of the k-slab, contiguous in
// memory) and B[k, columns] for k ascending in slabs of 16, double-buffered in LDS, one barrier per slab; a wavefront owns
// 16 rows x 64 columns: per k-step of 4 it reads one fragment of K, splits it into pos and neg in registers, reads four
// fragments of B and issues eight 16x16x4 MFMAs into 4 + 4 accumulators.  The epilogue, by mode: STORE writes Np and Nn;
// UPDATE_G reads Nn C, Np C and G and writes G (each element by the lane that read it: the sweep streams H^T, never G);
// PARTIAL writes the range's sums to slab z of the workspace, and k_convex_reduce adds the S slabs in ascending order and
// does what STORE or UPDATE_G would have done.  No float atomics, no exchange between workgroups, no residency assumption;
// with S = 1 an output's bits do not depend on W.
//
// The small products (K, H^T S, N C, W = X G, V = W H) go through gemm_strided; the three R x R products that contract over
// all of T (Sp, Sn, C) through k_convex_rr, the same tile with k split into convex_rr_splits(T, R) ranges summed in order.
// The error: k_convex_err leaves every exemplar's squared residual (float64), k_convex_check sums them in a fixed order,
// records the square root and applies pymf's stop rule on the device; once the loop has stopped, every kernel that writes
// G or H returns at once.
#include "evc_convex_plan.h"

namespace evc {

namespace {

constexpr int CVX_LDB = CONVEX_BR + 16;
constexpr int CVX_CT = CONVEX_BR / 16;       // column tiles of 16 per wavefront
static_assert(CONVEX_KS == 16 && CONVEX_BR == 64, "the staging maps below are written for slabs of 16 x 64 columns");
static_assert(CONVEX_BN == 16 * CONVEX_MAX_WAVES, "K is padded to the widest row block");

enum { CVX_STORE = 0, CVX_UPDATE_G = 1, CVX_PARTIAL = 2 };

template <typename T> struct Vec4;
template <> struct Vec4<double> { typedef f64x4 type; };
template <> struct Vec4<float> { typedef f32x4 type; };

__device__ __forceinline__ double absv(double v) { return __builtin_fabs(v); }
__device__ __forceinline__ float absv(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double sqrtv(double v) { return sqrt(v); }
__device__ __forceinline__ float sqrtv(float v) { return sqrtf(v); }

template <typename T> struct ConvexArgs {
    const T* K;             // [TP][TP]
    const T* B;             // element (k, c) at k bs_k + c bs_c: G or H^T
    long bs_k, bs_c;
    T* Op;                  // STORE: Np / Nn [T][R];  PARTIAL: slab z of which w at Op + (2 z + w) T R
    T* On;
    T* G;                   // UPDATE_G: element (t, c) at t ldg + c
    const T* NC1;           // [T][R]: Nn C
    const T* NC2;           // [T][R]: Np C
    const int* stop;
    long ldg;
    int T_, TP, R, S, mode;
    T eps;
};

// W wavefronts: the workgroup owns 16 W rows (the launch bound is the widest workgroup's for every W, as in k_semi_sweep)
template <typename T, int W>
__global__ __launch_bounds__(64 * CONVEX_MAX_WAVES) void k_convex_sweep(ConvexArgs<T> a) {
    typedef typename Mma<T>::acc_t acc_t;
    typedef typename Vec4<T>::type vec_t;
    constexpr int THREADS = 64 * W, BN = 16 * W, LDK = BN + 16;
    constexpr int BE = CONVEX_KS * CONVEX_BR / THREADS;      // elements of the B slab per thread: 2, 4 or 8
    __shared__ __attribute__((aligned(32))) T Ks[2][CONVEX_KS * LDK];
    __shared__ __attribute__((aligned(32))) T Bs[2][CONVEX_KS * CVX_LDB];
    if (*a.stop != 0) return;                 // uniform: the loop has stopped, G and H stay
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, q = lane >> 4;
    const int c0 = blockIdx.x * CONVEX_BR;
    const int n0 = blockIdx.y * BN;
    const bool k_fast = a.bs_k == 1;          // k is the contiguous direction of the source

    acc_t accp[CVX_CT], accn[CVX_CT];
#pragma unroll
    for (int j = 0; j < CVX_CT; ++j) accp[j] = accn[j] = acc_t{0, 0, 0, 0};

    // what a thread stages of a slab: one vector of four of K, BE elements of B (along k where k is contiguous)
    const int g_row = tid / (4 * W), g_col = (tid % (4 * W)) * 4;
    int b_k[BE], b_c[BE];
#pragma unroll
    for (int e = 0; e < BE; ++e) {
        if (k_fast) { b_k[e] = tid & 15; b_c[e] = (tid >> 4) + 4 * W * e; } else { b_c[e] = tid & 63; b_k[e] = (tid >> 6) + W * e; }
    }
    vec_t pk;
    T pb[BE];
    auto fetch = [&](int k0) {
        pk = *reinterpret_cast<const vec_t*>(a.K + (long)(k0 + g_row) * a.TP + n0 + g_col);      // k0 + g_row < TP: padded
#pragma unroll
        for (int e = 0; e < BE; ++e) {
            const int k = k0 + b_k[e];
            const int c = c0 + b_c[e];
            pb[e] = (k < a.T_ && c < a.R) ? a.B[(long)k * a.bs_k + (long)c * a.bs_c] : T(0);
        }
    };
    auto stage = [&](int b) {
        *reinterpret_cast<vec_t*>(&Ks[b][g_row * LDK + g_col]) = pk;
#pragma unroll
        for (int e = 0; e < BE; ++e) Bs[b][b_k[e] * CVX_LDB + b_c[e]] = pb[e];
    };

    // range z of S owns the k-slabs [z NS / S, (z + 1) NS / S): the split need not divide them, a range may be empty
    const int NS = (a.T_ + CONVEX_KS - 1) / CONVEX_KS;
    const int s_lo = (int)((long)blockIdx.z * NS / a.S), s_hi = (int)((long)(blockIdx.z + 1) * NS / a.S);
    if (s_lo < s_hi) {
        fetch(s_lo * CONVEX_KS);
        stage(0);
    }
    __syncthreads();
#pragma unroll 1
    for (int sl = s_lo; sl < s_hi; ++sl) {
        const int b = (sl - s_lo) & 1;
        if (sl + 1 < s_hi) fetch((sl + 1) * CONVEX_KS);
        const T* ks = &Ks[b][q * LDK + wave * 16 + i16];
        const T* bs = &Bs[b][q * CVX_LDB + i16];
#pragma unroll
        for (int st = 0; st < CONVEX_KS / 4; ++st) {
            const T g = ks[st * 4 * LDK];
            const T ga = absv(g);
            const T gp = (ga + g) * T(0.5), gn = (ga - g) * T(0.5);
#pragma unroll
            for (int j = 0; j < CVX_CT; ++j) {
                const T h = bs[st * 4 * CVX_LDB + j * 16];
                accp[j] = Mma<T>::mma(gp, h, accp[j]);
                accn[j] = Mma<T>::mma(gn, h, accn[j]);
            }
        }
        if (sl + 1 < s_hi) stage(b ^ 1);         // last read two barriers ago
        __syncthreads();
    }

    const long TR = (long)a.T_ * a.R;
    T* op = a.Op;
    T* on = a.On;
    if (a.mode == CVX_PARTIAL) {
        op = a.Op + 2 * (long)blockIdx.z * TR;
        on = op + TR;
    }
#pragma unroll
    for (int j = 0; j < CVX_CT; ++j) {
        const int c = c0 + j * 16 + i16;
        if (c >= a.R) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + wave * 16 + Mma<T>::row(lane, r);
            if (n >= a.T_) continue;
            const long i = (long)n * a.R + c;
            if (a.mode == CVX_UPDATE_G) {
                const T wa = accp[j][r] + a.NC1[i];
                const T wb = (accn[j][r] + a.NC2[i]) + a.eps;
                T* g = a.G + (long)n * a.ldg + c;
                *g = *g * sqrtv(wa / wb);
            } else {
                op[i] = accp[j][r];
                on[i] = accn[j][r];
            }
        }
    }
}

// the S ranges' partial sums, added in ascending order; then STORE or UPDATE_G as the sweep's own epilogue does
template <typename T>
__global__ __launch_bounds__(256) void k_convex_reduce(const T* __restrict__ part, int S, long TR, int R, int mode, T* Np, T* Nn,
                                                       T* G, long ldg, const T* __restrict__ NC1, const T* __restrict__ NC2,
                                                       T eps, const int* __restrict__ stop) {
    if (*stop != 0) return;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= TR) return;
    T p = part[i], n = part[TR + i];
    for (int z = 1; z < S; ++z) {
        p += part[2 * z * TR + i];
        n += part[(2 * z + 1) * TR + i];
    }
    if (mode == CVX_UPDATE_G) {
        const T wa = p + NC1[i];
        const T wb = (n + NC2[i]) + eps;
        T* g = G + (i / R) * ldg + i % R;
        *g = *g * sqrtv(wa / wb);
    } else {
        Np[i] = p;
        Nn[i] = n;
    }
}

// The R x R products whose contraction runs over all of T (G^T Np, G^T Nn, H H^T): C[z][i][j] = sum over the z-th of Z
// contiguous ranges of k-slabs of L[i lsi + k lsk] Rm[j rsj + k rsk].  k_gemm_strided's tile (64 x 64 outputs, four
// wavefronts, bounds-checked, any strides) with blockIdx.z owning a k-range: at R = 64 the whole product is one tile, and one
// workgroup walking T / 16 slabs took longer than both sweeps.  k_convex_rr_sum adds the Z slabs in ascending order.
template <typename T>
__global__ __launch_bounds__(256) void k_convex_rr(const T* __restrict__ L, long lsi, long lsk, const T* __restrict__ Rm, long rsj,
                                                   long rsk, T* __restrict__ C, int R, int Kd) {
    typedef typename Mma<T>::acc_t acc_t;
    __shared__ T sL[CONVEX_KS][64 + 1];
    __shared__ T sR[CONVEX_KS][64 + 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1, i16 = lane & 15, q = lane >> 4;
    const long bi = (long)blockIdx.y * 64, bj = (long)blockIdx.x * 64;
    acc_t acc[2][2];
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) acc[a][b] = acc_t{0, 0, 0, 0};
    int lrow[4], lk[4], rrow[4], rk[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (lsk == 1) { lk[e] = tid & 15; lrow[e] = (tid >> 4) + 16 * e; } else { lrow[e] = tid & 63; lk[e] = (tid >> 6) + 4 * e; }
        if (rsk == 1) { rk[e] = tid & 15; rrow[e] = (tid >> 4) + 16 * e; } else { rrow[e] = tid & 63; rk[e] = (tid >> 6) + 4 * e; }
    }
    T pl[4], pr[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long gi = bi + lrow[e], gk = k0 + lk[e];
            pl[e] = (gi < R && gk < Kd) ? L[gi * lsi + gk * lsk] : T(0);
            const long gj = bj + rrow[e], gk2 = k0 + rk[e];
            pr[e] = (gj < R && gk2 < Kd) ? Rm[gj * rsj + gk2 * rsk] : T(0);
        }
    };
    const int NS = (Kd + CONVEX_KS - 1) / CONVEX_KS;
    const int s_lo = (int)((long)blockIdx.z * NS / gridDim.z), s_hi = (int)((long)(blockIdx.z + 1) * NS / gridDim.z);
    if (s_lo < s_hi) fetch(s_lo * CONVEX_KS);
    for (int sl = s_lo; sl < s_hi; ++sl) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            sL[lk[e]][lrow[e]] = pl[e];
            sR[rk[e]][rrow[e]] = pr[e];
        }
        __syncthreads();
        if (sl + 1 < s_hi) fetch((sl + 1) * CONVEX_KS);
#pragma unroll
        for (int st = 0; st < CONVEX_KS / 4; ++st) {
            const int kk = 4 * st + q;
            T a[2], b[2];
            for (int mi = 0; mi < 2; ++mi) a[mi] = sL[kk][wm * 32 + 16 * mi + i16];
            for (int ni = 0; ni < 2; ++ni) b[ni] = sR[kk][wn * 32 + 16 * ni + i16];
            for (int mi = 0; mi < 2; ++mi)
                for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = Mma<T>::mma(a[mi], b[ni], acc[mi][ni]);
        }
        __syncthreads();
    }
    T* out = C + (long)blockIdx.z * R * R;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long row = bi + wm * 32 + 16 * mi + Mma<T>::row(lane, r);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                const long col = bj + wn * 32 + 16 * ni + i16;
                if (row < R && col < R) out[row * R + col] = acc[mi][ni][r];
            }
        }
}

template <typename T>
__global__ __launch_bounds__(256) void k_convex_rr_sum(const T* __restrict__ part, int Z, int RR, T* __restrict__ C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= RR) return;
    T v = part[i];
    for (int z = 1; z < Z; ++z) v += part[(long)z * RR + i];
    C[i] = v;
}

// H(t, r) <- H(t, r) * sqrt((Np + Q1) / ((Nn + Q2) + eps)) over the T x R elements; H(t, r) at t hs_t + r hs_r
template <typename T>
__global__ __launch_bounds__(256) void k_convex_h(T* H, long hs_t, long hs_r, const T* __restrict__ Np, const T* __restrict__ Nn,
                                                  const T* __restrict__ Q1, const T* __restrict__ Q2, int T_, int R, int t_fast,
                                                  T eps, const int* __restrict__ stop) {
    if (*stop != 0) return;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)T_ * R) return;
    const long t = t_fast ? i % T_ : i / R;
    const long r = t_fast ? i / T_ : i % R;
    const long j = t * R + r;
    const T ha = Np[j] + Q1[j];
    const T hb = (Nn[j] + Q2[j]) + eps;
    T* h = H + t * hs_t + r * hs_r;
    *h = *h * sqrtv(ha / hb);
}

// stop = 0, trace = NaN
__global__ void k_convex_state(int n_slots, int* stop, double* eprev, double* trace) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { *stop = 0; *eprev = 0.0; }
    if (i < n_slots) trace[i] = __builtin_nan("");
}

// err2[t] = sum_m (X(m, t) - V[t][m])^2 in float64; one wavefront per exemplar, shuffle reduction
template <typename T>
__global__ __launch_bounds__(256) void k_convex_err(const T* __restrict__ X, long xs_t, long xs_m, const T* __restrict__ V, int M,
                                                    int T_, double* __restrict__ err2) {
    const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T_) return;
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int m = lane; m < M; m += 64) {
        const double d = (double)X[t * xs_t + m * xs_m] - (double)V[t * M + m];
        acc += d * d;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) err2[t] = acc;
}

// one block: err = sqrt(sum of the exemplars' shares), summed in an order that depends on T only; check c (0: the start).
// pymf base.py:189-206, cnmf.py:172-175: from the third update on, |ferr[i] - ferr[i-1]| / T < tol stops; a NaN error
// compares false and the loop runs on
__global__ __launch_bounds__(256) void k_convex_check(const double* __restrict__ err2, int T_, int* stop, double* eprev,
                                                      double* trace, int c, int check_every, double tol) {
    __shared__ double red[256];
    if (*stop != 0) return;                     // uniform
    double acc = 0.0;
    for (int i = threadIdx.x; i < T_; i += 256) acc += err2[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double err = sqrt(red[0]);
    trace[c] = err;
    if (c >= 3 && fabs(err - *eprev) / (double)T_ < tol)
        *stop = c * check_every;
    else
        *eprev = err;
}

unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

template <typename T>
int convex_sweep(ConvexArgs<T> a, const ConvexPlan& pl, int mode, T* part, T* Np, T* Nn, hipStream_t s) {
    a.S = pl.S;
    a.mode = pl.S > 1 ? (int)CVX_PARTIAL : mode;
    a.Op = pl.S > 1 ? part : Np;
    a.On = pl.S > 1 ? part : Nn;
    const dim3 grid((unsigned)((a.R + CONVEX_BR - 1) / CONVEX_BR), (unsigned)(a.TP / (16 * pl.W)), (unsigned)pl.S);
    if (pl.W == 8) hipLaunchKernelGGL((k_convex_sweep<T, 8>), grid, dim3(512), 0, s, a);
    else if (pl.W == 4) hipLaunchKernelGGL((k_convex_sweep<T, 4>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_convex_sweep<T, 2>), grid, dim3(128), 0, s, a);
    HIP_TRY(hipGetLastError());
    if (pl.S > 1) {
        const long TR = (long)a.T_ * a.R;
        hipLaunchKernelGGL(k_convex_reduce<T>, dim3(blocks_of(TR)), dim3(256), 0, s, (const T*)part, pl.S, TR, a.R, mode, Np, Nn,
                           a.G, a.ldg, a.NC1, a.NC2, a.eps, a.stop);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// C (R x R, packed) = sum_k L[i lsi + k lsk] Rm[j rsj + k rsk] over k < T_, in Z k-ranges added in ascending order
template <typename T>
int convex_rr(const T* L, long lsi, long lsk, const T* Rm, long rsj, long rsk, T* C, int R, int T_, int Z, T* part,
              hipStream_t s) {
    if (Z <= 1) return (int)gemm_strided<T>(L, lsi, lsk, Rm, rsj, rsk, C, R, 1, R, R, T_, s);
    const unsigned tiles = (unsigned)((R + 63) / 64);
    hipLaunchKernelGGL(k_convex_rr<T>, dim3(tiles, tiles, (unsigned)Z), dim3(256), 0, s, L, lsi, lsk, Rm, rsj, rsk, part, R, T_);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_convex_rr_sum<T>, dim3(blocks_of((long)R * R)), dim3(256), 0, s, (const T*)part, Z, R * R, C);
    return (int)hipGetLastError();
}

// arguments already validated by convex_args_check; returns 0 or a hipError_t
template <typename T>
int convex_learn(const T* X, int ldx, T* G, int ldg, T* H, int ldh, T* Wout, int ldw, int M, int R, int T_,
                 const evc_convex_opts& o, const ConvexPlan& pl, void* ws, int* n_iter_out, double* err_out, hipStream_t s) {
    const ConvexWs w = carve_convex(ws, M, R, T_, pl.S, o.dtype);
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    const int n_slots = n_slots_for(o.iters, o.check_every);
    const int TP = round_up(T_, CONVEX_BN);
    const long xs_t = fm ? ldx : 1, xs_m = fm ? 1 : ldx, hs_t = fm ? ldh : 1, hs_r = fm ? 1 : ldh;
    T* K = reinterpret_cast<T*>(w.K);
    T* Np = reinterpret_cast<T*>(w.Np);
    T* Nn = reinterpret_cast<T*>(w.Nn);
    T* Q1 = reinterpret_cast<T*>(w.Q1);
    T* Q2 = reinterpret_cast<T*>(w.Q2);
    T* part = reinterpret_cast<T*>(w.part);
    T* rrpart = reinterpret_cast<T*>(w.rrpart);
    const int Z = convex_rr_splits(T_, R);
    T* Sp = reinterpret_cast<T*>(w.Sp);
    T* Sn = reinterpret_cast<T*>(w.Sn);
    T* Wm = reinterpret_cast<T*>(w.Wm);
    T* V = reinterpret_cast<T*>(w.V);

    hipLaunchKernelGGL(k_convex_state, dim3(blocks_of(n_slots)), dim3(256), 0, s, n_slots, w.stop, w.eprev, w.trace);
    HIP_TRY(hipGetLastError());
    const bool upd_h = o.update != EVC_CONVEX_G_ONLY, upd_g = o.update != EVC_CONVEX_H_ONLY;
    if (o.iters > 0) {
        HIP_TRY(hipMemsetAsync(K, 0, (size_t)TP * TP * sizeof(T), s));
        HIP_TRY(gemm_strided<T>(X, xs_t, xs_m, X, xs_t, xs_m, K, TP, 1, T_, T_, M, s));
    }

    const bool checks = o.check_every > 0;
    auto check = [&](int c) -> int {
        HIP_TRY(gemm_strided<T>(X, xs_m, xs_t, G, 1, ldg, Wm, R, 1, M, R, T_, s));          // W = X G
        HIP_TRY(gemm_strided<T>(H, hs_t, hs_r, Wm, R, 1, V, M, 1, T_, M, R, s));            // V^T = H^T W^T
        hipLaunchKernelGGL(k_convex_err<T>, dim3((T_ + 3) / 4), dim3(256), 0, s, X, xs_t, xs_m, (const T*)V, M, T_, w.err2);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_convex_check, dim3(1), dim3(256), 0, s, (const double*)w.err2, T_, w.stop, w.eprev, w.trace, c,
                           o.check_every, o.tol);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    if (checks) HIP_TRY(check(0));
    if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
    ConvexArgs<T> a;
    a.K = K; a.G = G; a.ldg = ldg; a.NC1 = Q1; a.NC2 = Q2; a.stop = w.stop;
    a.T_ = T_; a.TP = TP; a.R = R; a.eps = (T)o.eps;
    const unsigned nb = blocks_of((long)T_ * R);
    for (int it = 1; it <= o.iters; ++it) {
        if (it == 1 || upd_g) {                 // G is fixed otherwise, and so are Np, Nn, Sp and Sn
            a.B = G; a.bs_k = ldg; a.bs_c = 1;
            HIP_TRY(convex_sweep<T>(a, pl, CVX_STORE, part, Np, Nn, s));
            if (upd_h) {
                HIP_TRY(convex_rr<T>(G, 1, ldg, Np, 1, R, Sp, R, T_, Z, rrpart, s));        // Sp = G^T Np
                HIP_TRY(convex_rr<T>(G, 1, ldg, Nn, 1, R, Sn, R, T_, Z, rrpart, s));        // Sn = G^T Nn
            }
        }
        if (upd_h) {
            HIP_TRY(gemm_strided<T>(H, hs_t, hs_r, Sn, 1, R, Q1, R, 1, T_, R, R, s));       // Q1 = H^T Sn
            HIP_TRY(gemm_strided<T>(H, hs_t, hs_r, Sp, 1, R, Q2, R, 1, T_, R, R, s));       // Q2 = H^T Sp
            hipLaunchKernelGGL(k_convex_h<T>, dim3(nb), dim3(256), 0, s, H, hs_t, hs_r, (const T*)Np, (const T*)Nn, (const T*)Q1,
                               (const T*)Q2, T_, R, fm ? 0 : 1, (T)o.eps, (const int*)w.stop);
            HIP_TRY(hipGetLastError());
        }
        if (upd_g) {
            T* Cm = Sp;                         // C = H H^T takes the place of Sp: this iteration is done with it
            HIP_TRY(convex_rr<T>(H, hs_r, hs_t, H, hs_r, hs_t, Cm, R, T_, Z, rrpart, s));
            HIP_TRY(gemm_strided<T>(Nn, R, 1, Cm, 1, R, Q1, R, 1, T_, R, R, s));            // Nn C
            HIP_TRY(gemm_strided<T>(Np, R, 1, Cm, 1, R, Q2, R, 1, T_, R, R, s));            // Np C
            a.B = H; a.bs_k = hs_t; a.bs_c = hs_r;
            HIP_TRY(convex_sweep<T>(a, pl, CVX_UPDATE_G, part, Np, Nn, s));
        }
        if (checks && it % o.check_every == 0) HIP_TRY(check(it / o.check_every));
    }
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    if (Wout) HIP_TRY(gemm_strided<T>(X, xs_m, xs_t, G, 1, ldg, Wout, fm ? 1 : ldw, fm ? ldw : 1, M, R, T_, s));

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

size_t evc_convex_workspace_bytes(int M, int R, int T, int dtype) { return evc::convex_workspace_bytes(M, R, T, dtype); }

int evc_convex_splits(int R, int T) { return evc::convex_sizes_ok(1, R, T) ? evc::convex_plan(T, R).S : 0; }

int evc_convex_learn(const void* X, int ldx, void* G, int ldg, void* H, int ldh, void* W, int ldw, int M, int R, int T,
                     const evc_convex_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out, double* err_out,
                     evc_stream_t stream) {
    using namespace evc;
    ConvexPlan pl{0, 0};
    HIP_TRY(convex_args_check(X, ldx, G, ldg, H, ldh, W, ldw, M, R, T, opts, workspace, workspace_bytes, &pl));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (opts->dtype == EVC_F64)
        return convex_learn<double>(static_cast<const double*>(X), ldx, static_cast<double*>(G), ldg, static_cast<double*>(H), ldh,
                                    static_cast<double*>(W), ldw, M, R, T, *opts, pl, workspace, n_iter_out, err_out, s);
    return convex_learn<float>(static_cast<const float*>(X), ldx, static_cast<float*>(G), ldg, static_cast<float*>(H), ldh,
                               static_cast<float*>(W), ldw, M, R, T, *opts, pl, workspace, n_iter_out, err_out, s);
}

}  // extern "C"
