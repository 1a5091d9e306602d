// evc_prox_masked.hip - evc_prox_masked_solve: evc_prox_solve's proximal-gradient solves with a weight per bin of every
// frame (deComP's 2-D `mask`, lasso.py:120-189, 259-271, 306-328, 418-445) on a factored sweep that never forms A^T A.
// DESIGN.md §5.18.
//
// Once per call:  k_pm_norm leaves d, lambda_n = alpha / d_n and tol_n; k_pm_images the scaled dictionary in both
// orientations (Dn exemplar-major, Dm bin-major, zero-padded: evc_prox_masked_plan.h); k_pm_frames cnt_t and mask . X;
// k_pm_wbar the per-bin weights of every utterance's bound (mean or maximum over its frames: 256 strided partial results
// and one tree, an order fixed by the frame's position inside its utterance); k_pm_bound the Gershgorin column sums of
// Dm^T diag(wbar_u) Dm in panels of 16 rows that live in registers (k ascending, m ascending: nothing N x N is stored);
// k_pm_lip their maximum in one block's fixed tree and s_u = 1 / L_u; P = Dm^T (mask . X) by the bounds-checked strided
// contraction; k_prox_start scales the start and copies it to W_0 (it, the state, the finish and k_prox_check are
// evc_prox_solve's, evc_prox_kernels.h).  Without a mask the bound is computed once for all utterances.
// Per iteration i, two launches:
//     k_prox_resid   R[m, t] = mask[t, m] sum_n Dn[n, m] W[n, t]                 (contraction over N, R is M x T)
//     k_prox_back    acc[n, t] = sum_m Dm[m, n] R[m, t]                          (contraction over M), then k_prox_sweep's
//                    epilogue with thr = s_u (lambda_n cnt_t):  V = W + s_u (P - acc);  X_new = threshold(V, thr);
//                    W' = X_new + c_i (X_new - X_old);  the per-frame share of the statistic on check iterations
// Both run pm_slab_mma, k_prox_sweep's slab loop (evc_prox.hip) restated as a function: 16-deep k-slabs double-buffered in
// LDS, 16x16x4 MFMAs, one accumulator per output, k ascending over the whole contraction.  k_prox_sweep itself keeps its own
// copy of the loop: its bits and its speed are pinned by the existing tests and the benchmark, and it is left as it is.
// A wavefront whose 16 rows lie wholly beyond the last row (M = 25 in a 64-row block) stages its share of the slabs and
// issues no MFMA; a workgroup none of whose frames is live returns at once, in both kernels.
// A column of the accumulators only ever sees its own column of W, R, mask and X: a batch gives bitwise the per-utterance
// results and a NaN stays in its frame's column.
#include "evc_prox_kernels.h"
#include "evc_prox_masked_plan.h"

namespace evc {

namespace {

constexpr int PM_LDH = PROX_BT + 16;
constexpr int PM_FT = PROX_BT / 16;          // frame tiles of 16 per wavefront
static_assert(PROX_KS == 16 && PROX_BT == 64, "the staging maps below are written for slabs of 16 x 64 frames");
static_assert(PROX_BN == 16 * PROX_MAX_WAVES, "the images are padded to the widest row block");

// acc[j][r] += sum_k D[k, col0 + row] B[k, t0 + frame] for k = 0 .. K - 1 ascending, the workgroup's 16 W rows x 64 frames.
// D is a padded image with ldd elements per row: rows exist up to round_up(K, 16) and columns up to col0 + 16 W, so its
// loads are unchecked; B is [K][T_], checked.  Ds: [2][PROX_KS * (16 W + 16)], Bs: [2][PROX_KS * PM_LDH] in LDS.  `active`
// is uniform per wavefront: an idle wavefront stages and meets the barriers but issues no MFMA.  Ends with a barrier.
template <typename T, int W>
__device__ __forceinline__ void pm_slab_mma(const T* __restrict__ D, int ldd, int col0, const T* __restrict__ B, int K, int T_,
                                            long t0, bool active, typename Mma<T>::acc_t (&acc)[PM_FT], T* Ds, T* Bs) {
    typedef typename PVec4<T>::type vec_t;
    constexpr int THREADS = 64 * W, LDG = 16 * W + 16;
    constexpr int HE = PROX_KS * PROX_BT / THREADS;      // elements of the B slab per thread: 2 or 4
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, q = lane >> 4;
    const int g_row = tid / (4 * W), g_col = (tid % (4 * W)) * 4;
    const int h_t = tid & 63, h_k0 = tid >> 6;
    vec_t pg;
    T ph[HE];
    auto fetch = [&](int k0) {
        pg = *reinterpret_cast<const vec_t*>(D + (long)(k0 + g_row) * ldd + col0 + g_col);
#pragma unroll
        for (int e = 0; e < HE; ++e) {
            const int k = k0 + h_k0 + W * e;
            const long t = t0 + h_t;
            ph[e] = (k < K && t < T_) ? B[(long)k * T_ + t] : T(0);
        }
    };
    auto stage = [&](int b) {
        *reinterpret_cast<vec_t*>(&Ds[b * PROX_KS * LDG + g_row * LDG + g_col]) = pg;
#pragma unroll
        for (int e = 0; e < HE; ++e) Bs[b * PROX_KS * PM_LDH + (h_k0 + W * e) * PM_LDH + h_t] = ph[e];
    };
    const int NS = (K + PROX_KS - 1) / PROX_KS;
    fetch(0);
    stage(0);
    __syncthreads();
#pragma unroll 1
    for (int sl = 0; sl < NS; ++sl) {
        const int b = sl & 1;
        if (sl + 1 < NS) fetch((sl + 1) * PROX_KS);
        if (active) {
            const T* gs = &Ds[b * PROX_KS * LDG + q * LDG + wave * 16 + i16];
            const T* hs = &Bs[b * PROX_KS * PM_LDH + q * PM_LDH + i16];
#pragma unroll
            for (int st = 0; st < PROX_KS / 4; ++st) {
                const T g = gs[st * 4 * LDG];
#pragma unroll
                for (int j = 0; j < PM_FT; ++j) acc[j] = Mma<T>::mma(g, hs[st * 4 * PM_LDH + j * 16], acc[j]);
            }
        }
        if (sl + 1 < NS) stage(b ^ 1);         // last read two barriers ago
        __syncthreads();
    }
}

// is any frame of the workgroup's block live?  uniform; two barriers
__device__ __forceinline__ bool pm_block_live(long t0, int T_, const int* frame_utt, const int* stop, int* live) {
    const int tid = threadIdx.x;
    if (tid == 0) *live = 0;
    __syncthreads();
    if (tid < PROX_BT && t0 + tid < T_ && stop[frame_utt[t0 + tid]] == 0) atomicOr(live, 1);
    __syncthreads();
    return *live != 0;
}

template <typename T> struct PmResidArgs {
    const T* Dn;            // [pm_nk(N)][MP]
    const T* Win;           // [N][T_]
    T* R;                   // [M][T_]
    const T* mask;          // element (t, m) at t ms_t + m ms_m, or NULL: every weight is 1
    long ms_t, ms_m;
    const int* frame_utt;
    const int* stop;
    int M, MP, N, T_;
};

// W wavefronts: the workgroup owns 16 W bins x 64 frames of R
template <typename T, int W>
__global__ __launch_bounds__(64 * PROX_MAX_WAVES) void k_prox_resid(PmResidArgs<T> a) {
    typedef typename Mma<T>::acc_t acc_t;
    constexpr int BN = 16 * W, LDG = BN + 16;
    __shared__ __attribute__((aligned(32))) T Ds[2 * PROX_KS * LDG];
    __shared__ __attribute__((aligned(32))) T Bs[2 * PROX_KS * PM_LDH];
    __shared__ int live;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i16 = lane & 15;
    const long t0 = (long)blockIdx.x * PROX_BT;
    const int m0 = blockIdx.y * BN;           // m0 < M: the grid has ceil(M / BN) row blocks, and m0 + BN <= MP
    if (!pm_block_live(t0, a.T_, a.frame_utt, a.stop, &live)) return;

    acc_t acc[PM_FT];
#pragma unroll
    for (int j = 0; j < PM_FT; ++j) acc[j] = acc_t{0, 0, 0, 0};
    const bool active = m0 + wave * 16 < a.M;  // uniform per wavefront
    pm_slab_mma<T, W>(a.Dn, a.MP, m0, a.Win, a.N, a.T_, t0, active, acc, Ds, Bs);
    if (!active) return;
#pragma unroll
    for (int j = 0; j < PM_FT; ++j) {
        const long t = t0 + j * 16 + i16;
        if (t >= a.T_ || a.stop[a.frame_utt[t]] != 0) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + wave * 16 + Mma<T>::row(lane, r);
            if (m >= a.M) continue;
            a.R[(long)m * a.T_ + t] = a.mask ? a.mask[t * a.ms_t + m * a.ms_m] * acc[j][r] : acc[j][r];
        }
    }
}

template <typename T> struct PmBackArgs {
    const T* Dm;            // [pm_mk(M)][NP]
    const T* R;             // [M][T_]
    const T* P;             // [N][T_]
    const T* Win;           // [N][T_]
    T* Wout;                // [N][T_]
    T* X;                   // element (t, n) at t xs_t + n xs_n: X_old on entry, X_new on return
    long xs_t, xs_n;
    const T* lam;           // [N]
    const T* cf;            // [T_]: cnt_t | 1
    const T* tolv;          // [N]
    const T* s;             // [n_utt]: 1 / L_u
    double* partials;       // [row blocks][T_] on a check iteration, else NULL
    const int* frame_utt;
    const int* stop;
    int M, N, NP, T_;
    int signed_mode;
    T c;                    // the momentum coefficient of this iteration
};

// W wavefronts: the workgroup owns 16 W exemplar rows x 64 frames; the epilogue is k_prox_sweep's with the threshold and the
// step of the frame's own utterance
template <typename T, int W>
__global__ __launch_bounds__(64 * PROX_MAX_WAVES) void k_prox_back(PmBackArgs<T> a) {
    typedef typename Mma<T>::acc_t acc_t;
    constexpr int BN = 16 * W, LDG = BN + 16;
    __shared__ __attribute__((aligned(32))) T Ds[2 * PROX_KS * LDG];
    __shared__ __attribute__((aligned(32))) T Bs[2 * PROX_KS * PM_LDH];
    __shared__ int live;
    static_assert(sizeof(T) * PROX_KS * LDG >= sizeof(double) * W * PROX_BT, "the epilogue's reduction reuses Ds");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, q = lane >> 4;
    const long t0 = (long)blockIdx.x * PROX_BT;
    const int n0 = blockIdx.y * BN;           // n0 < N: the grid has ceil(N / BN) row blocks, and n0 + BN <= NP
    if (!pm_block_live(t0, a.T_, a.frame_utt, a.stop, &live)) return;

    acc_t acc[PM_FT];
#pragma unroll
    for (int j = 0; j < PM_FT; ++j) acc[j] = acc_t{0, 0, 0, 0};
    const bool active = n0 + wave * 16 < a.N;  // uniform per wavefront
    pm_slab_mma<T, W>(a.Dm, a.NP, n0, a.R, a.M, a.T_, t0, active, acc, Ds, Bs);

    const bool check = a.partials != nullptr;  // uniform
    double* red = reinterpret_cast<double*>(Ds);              // [W][PROX_BT]: every read of Ds lies before the last barrier
#pragma unroll
    for (int j = 0; j < PM_FT; ++j) {
        const long t = t0 + j * 16 + i16;
        double worst = -__builtin_inf();
        if (active && t < a.T_ && a.stop[a.frame_utt[t]] == 0) {
            const T s = a.s[a.frame_utt[t]];
            const T cf = a.cf[t];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wave * 16 + Mma<T>::row(lane, r);
                if (n >= a.N) continue;
                const long at = (long)n * a.T_ + t;
                T* px = a.X + t * a.xs_t + n * a.xs_n;
                const T xo = *px;
                const T v = a.Win[at] + s * (a.P[at] - acc[j][r]);
                const T thr = s * (a.lam[n] * cf);
                T xn;
                if (a.signed_mode) {
                    const T m = pabs(v) - thr;
                    const T sg = v > T(0) ? T(1) : (v < T(0) ? T(-1) : (v != v ? v : T(0)));
                    xn = (!(m <= T(0)) ? m : T(0)) * sg;
                } else {
                    const T m = v - thr;
                    xn = !(m <= T(0)) ? m : T(0);
                }
                *px = xn;
                a.Wout[at] = a.c == T(0) ? xn : xn + a.c * (xn - xo);
                if (check) worst = nanmax(worst, (double)(pabs(xn - xo) - a.tolv[n]));
            }
        }
        if (check) {                           // the lanes i16, i16 + 16, + 32, + 48 hold the same frame
            worst = nanmax(worst, __shfl_xor(worst, 16, 64));
            worst = nanmax(worst, __shfl_xor(worst, 32, 64));
            if (q == 0) red[wave * PROX_BT + j * 16 + i16] = worst;
        }
    }
    if (!check) return;                        // uniform
    __syncthreads();
    if (tid < PROX_BT && t0 + tid < a.T_) {
        double worst = red[tid];
#pragma unroll
        for (int w = 1; w < W; ++w) worst = nanmax(worst, red[w * PROX_BT + tid]);
        a.partials[(long)blockIdx.y * a.T_ + t0 + tid] = worst;      // -inf for a stopped frame: never read
    }
}

// one thread per exemplar: d_n = sqrt(sum_m A_mn^2), m ascending | 1;  lambda_n = alpha / d_n | alpha;  tol_n = tol d_n | tol
template <typename T>
__global__ void k_pm_norm(const T* __restrict__ A, long as_n, long as_m, int M, int N, int normalize, T alpha, T tol,
                          T* __restrict__ d, T* __restrict__ lam, T* __restrict__ tolv) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    T dn = T(1);
    if (normalize) {
        T sum = T(0);
        for (int m = 0; m < M; ++m) {
            const T v = A[n * as_n + m * as_m];
            sum += v * v;
        }
        dn = psqrt(sum);
    }
    d[n] = dn;
    lam[n] = normalize ? alpha / dn : alpha;
    tolv[n] = normalize ? tol * dn : tol;
}

// over the N x M elements: Dn[n][m] = Dm[m][n] = A_mn / d_n (normalize == 0: A_mn); the padding was zeroed before
template <typename T>
__global__ void k_pm_images(const T* __restrict__ A, long as_n, long as_m, int M, int N, int n_fast, int normalize,
                            const T* __restrict__ d, T* __restrict__ Dn, int MP, T* __restrict__ Dm, int NP) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * M) return;
    const long n = n_fast ? i % N : i / M;
    const long m = n_fast ? i / N : i % M;
    T v = A[n * as_n + m * as_m];
    if (normalize) v = v / d[n];
    Dn[n * MP + m] = v;
    Dm[m * NP + n] = v;
}

// one thread per frame: cnt_t = sum_m mask_tm, m ascending (M without a mask) - cf_t = cnt_t | 1 - and Xm[m][t] = mask_tm X_tm
template <typename T>
__global__ void k_pm_frames(const T* __restrict__ X, long xs_t, long xs_m, const T* __restrict__ mask, long ms_t, long ms_m,
                            int M, int T_, int normalize, T* __restrict__ cf, T* __restrict__ Xm) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T_) return;
    T cnt = mask ? T(0) : (T)M;
    for (int m = 0; m < M; ++m) {
        const T x = X[t * xs_t + m * xs_m];
        if (mask) {
            const T w = mask[t * ms_t + m * ms_m];
            cnt += w;
            Xm[(long)m * T_ + t] = x * w;
        } else {
            Xm[(long)m * T_ + t] = x;
        }
    }
    cf[t] = normalize ? cnt : T(1);
}

// one block per (utterance, bin): wbar_um = the mean | the maximum (a NaN wins) of mask_tm over the utterance's frames: thread
// i takes the frames i, i + 256, ... of the utterance in order, then one tree.  Without a mask: one row of ones.
template <typename T>
__global__ __launch_bounds__(256) void k_pm_wbar(const T* __restrict__ mask, long ms_t, long ms_m, int M,
                                                 const int* __restrict__ offs, int use_max, T* __restrict__ wbar) {
    __shared__ T red[256];
    const int u = blockIdx.x, m = blockIdx.y;
    if (!mask) {
        if (threadIdx.x == 0) wbar[(long)u * M + m] = T(1);
        return;
    }
    const long i0 = offs[u], i1 = offs[u + 1];
    T v = use_max ? -(T)__builtin_inf() : T(0);
    for (long i = i0 + threadIdx.x; i < i1; i += 256) {
        const T w = mask[i * ms_t + m * ms_m];
        v = use_max ? (T)nanmax((double)v, (double)w) : v + w;
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            const T a = red[threadIdx.x], b = red[threadIdx.x + w];
            red[threadIdx.x] = use_max ? (T)nanmax((double)a, (double)b) : a + b;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) wbar[(long)u * M + m] = use_max ? red[0] : red[0] / (T)(i1 - i0);
}

// The Gershgorin column sums of G_u = Dm^T diag(wbar_u) Dm without storing G_u: a block owns 128 columns n (one per thread)
// of utterance u and walks the rows k in panels of 16; a panel's 16 entries of column n live in registers and are summed over
// m ascending, the weighted panel rows pass through LDS in chunks of 64 bins; colsum_n = sum_k |G_kn| for k ascending.
constexpr int PM_BOUND_COLS = 128, PM_BOUND_BINS = 64;
static_assert(PROX_BN % PM_BOUND_COLS == 0, "a block's columns lie inside the padded image");
template <typename T>
__global__ __launch_bounds__(PM_BOUND_COLS) void k_pm_bound(const T* __restrict__ Dm, int NP, int M, int N,
                                                            const T* __restrict__ wbar, T* __restrict__ colsum) {
    __shared__ T tile[PM_BOUND_BINS * PROX_KS];
    const int u = blockIdx.x;
    const int n = blockIdx.y * PM_BOUND_COLS + threadIdx.x;       // n < NP
    const T* wb = wbar + (long)u * M;
    T sum = T(0);
    for (int k0 = 0; k0 < N; k0 += PROX_KS) {                     // k0 + 15 < round_up(N, 16) <= NP: zero in the padding
        T acc[PROX_KS];
#pragma unroll
        for (int kk = 0; kk < PROX_KS; ++kk) acc[kk] = T(0);
        for (int m0 = 0; m0 < M; m0 += PM_BOUND_BINS) {
            __syncthreads();
            for (int e = threadIdx.x; e < PM_BOUND_BINS * PROX_KS; e += PM_BOUND_COLS) {
                const int m = m0 + (e >> 4);
                tile[e] = m < M ? Dm[(long)m * NP + k0 + (e & 15)] * wb[m] : T(0);
            }
            __syncthreads();
            const int mend = M - m0 < PM_BOUND_BINS ? M - m0 : PM_BOUND_BINS;
            for (int mm = 0; mm < mend; ++mm) {
                const T a = Dm[(long)(m0 + mm) * NP + n];
#pragma unroll
                for (int kk = 0; kk < PROX_KS; ++kk) acc[kk] += tile[mm * PROX_KS + kk] * a;
            }
        }
#pragma unroll
        for (int kk = 0; kk < PROX_KS; ++kk) sum += pabs(acc[kk]);      // a padded row adds |0|
    }
    if (n < N) colsum[(long)u * N + n] = sum;
}

// one block per utterance: L_u = max_n colsum_n of its row (row 0 without a mask) in a fixed order (a NaN wins, as numpy's
// max), s_u = 1 / L_u or 1 / lipschitz
template <typename T>
__global__ __launch_bounds__(256) void k_pm_lip(const T* __restrict__ colsum, int N, int own_row, T lipschitz, T* __restrict__ s) {
    __shared__ double red[256];
    const int u = blockIdx.x;
    if (lipschitz > T(0)) {                    // uniform
        if (threadIdx.x == 0) s[u] = T(1) / lipschitz;
        return;
    }
    const T* row = colsum + (own_row ? (long)u * N : 0);
    double m = -__builtin_inf();
    for (int n = threadIdx.x; n < N; n += 256) m = nanmax(m, (double)row[n]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = nanmax(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) s[u] = T(1) / (T)red[0];
}

// arguments already validated by prox_masked_args_check; returns 0, -2 or a hipError_t
template <typename T>
int prox_masked_solve(const T* A, int lda, const T* X, int ldx, const T* mask, int ldm, T* H, int ldh, int M, int N, int T_,
                      const int* utt_offsets, int n_utt, const evc_prox_masked_opts& o, void* ws, size_t ws_bytes,
                      int* n_iter_out, double* change_out, hipStream_t s) {
    const ProxMaskedWs w = carve_prox_masked(ws, M, N, T_, n_utt, o.dtype);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    const int NK = pm_nk(N), MP = pm_mp(M), MK = pm_mk(M), NP = pm_np(N);
    const long as_n = fm ? lda : 1, as_m = fm ? 1 : lda, xs_t = fm ? ldx : 1, xs_m = fm ? 1 : ldx;
    const long ms_t = fm ? ldm : 1, ms_m = fm ? 1 : ldm, hs_t = fm ? ldh : 1, hs_n = fm ? 1 : ldh;

    T* Dn = reinterpret_cast<T*>(w.Dn);
    T* Dm = reinterpret_cast<T*>(w.Dm);
    T* P = reinterpret_cast<T*>(w.P);
    T* Wb[2] = {reinterpret_cast<T*>(w.W[0]), reinterpret_cast<T*>(w.W[1])};
    T* R = reinterpret_cast<T*>(w.R);
    T* Xm = reinterpret_cast<T*>(w.Xm);
    T* lam = reinterpret_cast<T*>(w.lam);
    T* tolv = reinterpret_cast<T*>(w.tolv);
    T* d = reinterpret_cast<T*>(w.d);
    T* colsum = reinterpret_cast<T*>(w.colsum);
    T* wbar = reinterpret_cast<T*>(w.wbar);
    T* sv = reinterpret_cast<T*>(w.s);
    T* cf = reinterpret_cast<T*>(w.cf);
    auto prepare = [&]() -> int {
        HIP_TRY(hipMemsetAsync(Dn, 0, (size_t)NK * MP * sizeof(T), s));
        HIP_TRY(hipMemsetAsync(Dm, 0, (size_t)MK * NP * sizeof(T), s));
        hipLaunchKernelGGL(k_pm_norm<T>, dim3(prox_blocks_of(N)), dim3(256), 0, s, A, as_n, as_m, M, N, o.normalize, (T)o.alpha,
                           (T)o.tol, d, lam, tolv);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_pm_images<T>, dim3(prox_blocks_of((long)N * M)), dim3(256), 0, s, A, as_n, as_m, M, N, fm ? 0 : 1,
                           o.normalize, (const T*)d, Dn, MP, Dm, NP);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_pm_frames<T>, dim3(prox_blocks_of(T_)), dim3(256), 0, s, X, xs_t, xs_m, mask, ms_t, ms_m, M, T_,
                           o.normalize, cf, Xm);
        HIP_TRY(hipGetLastError());
        const int n_bounds = mask ? n_utt : 1;  // without a mask every utterance has the same bound
        if (!(o.lipschitz > 0.0)) {
            hipLaunchKernelGGL(k_pm_wbar<T>, dim3(n_bounds, M), dim3(256), 0, s, mask, ms_t, ms_m, M, (const int*)w.offs,
                               o.lip_weights == EVC_PROX_LIP_MAX ? 1 : 0, wbar);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_pm_bound<T>, dim3(n_bounds, NP / PM_BOUND_COLS), dim3(PM_BOUND_COLS), 0, s, (const T*)Dm, NP, M, N,
                               (const T*)wbar, colsum);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_pm_lip<T>, dim3(n_utt), dim3(256), 0, s, (const T*)colsum, N, mask ? 1 : 0, (T)o.lipschitz, sv);
        HIP_TRY(hipGetLastError());
        HIP_TRY(gemm_strided<T>(Dm, 1, NP, Xm, 1, T_, P, T_, 1, N, T_, M, s));
        hipLaunchKernelGGL(k_prox_start<T>, dim3(prox_blocks_of((long)N * T_)), dim3(256), 0, s, (T*)nullptr, H, hs_t, hs_n, Wb[0],
                           (const T*)d, N, T_, fm ? 1 : 0, o.normalize, o.init_mode == EVC_INIT_GIVEN ? 1 : 0, (T)o.init_value);
        return (int)hipGetLastError();
    };

    PmResidArgs<T> ra;
    ra.Dn = Dn; ra.R = R; ra.mask = mask; ra.ms_t = ms_t; ra.ms_m = ms_m; ra.frame_utt = w.frame_utt; ra.stop = w.stop;
    ra.M = M; ra.MP = MP; ra.N = N; ra.T_ = T_;
    PmBackArgs<T> ba;
    ba.Dm = Dm; ba.R = R; ba.P = P; ba.X = H; ba.xs_t = hs_t; ba.xs_n = hs_n; ba.lam = lam; ba.cf = cf; ba.tolv = tolv;
    ba.s = sv; ba.frame_utt = w.frame_utt; ba.stop = w.stop;
    ba.M = M; ba.N = N; ba.NP = NP; ba.T_ = T_; ba.signed_mode = o.mode == EVC_PROX_SIGNED ? 1 : 0;
    const int Wr = pm_resid_waves(M, T_), Wk = pm_back_waves(N, T_);
    const unsigned frame_blocks = (unsigned)((T_ + PROX_BT - 1) / PROX_BT);
    const int row_blocks = (N + 16 * Wk - 1) / (16 * Wk);
    const dim3 rgrid(frame_blocks, (unsigned)((M + 16 * Wr - 1) / (16 * Wr))), bgrid(frame_blocks, (unsigned)row_blocks);
    auto sweep = [&](int, const T* Win, T* Wout, double* partials, T c) -> int {
        ra.Win = ba.Win = Win;
        ba.Wout = Wout; ba.partials = partials; ba.c = c;
        if (Wr == 8) hipLaunchKernelGGL((k_prox_resid<T, 8>), rgrid, dim3(512), 0, s, ra);
        else hipLaunchKernelGGL((k_prox_resid<T, 4>), rgrid, dim3(256), 0, s, ra);
        HIP_TRY(hipGetLastError());
        if (Wk == 8) hipLaunchKernelGGL((k_prox_back<T, 8>), bgrid, dim3(512), 0, s, ba);
        else hipLaunchKernelGGL((k_prox_back<T, 4>), bgrid, dim3(256), 0, s, ba);
        return (int)hipGetLastError();
    };
    return prox_solve_frame<T>(o, w, Wb, (const T*)d, row_blocks, H, hs_t, hs_n, fm ? 1 : 0, N, T_, utt_offsets, n_utt,
                               n_iter_out, change_out, s, prepare, sweep);
}

}  // namespace

}  // namespace evc

extern "C" {

size_t evc_prox_masked_workspace_bytes(int M, int N, int T, int n_utt, int dtype) {
    return evc::prox_masked_workspace_bytes(M, N, T, n_utt, dtype);
}

int evc_prox_masked_solve(const void* A, int lda, const void* X, int ldx, const void* mask, int ldm, void* H, int ldh, int M,
                          int N, int T, const int* utt_offsets, int n_utt, const evc_prox_masked_opts* opts, void* workspace,
                          size_t workspace_bytes, int* n_iter_out, double* change_out, evc_stream_t stream) {
    using namespace evc;
    HIP_TRY(prox_masked_args_check(A, lda, X, ldx, mask, ldm, H, ldh, M, N, T, utt_offsets, n_utt, opts, workspace,
                                   workspace_bytes));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (opts->dtype == EVC_F64)
        return prox_masked_solve<double>(static_cast<const double*>(A), lda, static_cast<const double*>(X), ldx,
                                         static_cast<const double*>(mask), ldm, static_cast<double*>(H), ldh, M, N, T,
                                         utt_offsets, n_utt, *opts, workspace, workspace_bytes, n_iter_out, change_out, s);
    return prox_masked_solve<float>(static_cast<const float*>(A), lda, static_cast<const float*>(X), ldx,
                                    static_cast<const float*>(mask), ldm, static_cast<float*>(H), ldh, M, N, T, utt_offsets,
                                    n_utt, *opts, workspace, workspace_bytes, n_iter_out, change_out, s);
}

}  // extern "C"
