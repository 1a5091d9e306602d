// evc_prox.hip - evc_prox_solve: L1-penalised activations by proximal gradient, ISTA / FISTA / Nesterov, signed or
// non-negative (deComP lasso.py:97-189, 228-256, 274-297, 331-357, 388-415; math_utils/eigen.py:9-20).  DESIGN.md §5.17.
//
// Once per call:  G = A^T A (N x N, zero-padded to NP = round_up(N, 128) in both directions) and P = A^T X (N x T), both by
// the bounds-checked strided contraction on the caller's A and X (nothing is packed); k_prox_diag, k_prox_scale and
// k_prox_lip leave d, the scaled G, lambda, tol_n, the Gershgorin bound L (column sums k-ascending, their maximum in one
// block's fixed tree), s = 1 / L and thr = s lambda; k_prox_start scales P and the start and copies the start to W_0.
// Per iteration i:
//     V = W + s (P - G W);   X_new = max(V - thr, 0)  |  sign(V) max(|V| - thr, 0);   W' = X_new + c_i (X_new - X_old)
//
// k_prox_sweep<T, W>: one launch per iteration, k_semi_sweep's geometry (evc_semi.hip) with one accumulator per output: a
// workgroup of W = 8 wavefronts owns PROX_BN = 128 exemplar rows x PROX_BT = 64 frame columns (W = 4, 64 rows, where
// 128-row workgroups would leave compute units empty: prox_waves decides from the sizes alone, and an output's bits do not
// depend on W).  It streams G[k, rows] (G is symmetric: the rows of the block are read as columns of the k-slab, contiguous
// in memory) and W_in[k, frames] for k ascending over the whole of N in slabs of PROX_KS = 16, double-buffered in LDS: the
// next slab's global loads fly while this one is multiplied, one barrier per slab.  A wavefront owns 16 rows x 64 frames:
// per k-step of 4 it reads one fragment of G and four of W_in and issues four 16x16x4 MFMAs into 4 accumulators.  The LDS
// rows are 16 elements longer than the block.  The epilogue reads P, W_in and X_old of its own block, writes X_new in place
// (H, the caller's strides: an element is read by its owner only) and W' to the OTHER W buffer (every workgroup reads whole
// columns of W_in).  On a check iteration it also reduces |X_new - X_old| - tol_n over its rows per frame - registers, wave
// shuffle, LDS - and stores one share per (row block, frame); k_prox_check takes an utterance's maximum over row blocks
// and frames in a fixed order, records it and sets stop[u].  A frame whose utterance has stopped is left as it is, and a
// workgroup none of whose frames is live returns at once.
// Every output's sum runs over k = 0 .. N - 1 in one fixed MFMA order: no split over k, no float atomics, no exchange between
// workgroups, no residency assumption.  A column of the accumulators only ever sees its own column of W: a batch gives
// bitwise the per-utterance results and a NaN stays in its frame's column.
// k_prox_start, k_prox_finish and k_prox_check live in evc_prox_kernels.h, which evc_prox_masked.hip includes too, with the host
// frame of a call (prox_solve_frame): here are the preparation and the sweep it is given.
#include "evc_prox_kernels.h"

namespace evc {

namespace {

constexpr int PROX_LDH = PROX_BT + 16;
constexpr int PROX_FT = PROX_BT / 16;        // frame tiles of 16 per wavefront
static_assert(PROX_KS == 16 && PROX_BT == 64, "the staging maps below are written for slabs of 16 x 64 frames");
static_assert(PROX_BN == 16 * PROX_MAX_WAVES, "G is padded to the widest row block");

template <typename T> struct ProxArgs {
    const T* G;             // [NP][NP]
    const T* P;             // [N][T_]
    const T* Win;           // [N][T_]
    T* Wout;                // [N][T_]
    T* X;                   // element (t, n) at t xs_t + n xs_n: X_old on entry, X_new on return
    long xs_t, xs_n;
    const T* thr;           // [N]
    const T* tolv;          // [N]
    const T* s;             // [1]: 1 / L
    double* partials;       // [row blocks][T_] on a check iteration, else NULL
    const int* frame_utt;
    const int* stop;
    int N, NP, T_;
    int signed_mode;
    T c;                    // the momentum coefficient of this iteration
};

// W wavefronts: the workgroup owns 16 W exemplar rows (8 or 4: prox_waves, evc_prox_plan.h, decides from the sizes alone)
// (the launch bound is the widest workgroup's for every W, as in k_semi_sweep)
template <typename T, int W>
__global__ __launch_bounds__(64 * PROX_MAX_WAVES) void k_prox_sweep(ProxArgs<T> a) {
    typedef typename Mma<T>::acc_t acc_t;
    typedef typename PVec4<T>::type vec_t;
    constexpr int THREADS = 64 * W, BN = 16 * W, LDG = BN + 16;
    constexpr int HE = PROX_KS * PROX_BT / THREADS;      // elements of the W_in slab per thread: 2 or 4
    __shared__ __attribute__((aligned(32))) T Gs[2][PROX_KS * LDG];
    __shared__ __attribute__((aligned(32))) T Hs[2][PROX_KS * PROX_LDH];
    __shared__ int live;
    static_assert(sizeof(T) * PROX_KS * LDG >= sizeof(double) * W * PROX_BT, "the epilogue's reduction reuses Gs[0]");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, q = lane >> 4;
    const long t0 = (long)blockIdx.x * PROX_BT;
    const int n0 = blockIdx.y * BN;           // n0 < N: the grid has ceil(N / BN) row blocks, and n0 + BN <= NP

    if (tid == 0) live = 0;
    __syncthreads();
    if (tid < PROX_BT && t0 + tid < a.T_ && a.stop[a.frame_utt[t0 + tid]] == 0) atomicOr(&live, 1);
    __syncthreads();
    if (!live) return;                        // uniform: every frame of the block belongs to a stopped utterance

    acc_t acc[PROX_FT];
#pragma unroll
    for (int j = 0; j < PROX_FT; ++j) acc[j] = acc_t{0, 0, 0, 0};

    // what a thread stages of a slab: one vector of four of G, HE elements of W_in (frames are its contiguous direction)
    const int g_row = tid / (4 * W), g_col = (tid % (4 * W)) * 4;
    const int h_t = tid & 63, h_k0 = tid >> 6;
    vec_t pg;
    T ph[HE];
    auto fetch = [&](int k0) {
        pg = *reinterpret_cast<const vec_t*>(a.G + (long)(k0 + g_row) * a.NP + n0 + g_col);      // k0 + g_row < NP: padded
#pragma unroll
        for (int e = 0; e < HE; ++e) {
            const int k = k0 + h_k0 + W * e;
            const long t = t0 + h_t;
            ph[e] = (k < a.N && t < a.T_) ? a.Win[(long)k * a.T_ + t] : T(0);
        }
    };
    auto stage = [&](int b) {
        *reinterpret_cast<vec_t*>(&Gs[b][g_row * LDG + g_col]) = pg;
#pragma unroll
        for (int e = 0; e < HE; ++e) Hs[b][(h_k0 + W * e) * PROX_LDH + h_t] = ph[e];
    };

    const int NS = (a.N + PROX_KS - 1) / PROX_KS;
    fetch(0);
    stage(0);
    __syncthreads();
#pragma unroll 1
    for (int sl = 0; sl < NS; ++sl) {
        const int b = sl & 1;
        if (sl + 1 < NS) fetch((sl + 1) * PROX_KS);
        const T* gs = &Gs[b][q * LDG + wave * 16 + i16];
        const T* hs = &Hs[b][q * PROX_LDH + i16];
#pragma unroll
        for (int st = 0; st < PROX_KS / 4; ++st) {
            const T g = gs[st * 4 * LDG];
#pragma unroll
            for (int j = 0; j < PROX_FT; ++j) acc[j] = Mma<T>::mma(g, hs[st * 4 * PROX_LDH + j * 16], acc[j]);
        }
        if (sl + 1 < NS) stage(b ^ 1);         // last read two barriers ago
        __syncthreads();
    }

    const T s = a.s[0];
    const bool check = a.partials != nullptr;  // uniform
    double* red = reinterpret_cast<double*>(&Gs[0][0]);      // [W][PROX_BT]: every read of Gs lies before the last barrier
#pragma unroll
    for (int j = 0; j < PROX_FT; ++j) {
        const long t = t0 + j * 16 + i16;
        double worst = -__builtin_inf();
        if (t < a.T_ && a.stop[a.frame_utt[t]] == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wave * 16 + Mma<T>::row(lane, r);
                if (n >= a.N) continue;
                const long at = (long)n * a.T_ + t;
                T* px = a.X + t * a.xs_t + n * a.xs_n;
                const T xo = *px;
                const T v = a.Win[at] + s * (a.P[at] - acc[j][r]);
                const T thr = a.thr[n];
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

// d_n = sqrt(G_nn) | 1;  thr_n = lambda_n = (alpha / d_n) M | alpha (k_prox_lip multiplies it by s);  tol_n = tol d_n | tol
template <typename T>
__global__ void k_prox_diag(const T* __restrict__ G, int N, int NP, int M, int normalize, T alpha, T tol, T* __restrict__ d,
                            T* __restrict__ thr, T* __restrict__ tolv) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const T dn = normalize ? psqrt(G[(long)n * NP + n]) : T(1);
    d[n] = dn;
    thr[n] = normalize ? (alpha / dn) * (T)M : alpha;
    tolv[n] = normalize ? tol * dn : tol;
}

// one thread per column n: G_kn <- G_kn / (d_k d_n) (the product commutes: G stays symmetric to the bit) and
// colsum_n = sum_k |G_kn| for k ascending
template <typename T>
__global__ void k_prox_scale(T* __restrict__ G, int N, int NP, int normalize, const T* __restrict__ d, T* __restrict__ colsum) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const T dn = d[n];
    T sum = T(0);
    for (int k = 0; k < N; ++k) {
        T g = G[(long)k * NP + n];
        if (normalize) {
            g = g / (d[k] * dn);
            G[(long)k * NP + n] = g;
        }
        sum += pabs(g);
    }
    colsum[n] = sum;
}

// one block: L = max_n colsum_n in a fixed order (a NaN wins, as numpy's max), s = 1 / L or 1 / lipschitz; thr_n = s lambda_n
template <typename T>
__global__ __launch_bounds__(256) void k_prox_lip(T* __restrict__ lip, int N, T lipschitz, T* __restrict__ thr) {
    __shared__ double red[256];
    double m = -__builtin_inf();
    for (int n = threadIdx.x; n < N; n += 256) m = nanmax(m, (double)lip[1 + n]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = nanmax(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    const T s = T(1) / (lipschitz > T(0) ? lipschitz : (T)red[0]);
    if (threadIdx.x == 0) lip[0] = s;
    for (int n = threadIdx.x; n < N; n += 256) thr[n] = s * thr[n];
}

// arguments already validated by prox_args_check; returns 0, -2 or a hipError_t
template <typename T>
int prox_solve(const T* A, int lda, const T* X, int ldx, T* H, int ldh, int M, int N, int T_, const int* utt_offsets, int n_utt,
               const evc_prox_opts& o, void* ws, size_t ws_bytes, int* n_iter_out, double* change_out, hipStream_t s) {
    const ProxWs w = carve_prox(ws, N, T_, n_utt, o.dtype);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    const int NP = round_up(N, PROX_BN);
    const long as_n = fm ? lda : 1, as_m = fm ? 1 : lda, xs_t = fm ? ldx : 1, xs_m = fm ? 1 : ldx;
    const long hs_t = fm ? ldh : 1, hs_n = fm ? 1 : ldh;

    T* G = reinterpret_cast<T*>(w.G);
    T* P = reinterpret_cast<T*>(w.P);
    T* Wb[2] = {reinterpret_cast<T*>(w.W[0]), reinterpret_cast<T*>(w.W[1])};
    T* thr = reinterpret_cast<T*>(w.thr);
    T* tolv = reinterpret_cast<T*>(w.tolv);
    T* d = reinterpret_cast<T*>(w.d);
    T* lip = reinterpret_cast<T*>(w.lip);
    auto prepare = [&]() -> int {
        HIP_TRY(hipMemsetAsync(G, 0, (size_t)NP * NP * sizeof(T), s));
        HIP_TRY(gemm_strided<T>(A, as_n, as_m, A, as_n, as_m, G, NP, 1, N, N, M, s));
        HIP_TRY(gemm_strided<T>(A, as_n, as_m, X, xs_t, xs_m, P, T_, 1, N, T_, M, s));
        const unsigned nbn = prox_blocks_of(N);
        hipLaunchKernelGGL(k_prox_diag<T>, dim3(nbn), dim3(256), 0, s, (const T*)G, N, NP, M, o.normalize, (T)o.alpha, (T)o.tol, d,
                           thr, tolv);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_prox_scale<T>, dim3(nbn), dim3(256), 0, s, G, N, NP, o.normalize, (const T*)d, lip + 1);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_prox_lip<T>, dim3(1), dim3(256), 0, s, lip, N, (T)o.lipschitz, thr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_prox_start<T>, dim3(prox_blocks_of((long)N * T_)), dim3(256), 0, s, P, H, hs_t, hs_n, Wb[0],
                           (const T*)d, N, T_, fm ? 1 : 0, o.normalize, o.init_mode == EVC_INIT_GIVEN ? 1 : 0, (T)o.init_value);
        return (int)hipGetLastError();
    };

    ProxArgs<T> a;
    a.G = G; a.P = P; a.X = H; a.xs_t = hs_t; a.xs_n = hs_n; a.thr = thr; a.tolv = tolv; a.s = lip;
    a.frame_utt = w.frame_utt; a.stop = w.stop;
    a.N = N; a.NP = NP; a.T_ = T_; a.signed_mode = o.mode == EVC_PROX_SIGNED ? 1 : 0;
    const int W = prox_waves(N, T_);
    const int row_blocks = (N + 16 * W - 1) / (16 * W);
    const dim3 grid((unsigned)((T_ + PROX_BT - 1) / PROX_BT), (unsigned)row_blocks);
    auto sweep = [&](int, const T* Win, T* Wout, double* partials, T c) -> int {
        a.Win = Win; a.Wout = Wout; a.partials = partials; a.c = c;
        if (W == 8) hipLaunchKernelGGL((k_prox_sweep<T, 8>), grid, dim3(512), 0, s, a);
        else hipLaunchKernelGGL((k_prox_sweep<T, 4>), grid, dim3(256), 0, s, a);
        return (int)hipGetLastError();
    };
    return prox_solve_frame<T>(o, w, Wb, (const T*)d, row_blocks, H, hs_t, hs_n, fm ? 1 : 0, N, T_, utt_offsets, n_utt,
                               n_iter_out, change_out, s, prepare, sweep);
}

}  // namespace

}  // namespace evc

extern "C" {

size_t evc_prox_workspace_bytes(int M, int N, int T, int n_utt, int dtype) {
    return evc::prox_workspace_bytes(M, N, T, n_utt, dtype);
}

int evc_prox_solve(const void* A, int lda, const void* X, int ldx, void* H, int ldh, int M, int N, int T,
                   const int* utt_offsets, int n_utt, const evc_prox_opts* opts, void* workspace, size_t workspace_bytes,
                   int* n_iter_out, double* change_out, evc_stream_t stream) {
    using namespace evc;
    HIP_TRY(prox_args_check(A, lda, X, ldx, H, ldh, M, N, T, utt_offsets, n_utt, opts, workspace, workspace_bytes));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (opts->dtype == EVC_F64)
        return prox_solve<double>(static_cast<const double*>(A), lda, static_cast<const double*>(X), ldx,
                                  static_cast<double*>(H), ldh, M, N, T, utt_offsets, n_utt, *opts, workspace, workspace_bytes,
                                  n_iter_out, change_out, s);
    return prox_solve<float>(static_cast<const float*>(A), lda, static_cast<const float*>(X), ldx, static_cast<float*>(H), ldh,
                             M, N, T, utt_offsets, n_utt, *opts, workspace, workspace_bytes, n_iter_out, change_out, s);
}

}  // extern "C"
