// evc_semi.hip - evc_semi_solve: semi-NMF activations with the dictionary fixed (Ding, Li and Jordan 2010; pymf snmf.py:66-85
// with compute_w=False).  X and A are signed, only H >= 0.  DESIGN.md §5.16.
//
// Once per call:  G = A^T A (N x N, zero-padded to NP = round_up(N, 128) in both directions) and P = A^T X (N x T), both by
// the bounds-checked strided contraction on the caller's A and X (nothing is packed).  Per iteration, with
// pos(m) = (|m| + m) / 2 and neg(m) = (|m| - m) / 2 as written:
//     H1 = pos(P) + neg(G) H;   H2 = (neg(P) + pos(G) H) + eps;   H' = H * sqrt(H1 / H2)
// The positive and negative parts of G do not factor through A, so this is a Gram-form sweep, and the two products are two
// sums of non-negative terms of their own: exact zeros stay exact.
//
// k_semi_sweep<T, W>: one launch per iteration, a workgroup of W = 8 wavefronts owns SEMI_BN = 128 exemplar rows x SEMI_BT = 64
// frame columns (W = 4, 64 rows, where 128-row workgroups would leave compute units empty: semi_waves decides from the
// sizes alone, and an output's bits do not depend on W).  It streams G[k, rows] (G is symmetric: the rows of the block are read as columns of the k-slab, contiguous
// in memory) and H[k, frames] for k ascending over the whole of N in slabs of SEMI_KS = 16, double-buffered in LDS: the next
// slab's global loads fly while this one is multiplied, one barrier per slab.  A wavefront owns 16 rows x 64 frames: per
// k-step of 4 it reads one fragment of G, splits it into pos and neg in registers, reads four fragments of H and issues eight
// 16x16x4 MFMAs into 4 + 4 accumulators.  The LDS rows are 16 elements longer than the block (the four lane groups of a
// fragment read fall into disjoint banks in both element types).  The epilogue reads P and the old H of the block and writes
// H' to the OTHER buffer - every output needs the whole old column - with the destination's own strides; a frame whose
// utterance has stopped is copied through, and a workgroup none of whose frames is live only copies.
// Every output's sums run over k = 0 .. N - 1 in one fixed MFMA order: no split over k, no float atomics, no exchange between
// workgroups, no residency assumption.  A column of the accumulators only ever sees its own column of H: a batch gives
// bitwise the per-utterance results and a NaN stays in its frame's column.
//
// The error: V = A H by the strided contraction, k_semi_err leaves every frame's squared residual (float64), k_semi_check
// sums an utterance's in a fixed order, records the square root and applies pymf's stop rule on the device.
// The per-utterance state, its head and the read-back are evc_solve_state.h's, shared with the proximal-gradient solves.
#include "evc_semi_plan.h"
#include "evc_solve_state.h"

namespace evc {

namespace {

constexpr int SEMI_LDH = SEMI_BT + 16;
constexpr int SEMI_FT = SEMI_BT / 16;        // frame tiles of 16 per wavefront
static_assert(SEMI_KS == 16 && SEMI_BT == 64, "the staging maps below are written for slabs of 16 x 64 frames");
static_assert(SEMI_BN == 16 * SEMI_MAX_WAVES, "G is padded to the widest row block");

template <typename T> struct Vec4;
template <> struct Vec4<double> { typedef f64x4 type; };
template <> struct Vec4<float> { typedef f32x4 type; };

__device__ __forceinline__ double absv(double v) { return __builtin_fabs(v); }
__device__ __forceinline__ float absv(float v) { return __builtin_fabsf(v); }
__device__ __forceinline__ double sqrtv(double v) { return sqrt(v); }
__device__ __forceinline__ float sqrtv(float v) { return sqrtf(v); }

template <typename T> struct SemiArgs {
    const T* G;             // [NP][NP]
    const T* P;             // [N][T_]
    const T* Hin;           // element (t, n) at t is_t + n is_n
    T* Hout;                // element (t, n) at t os_t + n os_n
    long is_t, is_n, os_t, os_n;
    const int* frame_utt;
    const int* stop;
    int N, NP, T_;
    T eps;
};

// W wavefronts: the workgroup owns 16 W exemplar rows (8 or 4: semi_waves, evc_semi_plan.h, decides from the sizes alone)
// (the launch bound is the widest workgroup's for every W: it keeps the narrower ones at its register count, so that as
// many wavefronts fit a compute unit)
template <typename T, int W>
__global__ __launch_bounds__(64 * SEMI_MAX_WAVES) void k_semi_sweep(SemiArgs<T> a) {
    typedef typename Mma<T>::acc_t acc_t;
    typedef typename Vec4<T>::type vec_t;
    constexpr int THREADS = 64 * W, BN = 16 * W, LDG = BN + 16;
    constexpr int HE = SEMI_KS * SEMI_BT / THREADS;      // elements of the H slab per thread: 2 or 4
    __shared__ __attribute__((aligned(32))) T Gs[2][SEMI_KS * LDG];
    __shared__ __attribute__((aligned(32))) T Hs[2][SEMI_KS * SEMI_LDH];
    __shared__ int live;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, q = lane >> 4;
    const long t0 = (long)blockIdx.x * SEMI_BT;
    const int n0 = blockIdx.y * BN;
    const bool k_fast = a.is_n == 1;          // the exemplars are the contiguous direction of the source

    if (tid == 0) live = 0;
    __syncthreads();
    if (tid < SEMI_BT && t0 + tid < a.T_ && a.stop[a.frame_utt[t0 + tid]] == 0) atomicOr(&live, 1);
    __syncthreads();
    if (!live) {                              // uniform: every frame of the block belongs to a stopped utterance
        for (int e = tid; e < BN * SEMI_BT; e += THREADS) {
            const int n = n0 + (k_fast ? e % BN : e / SEMI_BT);
            const long t = t0 + (k_fast ? e / BN : e % SEMI_BT);
            if (n < a.N && t < a.T_) a.Hout[t * a.os_t + n * a.os_n] = a.Hin[t * a.is_t + n * a.is_n];
        }
        return;
    }

    acc_t accp[SEMI_FT], accn[SEMI_FT];
#pragma unroll
    for (int j = 0; j < SEMI_FT; ++j) accp[j] = accn[j] = acc_t{0, 0, 0, 0};

    // what a thread stages of a slab: one vector of four of G, HE elements of H (along k where k is contiguous)
    const int g_row = tid / (4 * W), g_col = (tid % (4 * W)) * 4;
    int h_k[HE], h_t[HE];
#pragma unroll
    for (int e = 0; e < HE; ++e) {
        if (k_fast) { h_k[e] = tid & 15; h_t[e] = (tid >> 4) + 4 * W * e; } else { h_t[e] = tid & 63; h_k[e] = (tid >> 6) + W * e; }
    }
    vec_t pg;
    T ph[HE];
    auto fetch = [&](int k0) {
        pg = *reinterpret_cast<const vec_t*>(a.G + (long)(k0 + g_row) * a.NP + n0 + g_col);      // k0 + g_row < NP: padded
#pragma unroll
        for (int e = 0; e < HE; ++e) {
            const int k = k0 + h_k[e];
            const long t = t0 + h_t[e];
            ph[e] = (k < a.N && t < a.T_) ? a.Hin[t * a.is_t + (long)k * a.is_n] : T(0);
        }
    };
    auto stage = [&](int b) {
        *reinterpret_cast<vec_t*>(&Gs[b][g_row * LDG + g_col]) = pg;
#pragma unroll
        for (int e = 0; e < HE; ++e) Hs[b][h_k[e] * SEMI_LDH + h_t[e]] = ph[e];
    };

    const int NS = (a.N + SEMI_KS - 1) / SEMI_KS;
    fetch(0);
    stage(0);
    __syncthreads();
#pragma unroll 1
    for (int sl = 0; sl < NS; ++sl) {
        const int b = sl & 1;
        if (sl + 1 < NS) fetch((sl + 1) * SEMI_KS);
        const T* gs = &Gs[b][q * LDG + wave * 16 + i16];
        const T* hs = &Hs[b][q * SEMI_LDH + i16];
#pragma unroll
        for (int st = 0; st < SEMI_KS / 4; ++st) {
            const T g = gs[st * 4 * LDG];
            const T ga = absv(g);
            const T gp = (ga + g) * T(0.5), gn = (ga - g) * T(0.5);
#pragma unroll
            for (int j = 0; j < SEMI_FT; ++j) {
                const T h = hs[st * 4 * SEMI_LDH + j * 16];
                accp[j] = Mma<T>::mma(gp, h, accp[j]);
                accn[j] = Mma<T>::mma(gn, h, accn[j]);
            }
        }
        if (sl + 1 < NS) stage(b ^ 1);         // last read two barriers ago
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < SEMI_FT; ++j) {
        const long t = t0 + j * 16 + i16;
        if (t >= a.T_) continue;
        const bool stopped = a.stop[a.frame_utt[t]] != 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + wave * 16 + Mma<T>::row(lane, r);
            if (n >= a.N) continue;
            const T h = a.Hin[t * a.is_t + n * a.is_n];
            T hn = h;
            if (!stopped) {
                const T p = a.P[(long)n * a.T_ + t];
                const T pa = absv(p);
                const T h1 = (pa + p) * T(0.5) + accn[j][r];
                const T h2 = ((pa - p) * T(0.5) + accp[j][r]) + a.eps;
                hn = h * sqrtv(h1 / h2);
            }
            a.Hout[t * a.os_t + n * a.os_n] = hn;
        }
    }
}

// dst(t, n) = src ? src(t, n) : value over the N x T_ elements, each side with its own strides
template <typename T>
__global__ void k_semi_copy(const T* __restrict__ src, long ss_t, long ss_n, T* __restrict__ dst, long ds_t, long ds_n, int N,
                            int T_, int n_fast, T value) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)N * T_) return;
    const long t = n_fast ? i / N : i % T_;
    const long n = n_fast ? i % N : i / T_;
    dst[t * ds_t + n * ds_n] = src ? src[t * ss_t + n * ss_n] : value;
}

// err2[t] = sum_m (X(m, t) - V[t][m])^2 in float64; one wavefront per frame, shuffle reduction
template <typename T>
__global__ __launch_bounds__(256) void k_semi_err(const T* __restrict__ X, long xs_t, long xs_m, const T* __restrict__ V, int M,
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

// one block per utterance: err = sqrt(sum of its frames' shares), summed in an order that depends on the utterance's length
// only; check c (0: the start).  pymf base.py:189-206, 266-270: from the third update on, |ferr[i] - ferr[i-1]| / T_u < tol
// stops; a NaN error compares false and the utterance runs on
__global__ __launch_bounds__(256) void k_semi_check(const double* __restrict__ err2, const int* __restrict__ offs, int* stop,
                                                    double* eprev, double* trace, int n_slots, int c, int check_every,
                                                    int stop_rule, double tol) {
    __shared__ double red[256];
    const int u = blockIdx.x;
    const long i0 = offs[u], i1 = offs[u + 1];
    if (stop[u] != 0 || i0 == i1) return;       // uniform per block
    double acc = 0.0;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) acc += err2[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double err = sqrt(red[0]);
    trace[(long)u * n_slots + c] = err;
    if (c > 0 && stop_rule == EVC_STOP_PYMF && c >= 3 && fabs(err - eprev[u]) / (double)(i1 - i0) < tol)
        stop[u] = c * check_every;
    else
        eprev[u] = err;
}

unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

template <typename T> struct SemiBuf {
    T* p;
    long s_t, s_n;
};

// arguments already validated by semi_args_check; returns 0, -2 or a hipError_t
template <typename T>
int semi_solve(const T* A, int lda, const T* X, int ldx, T* H, int ldh, int M, int N, int T_, const int* utt_offsets, int n_utt,
               const evc_semi_opts& o, void* ws, size_t ws_bytes, int* n_iter_out, double* err_out, hipStream_t s) {
    const SemiWs w = carve_semi(ws, M, N, T_, n_utt, o.dtype);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    const int n_slots = n_slots_for(o.iters, o.check_every);
    const int NP = round_up(N, SEMI_BN);
    const long as_n = fm ? lda : 1, as_m = fm ? 1 : lda, xs_t = fm ? ldx : 1, xs_m = fm ? 1 : ldx;

    HIP_TRY(solve_state_head(utt_offsets, n_utt, T_, n_slots, w.offs, w.stop, w.trace, w.frame_utt, s));

    if (T_ > 0) {
        T* G = reinterpret_cast<T*>(w.G);
        T* P = reinterpret_cast<T*>(w.P);
        T* V = reinterpret_cast<T*>(w.V);
        HIP_TRY(hipMemsetAsync(G, 0, (size_t)NP * NP * sizeof(T), s));
        HIP_TRY(gemm_strided<T>(A, as_n, as_m, A, as_n, as_m, G, NP, 1, N, N, M, s));
        HIP_TRY(gemm_strided<T>(A, as_n, as_m, X, xs_t, xs_m, P, T_, 1, N, T_, M, s));

        // the caller's H and the packed second buffer; after `iters` swaps the result stands in the caller's
        const SemiBuf<T> own = {H, fm ? (long)ldh : 1L, fm ? 1L : (long)ldh};
        const SemiBuf<T> second = {reinterpret_cast<T*>(w.H2), fm ? (long)N : 1L, fm ? 1L : (long)T_};
        SemiBuf<T> cur = o.iters % 2 == 0 ? own : second, nxt = o.iters % 2 == 0 ? second : own;
        const unsigned nb = blocks_of((long)N * T_);
        if (o.init_mode == EVC_INIT_CONST) {
            hipLaunchKernelGGL(k_semi_copy<T>, dim3(nb), dim3(256), 0, s, (const T*)nullptr, 0L, 0L, cur.p, cur.s_t, cur.s_n, N, T_,
                               fm ? 1 : 0, (T)o.init_value);
            HIP_TRY(hipGetLastError());
        } else if (cur.p != H) {
            hipLaunchKernelGGL(k_semi_copy<T>, dim3(nb), dim3(256), 0, s, (const T*)H, own.s_t, own.s_n, cur.p, cur.s_t, cur.s_n, N,
                               T_, fm ? 1 : 0, T(0));
            HIP_TRY(hipGetLastError());
        }

        const bool checks = o.check_every > 0;
        auto check = [&](const SemiBuf<T>& b, int c) -> int {
            HIP_TRY(gemm_strided<T>(b.p, b.s_t, b.s_n, A, as_m, as_n, V, M, 1, T_, M, N, s));
            hipLaunchKernelGGL(k_semi_err<T>, dim3((T_ + 3) / 4), dim3(256), 0, s, X, xs_t, xs_m, (const T*)V, M, T_, w.err2);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_semi_check, dim3(n_utt), dim3(256), 0, s, (const double*)w.err2, (const int*)w.offs, w.stop,
                               w.eprev, w.trace, n_slots, c, o.check_every, o.stop_rule, o.tol);
            HIP_TRY(hipGetLastError());
            return 0;
        };
        if (checks) HIP_TRY(check(cur, 0));
        if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
        SemiArgs<T> a;
        a.G = G; a.P = P; a.frame_utt = w.frame_utt; a.stop = w.stop;
        a.N = N; a.NP = NP; a.T_ = T_; a.eps = (T)o.eps;
        const int W = semi_waves(N, T_);
        const dim3 grid((unsigned)((T_ + SEMI_BT - 1) / SEMI_BT), (unsigned)(NP / (16 * W)));
        for (int it = 1; it <= o.iters; ++it) {
            a.Hin = cur.p; a.is_t = cur.s_t; a.is_n = cur.s_n;
            a.Hout = nxt.p; a.os_t = nxt.s_t; a.os_n = nxt.s_n;
            if (W == 8) hipLaunchKernelGGL((k_semi_sweep<T, 8>), grid, dim3(512), 0, s, a);
            else hipLaunchKernelGGL((k_semi_sweep<T, 4>), grid, dim3(256), 0, s, a);
            HIP_TRY(hipGetLastError());
            const SemiBuf<T> tmp = cur; cur = nxt; nxt = tmp;
            if (checks && it % o.check_every == 0) HIP_TRY(check(cur, it / o.check_every));
        }
        if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    } else {
        if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
        if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    }

    return solve_read_back(w.stop, w.trace, n_utt, n_slots, o.iters, n_iter_out, err_out, s);
}

}  // namespace

}  // namespace evc

extern "C" {

size_t evc_semi_workspace_bytes(int M, int N, int T, int n_utt, int dtype) {
    return evc::semi_workspace_bytes(M, N, T, n_utt, dtype);
}

int evc_semi_solve(const void* A, int lda, const void* X, int ldx, void* H, int ldh, int M, int N, int T,
                   const int* utt_offsets, int n_utt, const evc_semi_opts* opts, void* workspace, size_t workspace_bytes,
                   int* n_iter_out, double* err_out, evc_stream_t stream) {
    using namespace evc;
    HIP_TRY(semi_args_check(A, lda, X, ldx, H, ldh, M, N, T, utt_offsets, n_utt, opts, workspace, workspace_bytes));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (opts->dtype == EVC_F64)
        return semi_solve<double>(static_cast<const double*>(A), lda, static_cast<const double*>(X), ldx,
                                  static_cast<double*>(H), ldh, M, N, T, utt_offsets, n_utt, *opts, workspace, workspace_bytes,
                                  n_iter_out, err_out, s);
    return semi_solve<float>(static_cast<const float*>(A), lda, static_cast<const float*>(X), ldx, static_cast<float*>(H), ldh,
                             M, N, T, utt_offsets, n_utt, *opts, workspace, workspace_bytes, n_iter_out, err_out, s);
}

}  // extern "C"
