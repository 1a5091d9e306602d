// evc_cd.hip - coordinate-descent activation solve: scikit-learn's solver='cd' with a fixed dictionary
// (non_negative_factorization(..., update_H=False, solver='cd', shuffle=False), _nmf.py:376-404,496-521 and
// _cdnmf_fast.pyx), the call of 04_align_n_nmf_pytorch.py:189-210.
//
// Algebra.  sklearn sweeps the components t = 0..N-1 in order and, for every frame, takes
//   grad = G[t,:] w - P[t]   (G = A A^T + l2 I, P = A x - l1),   w_t <- max(w_t - grad / G[t,t], 0)
// at 2N^2 flop per frame and sweep.  The same steps in the same order, reassociated: keep the residual
// r = w A - x of every frame (M values), then grad_t = r . a_t + l2 w_t + l1 and every step adds delta_t a_t to r:
// 4MN flop.  The components are taken in blocks of 16: the block's 16 gradients are formed from r at the block's
// start (16 dot products of length M), the 16 steps run in order and correct the later gradients of the block with
// the block's diagonal Gram block G_bb (a rank-1 update per step), then r += sum_j delta_j a_j.  Only the rounding
// differs from sklearn.  The division grad / hess is the IEEE one (no reciprocal), as in sklearn.
//
// Kernel k_cd_sweep<T, MPL>: plain VALU arithmetic (float64 / float32), one wavefront per frame tile.  A frame
// is served by a group of L lanes (L a power of two, from M alone: the smallest with ceil(M / L) <= 16); lane q of
// the group holds r[m] for m = q, q + L, ... in registers (MPL >= ceil(M / L) slots), the group's partial dot products
// are summed by an xor butterfly (bitwise the same sum in every lane of the group), and every lane of the group runs
// the 16 sequential steps.  A tile is 64 / L frames of ONE utterance (utterances start at a tile boundary), so the
// arithmetic of a frame never depends on the other frames of the call: a batched solve is bitwise the solo solves.
//
// One launch per iteration; no inter-workgroup exchange inside a launch.  Launch k first judges iteration k-1 of
// its utterance: every workgroup sums the per-tile violation partials of the previous launch in tile order (the same
// bits in every workgroup), applies sklearn's rule (violation_init == 0, or violation / violation_init <= tol, or
// max_iter reached) and returns at once if the utterance has stopped; the utterance's first tile records the value,
// violation_init and the stop iteration.  A final launch (k = max_iter + 1) only judges.  The violation is
// accumulated in float64 for both element types; padded frames contribute nothing.
//
// evc_cd_learn (the end of this file) alternates that sweep with a Gram-form sweep over the dictionary's rows
// (k_cd_dict_sweep): sklearn's solver='cd' with update_H=True.
#include "evc_internal.h"

namespace evc {

namespace {

constexpr int CD_B = 16;        // components per block
constexpr int CD_WAVE = 64;

// the packed dictionary: blocks of 16 components, bin-major inside a block (the 16 values a lane needs for one bin
// are contiguous)
__device__ __forceinline__ long cd_at(int n, int m, int Mr) { return ((long)(n / CD_B) * Mr + m) * CD_B + n % CD_B; }

template <typename T>
__global__ void k_cd_pack_dict(const T* __restrict__ A, int lda, int fm, int M, int N, int Np, int Mr,
                               T* __restrict__ Ac) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)Np * Mr) return;
    const int n = (int)(i / Mr), m = (int)(i % Mr);
    T v = T(0);
    if (n < N && m < M) v = fm ? A[(long)n * lda + m] : A[(long)m * lda + n];
    Ac[cd_at(n, m, Mr)] = v;
}

// one workgroup of 16 x 16 threads per block of 16 components: Gb[b][j][k] = a_j . a_k, hess = |a_j|^2 + l2
template <typename T>
__global__ void k_cd_gram_blocks(const T* __restrict__ Ac, int M, int N, int Mr, double l2, T* __restrict__ Gb,
                                 T* __restrict__ hess) {
    const int b = blockIdx.x, j = threadIdx.x >> 4, k = threadIdx.x & 15;
    T s = T(0);
    for (int m = 0; m < M; ++m) s += Ac[cd_at(b * CD_B + j, m, Mr)] * Ac[cd_at(b * CD_B + k, m, Mr)];
    Gb[(long)b * CD_B * CD_B + j * CD_B + k] = s;
    if (j == k) {
        const int c = b * CD_B + j;
        hess[c] = c < N ? s + (T)l2 : T(0);
    }
}

// r = w A - x per frame slot (w = H on entry for EVC_INIT_GIVEN, else 0 and H is zeroed by the host); padding 0
template <typename T>
__global__ void k_cd_init_resid(const T* __restrict__ X, int ldx, const T* __restrict__ H, int ldh, int fm, int given,
                                const T* __restrict__ Ac, const int4* __restrict__ tiles, int n_tiles, int F, int M,
                                int N, int Mr, T* __restrict__ R) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n_tiles * F * Mr) return;
    const long slot = i / Mr;
    const int m = (int)(i % Mr);
    const int4 tl = tiles[slot / F];
    const int g = (int)(slot % F);
    T v = T(0);
    if (g < tl.z && m < M) {
        const long f = tl.y + g;
        if (given)
            for (int n = 0; n < N; ++n) v += (fm ? H[f * ldh + n] : H[(long)n * ldh + f]) * Ac[cd_at(n, m, Mr)];
        v -= fm ? X[f * ldx + m] : X[(long)m * ldx + f];
    }
    R[i] = v;
}

}  // namespace

template <typename T> struct CdArgs {
    const T* Ac;            // [Np/16][Mr][16] dictionary rows, zero-padded (cd_at)
    const T* Gb;            // [Np/16][16][16] diagonal Gram blocks
    const T* hess;          // [Np] |a_t|^2 + l2 (0 for padding components)
    T* R;                   // [n_tiles * F][Mr] residual w A - x of every frame slot
    T* H;
    long ldh;
    int fm;                 // 1: H[t * ldh + n]; 0: H[n * ldh + t]
    const int4* tiles;      // {utterance, first frame, frames, first tile of the utterance}
    const int* utt_tile0;   // [n_utt + 1] first tile of every utterance
    double* part;           // [2][n_tiles] per-tile violation of the last two launches
    int* stop;              // [n_utt] 0: running; else the iteration the utterance stopped at (= n_iter)
    double* vinit;          // [n_utt]
    double* trace;          // [n_utt][CD_TRACE_CAP] violation of iteration i at slot (i - 1) % CD_TRACE_CAP
    int n_tiles, M, N, Np, Mr, L, mpl, max_iter;
    double tol;
    T l1, l2;
};

template <typename T, int MPL>
__global__ __launch_bounds__(CD_WAVE) void k_cd_sweep(CdArgs<T> a, int k) {
    __shared__ double sv[CD_WAVE];
    __shared__ T Gs[CD_B * CD_B + CD_B];            // the block's G_bb, then its 16 hess values
    const int tile = blockIdx.x;
    const int4 tl = a.tiles[tile];
    const int u = tl.x;
    if (a.stop[u] != 0) return;
    if (k >= 2) {                                  // judge iteration k - 1 of utterance u
        const int it = k - 1;
        const double* p = a.part + (size_t)(it & 1) * a.n_tiles;
        double s = 0.0;
        for (int q = a.utt_tile0[u]; q < a.utt_tile0[u + 1]; ++q) s += p[q];
        const double vi = it == 1 ? s : a.vinit[u];
        const bool stop_now = vi == 0.0 || s / vi <= a.tol || it >= a.max_iter;
        if (tile == tl.w && threadIdx.x == 0) {
            a.trace[(size_t)u * CD_TRACE_CAP + (it - 1) % CD_TRACE_CAP] = s;
            if (it == 1) a.vinit[u] = s;
            if (stop_now) a.stop[u] = it;
        }
        if (stop_now) return;
    }
    const int L = a.L;
    const int mpl = a.mpl;
    const int lane = threadIdx.x;
    const int g = lane / L;                        // frame of the tile
    const int q = lane % L;                        // lane in the frame's group
    const int F = CD_WAVE / L;
    const bool valid = g < tl.z;
    const long f = (long)tl.y + g;
    const long slot = (long)tile * F + g;
    T* Rs = a.R + slot * a.Mr + q;
    T r[MPL];
#pragma unroll
    for (int kk = 0; kk < MPL; ++kk) r[kk] = kk < mpl ? Rs[kk * L] : T(0);
    const long hs_t = a.fm ? a.ldh : 1, hs_n = a.fm ? 1 : a.ldh;
    T* Hf = a.H + (valid ? f : 0) * hs_t;
    double viol = 0.0;
    const int nb = a.Np / CD_B;
#pragma unroll 1
    for (int b = 0; b < nb; ++b) {
        const int c0 = b * CD_B;
        T w[CD_B], gr[CD_B], d[CD_B];
#pragma unroll
        for (int j = 0; j < CD_B; ++j) {      // branch-free: clamped address, then select
            const int c = c0 + j < a.N ? c0 + j : a.N - 1;
            const T v = Hf[c * hs_n];
            w[j] = (valid && c0 + j < a.N) ? v : T(0);
        }
        const T* Ab = a.Ac + ((long)b * a.Mr + q) * CD_B;     // a_{c0+j}[q + L kk] at Ab[kk * L * 16 + j]
        {
            const T* G = a.Gb + (long)b * CD_B * CD_B;
#pragma unroll
            for (int i = 0; i < CD_B * CD_B / CD_WAVE; ++i) Gs[i * CD_WAVE + lane] = G[i * CD_WAVE + lane];
            if (lane < CD_B) Gs[CD_B * CD_B + lane] = a.hess[c0 + lane];
        }
        __syncthreads();
        // 1. the block's gradients at its start: r . a_j, summed over the lane group
#pragma unroll
        for (int j = 0; j < CD_B; ++j) gr[j] = T(0);
#pragma unroll
        for (int kk = 0; kk < MPL; ++kk)
            if (kk < mpl) {
                const T* ap = Ab + (long)kk * L * CD_B;
#pragma unroll
                for (int j = 0; j < CD_B; ++j) gr[j] = fma(r[kk], ap[j], gr[j]);
            }
#pragma unroll 1
        for (int o = 1; o < L; o <<= 1)
#pragma unroll
            for (int j = 0; j < CD_B; ++j) gr[j] += __shfl_xor(gr[j], o);
#pragma unroll
        for (int j = 0; j < CD_B; ++j) gr[j] = (gr[j] + a.l2 * w[j]) + a.l1;
        // 2. the 16 coordinate steps in sklearn's order
#pragma unroll
        for (int j = 0; j < CD_B; ++j) {
            // keep the compiler from hoisting every step's 15 Gram reads to the top of the block (a register per value)
            __asm__ volatile("" ::: "memory");
            const T grad = gr[j];
            const T pg = w[j] == T(0) ? (grad < T(0) ? grad : T(0)) : grad;
            if (c0 + j < a.N) viol += fabs((double)pg);
            const T h = Gs[CD_B * CD_B + j];
            T dj = T(0);
            if (h != T(0)) {
                const T v = w[j] - grad / h;
                const T nw = v > T(0) ? v : T(0);
                dj = nw - w[j];
                w[j] = nw;
            }
            d[j] = dj;
#pragma unroll
            for (int kk = j + 1; kk < CD_B; ++kk) gr[kk] = fma(dj, Gs[j * CD_B + kk], gr[kk]);
        }
        if (valid && q == 0) {
#pragma unroll
            for (int j = 0; j < CD_B; ++j)
                if (c0 + j < a.N) Hf[(c0 + j) * hs_n] = w[j];
        }
        // 3. r += sum_j delta_j a_j (j in order)
#pragma unroll
        for (int kk = 0; kk < MPL; ++kk)
            if (kk < mpl) {
                const T* ap = Ab + (long)kk * L * CD_B;
                T v = r[kk];
#pragma unroll
                for (int j = 0; j < CD_B; ++j) v = fma(d[j], ap[j], v);
                r[kk] = v;
            }
        __syncthreads();
    }
#pragma unroll
    for (int kk = 0; kk < MPL; ++kk)
        if (kk < mpl) Rs[kk * L] = r[kk];
    if (q == 0) sv[g] = valid ? viol : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < F; ++i) s += sv[i];
        a.part[(size_t)(k & 1) * a.n_tiles + tile] = s;
    }
}

CdGeometry cd_geometry(int M) {
    CdGeometry g{};
    if (M < 1 || M > CD_MAX_M) return g;
    int L = 1;
    while ((M + L - 1) / L > 16) L *= 2;
    g.L = L;
    g.mpl = (M + L - 1) / L;
    g.Mr = g.mpl * L;
    g.F = CD_WAVE / L;
    return g;
}

namespace {

template <typename T, int MPL>
hipError_t launch_sweep_mpl(const CdArgs<T>& a, int k, hipStream_t s) {
    hipLaunchKernelGGL((k_cd_sweep<T, MPL>), dim3(a.n_tiles), dim3(CD_WAVE), 0, s, a, k);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_sweep(const CdArgs<T>& a, int k, hipStream_t s) {
    if (a.mpl <= 1) return launch_sweep_mpl<T, 1>(a, k, s);
    if (a.mpl <= 8) return launch_sweep_mpl<T, 8>(a, k, s);
    return launch_sweep_mpl<T, 16>(a, k, s);
}

__global__ void k_cd_state_init(int* stop, double* vinit, double* trace, int n_utt) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_utt) {
        stop[i] = 0;
        vinit[i] = 0.0;
    }
    if (i < (long)n_utt * CD_TRACE_CAP) trace[i] = __builtin_nan("");
}

template <typename T> struct CdWs {
    T *Ac, *Gb, *hess, *R;
    int4* tiles;
    int* utt_tile0;
    double* part;
    int* stop;
    double *vinit, *trace;
    size_t bytes;
};

// The workspace: [Ac | Gb | hess | R | tiles | utt_tile0 | part | stop | vinit | trace], each 256-byte aligned (ws == NULL:
// sizes only).
template <typename T> CdWs<T> carve_cd(void* ws, const CdGeometry& g, int N, int T_, int n_utt) {
    CdWs<T> w;
    Carver c = Carver::rounded(ws);
    const size_t Np = (size_t)round_up(N, CD_B);
    const size_t nt = (size_t)frame_tile_cap(T_, g.F, n_utt);
    w.Ac = c.take<T>(Np * g.Mr);
    w.Gb = c.take<T>(Np * CD_B);
    w.hess = c.take<T>(Np);
    w.R = c.take<T>(nt * g.F * g.Mr);
    w.tiles = c.take<int4>(nt);
    w.utt_tile0 = c.take<int>((size_t)n_utt + 1);
    w.part = c.take<double>(2 * nt);
    w.stop = c.take<int>(n_utt);
    w.vinit = c.take<double>(n_utt);
    w.trace = c.take<double>((size_t)n_utt * CD_TRACE_CAP);
    w.bytes = c.bytes();
    return w;
}

}  // namespace

size_t cd_workspace_bytes(int M, int N, int T_, int n_utt, int esize) {
    const CdGeometry g = cd_geometry(M);
    if (g.L == 0 || N < 1 || T_ < 0 || n_utt < 1 || (esize != 4 && esize != 8)) return 0;
    return (esize == 8 ? carve_cd<double>(nullptr, g, N, T_, n_utt).bytes : carve_cd<float>(nullptr, g, N, T_, n_utt).bytes) + 256;
}

namespace {

// Carves the workspace, stages the tile table and clears the per-utterance state; everything of CdArgs but the
// dictionary-dependent arrays' contents (cd_refresh) is final afterwards.  Returns ST_OK, ST_BADARG, ST_WORKSPACE or a hipError_t.
template <typename T>
int cd_setup(T* H, int ldh, int M, int N, int T_, const int* utt_offsets, int n_utt, bool fm, int max_iter, double tol,
             double l1, double l2, void* ws, size_t ws_bytes, hipStream_t s, CdArgs<T>* out) {
    const CdGeometry g = cd_geometry(M);
    const int Np = round_up(N, CD_B);
    const CdWs<T> w = carve_cd<T>(ws, g, N, T_, n_utt);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    int n_tiles;
    HIP_TRY(frame_tiles_stage(g.F, utt_offsets, n_utt, T_, w.tiles, w.utt_tile0, nullptr, s, &n_tiles));
    {
        const long n = (long)n_utt * CD_TRACE_CAP;
        hipLaunchKernelGGL(k_cd_state_init, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w.stop, w.vinit, w.trace,
                           n_utt);
        HIP_TRY(hipGetLastError());
    }
    CdArgs<T>& a = *out;
    a.Ac = w.Ac; a.Gb = w.Gb; a.hess = w.hess; a.R = w.R; a.H = H; a.ldh = ldh; a.fm = fm ? 1 : 0;
    a.tiles = w.tiles; a.utt_tile0 = w.utt_tile0; a.part = w.part; a.stop = w.stop; a.vinit = w.vinit; a.trace = w.trace;
    a.n_tiles = n_tiles; a.M = M; a.N = N; a.Np = Np; a.Mr = g.Mr; a.L = g.L; a.mpl = g.mpl;
    a.max_iter = max_iter; a.tol = tol; a.l1 = (T)l1; a.l2 = (T)l2;
    return 0;
}

// What depends on the dictionary and on the start: the packed dictionary, its diagonal Gram blocks and the residual
// h A - x of every frame slot (given: from the activations in a.H; else from 0).
template <typename T>
int cd_refresh(const CdArgs<T>& a, const T* A, int lda, const T* X, int ldx, int given, double l2, hipStream_t s) {
    const int F = CD_WAVE / a.L;
    {
        const long n = (long)a.Np * a.Mr;
        hipLaunchKernelGGL(k_cd_pack_dict<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, A, lda, a.fm, a.M, a.N,
                           a.Np, a.Mr, const_cast<T*>(a.Ac));
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_cd_gram_blocks<T>, dim3(a.Np / CD_B), dim3(CD_B * CD_B), 0, s, a.Ac, a.M, a.N, a.Mr, l2,
                           const_cast<T*>(a.Gb), const_cast<T*>(a.hess));
        HIP_TRY(hipGetLastError());
    }
    if (a.n_tiles > 0) {
        const long n = (long)a.n_tiles * F * a.Mr;
        hipLaunchKernelGGL(k_cd_init_resid<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, X, ldx, a.H, (int)a.ldh,
                           a.fm, given, a.Ac, a.tiles, a.n_tiles, F, a.M, a.N, a.Mr, a.R);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// arguments already validated by evc_cd_solve; returns 0, -1, -2 or a hipError_t
template <typename T>
int cd_solve(const T* A, int lda, const T* X, int ldx, T* H, int ldh, int M, int N, int T_, const int* utt_offsets,
             int n_utt, const evc_cd_opts& o, void* ws, size_t ws_bytes, int* n_iter_out, double* violation_out,
             hipStream_t s, int* launches_out) {
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    CdArgs<T> a;
    {
        const int st = cd_setup<T>(H, ldh, M, N, T_, utt_offsets, n_utt, fm, o.max_iter, o.tol, o.l1, o.l2, ws, ws_bytes, s,
                                   &a);
        if (st != 0) return st;
    }
    const int n_tiles = a.n_tiles;
    int* const stop = a.stop;
    double* const trace = a.trace;
    hipError_t e = hipSuccess;
    const int es = (int)sizeof(T);
    if (o.init_mode == EVC_INIT_SKLEARN && T_ > 0) {
        if (fm) HIP_TRY(hipMemset2DAsync(H, (size_t)ldh * es, 0, (size_t)N * es, T_, s));
        else HIP_TRY(hipMemset2DAsync(H, (size_t)ldh * es, 0, (size_t)T_ * es, N, s));
    }
    {
        const int st = cd_refresh<T>(a, A, lda, X, ldx, o.init_mode == EVC_INIT_GIVEN ? 1 : 0, o.l2, s);
        if (st != 0) return st;
    }

    const bool run = n_tiles > 0 && o.max_iter > 0;
    int launches = 0;
    int copied = 0;         // iterations whose violation has been copied to violation_out
    if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
    if (run) {
        for (int k = 1; k <= o.max_iter + 1; ++k) {
            HIP_TRY(launch_sweep<T>(a, k, s));
            ++launches;
            const int judged = k - 1;
            if (violation_out && judged > copied && (judged - copied == CD_TRACE_CAP || k == o.max_iter + 1)) {
                const int cnt = judged - copied;
                HIP_TRY(hipMemcpy2DAsync(violation_out + copied, sizeof(double) * o.max_iter, trace,
                                         sizeof(double) * CD_TRACE_CAP, sizeof(double) * cnt, n_utt,
                                         hipMemcpyDeviceToHost, s));
                copied = judged;
            }
        }
    }
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    if (launches_out) *launches_out = launches;
    if (n_iter_out || violation_out) {
        int* ni_h = static_cast<int*>(malloc(sizeof(int) * n_utt));
        if (!ni_h) return (int)hipErrorOutOfMemory;
        e = run ? hipMemcpyAsync(ni_h, stop, sizeof(int) * n_utt, hipMemcpyDeviceToHost, s) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        for (int u = 0; e == hipSuccess && u < n_utt; ++u) {
            const int tu = utt_offsets ? utt_offsets[u + 1] - utt_offsets[u] : T_;
            // an utterance without frames has violation 0 at its first iteration, where sklearn's rule stops it
            const int ni = o.max_iter == 0 ? 0 : (tu == 0 || !run) ? 1 : ni_h[u];
            if (n_iter_out) n_iter_out[u] = ni;
            if (violation_out)
                for (int i = 0; i < o.max_iter; ++i) {
                    double* v = violation_out + (size_t)u * o.max_iter + i;
                    if (i >= ni) *v = __builtin_nan("");
                    else if (tu == 0 || !run) *v = 0.0;
                }
        }
        free(ni_h);
        HIP_TRY(e);
    }
    return 0;
}

// ---- evc_cd_learn: the alternating form (sklearn solver='cd', update_H=True), DESIGN.md §5.8 ----
//
// Per iteration the activation half is one k_cd_sweep launch (k = 1: no judging) on the freshly packed dictionary, and
// the dictionary half is sklearn's _update_coordinate_descent(X^T, H^T, W) in Gram form: G = H H^T + l2 I and
// P = X H^T - l1 come from k_dict_grad's one-operand contraction (frames split into S ranges, partial sums added in
// ascending order by k_cdl_finish), then k_cd_dict_sweep runs the M independent row sweeps.

template <typename T> struct CdDictArgs {
    const T* G;             // [Rp][ld] H H^T + l2 I, rows and columns past R zero
    const T* P;             // [M][ld]  X H^T - l1
    const T* Gb;            // [Rp/16][16][16] diagonal blocks of G
    const T* hess;          // [Rp] G[t][t] (0 for padding components)
    T* W;
    long ws_m, ws_r;        // W[m * ws_m + r * ws_r]
    double* part;           // [ceil(M / (64 / L))] per-wavefront violation
    int ld, M, R, Rp, L, rpl;
};

// The sibling of k_cd_sweep with the Gram matrix in the dictionary's place: a dictionary row (one bin) is served by L
// lanes (from R alone), lane q keeps w[q], w[q + L], ... in registers; per block of 16 components the gradients at the
// block's start are 16 dot products G[c, :] . w summed by the xor butterfly, then every lane of the group runs the 16
// in-order steps and the owning lanes store the new values.  No residual, no second pass over G; a row's arithmetic
// does not depend on the other rows of its wavefront.  (The butterfly and the steps restate k_cd_sweep's: sharing
// them as device functions would have meant touching that kernel.)
template <typename T, int RPL>
__global__ __launch_bounds__(CD_WAVE) void k_cd_dict_sweep(CdDictArgs<T> a) {
    __shared__ double sv[CD_WAVE];
    __shared__ T Gs[CD_B * CD_B + CD_B];            // the block's G_bb, then its 16 hess values
    __shared__ T wn[CD_WAVE * CD_B];                // the block's new values, per row of the wavefront
    const int L = a.L, rpl = a.rpl;
    const int lane = threadIdx.x;
    const int g = lane / L;                        // row of the wavefront
    const int q = lane % L;                        // lane in the row's group
    const int F = CD_WAVE / L;
    const int m = blockIdx.x * F + g;
    const bool valid = m < a.M;
    T* Wm = a.W + (long)(valid ? m : 0) * a.ws_m;
    const T* Pm = a.P + (long)(valid ? m : 0) * a.ld;
    T w[RPL];
#pragma unroll
    for (int kk = 0; kk < RPL; ++kk) {
        const int c = q + kk * L;
        const T v = Wm[(long)(c < a.R ? c : a.R - 1) * a.ws_r];
        w[kk] = (valid && kk < rpl && c < a.R) ? v : T(0);
    }
    double viol = 0.0;
    const int nb = a.Rp / CD_B;
#pragma unroll 1
    for (int b = 0; b < nb; ++b) {
        const int c0 = b * CD_B;
        T wb[CD_B], gr[CD_B];
#pragma unroll
        for (int j = 0; j < CD_B; ++j) {
            const int c = c0 + j < a.R ? c0 + j : a.R - 1;
            const T v = Wm[(long)c * a.ws_r];
            wb[j] = (valid && c0 + j < a.R) ? v : T(0);
        }
        {
            const T* G = a.Gb + (long)b * CD_B * CD_B;
#pragma unroll
            for (int i = 0; i < CD_B * CD_B / CD_WAVE; ++i) Gs[i * CD_WAVE + lane] = G[i * CD_WAVE + lane];
            if (lane < CD_B) Gs[CD_B * CD_B + lane] = a.hess[c0 + lane];
        }
        __syncthreads();
        // 1. the block's gradients at its start: G[c0 + j, :] . w, summed over the lane group, minus P
#pragma unroll
        for (int j = 0; j < CD_B; ++j) gr[j] = T(0);
#pragma unroll
        for (int kk = 0; kk < RPL; ++kk)
            if (kk < rpl) {
                const T* gp = a.G + (long)c0 * a.ld + q + kk * L;
#pragma unroll
                for (int j = 0; j < CD_B; ++j) gr[j] = fma(gp[(long)j * a.ld], w[kk], gr[j]);
            }
#pragma unroll 1
        for (int o = 1; o < L; o <<= 1)
#pragma unroll
            for (int j = 0; j < CD_B; ++j) gr[j] += __shfl_xor(gr[j], o);
#pragma unroll
        for (int j = 0; j < CD_B; ++j) gr[j] -= Pm[c0 + j];
        // 2. the 16 coordinate steps in sklearn's order
#pragma unroll
        for (int j = 0; j < CD_B; ++j) {
            __asm__ volatile("" ::: "memory");      // as in k_cd_sweep: keep the Gram reads at their steps
            const T grad = gr[j];
            const T pg = wb[j] == T(0) ? (grad < T(0) ? grad : T(0)) : grad;
            if (valid && c0 + j < a.R) viol += fabs((double)pg);
            const T h = Gs[CD_B * CD_B + j];
            T dj = T(0);
            if (h != T(0)) {
                const T v = wb[j] - grad / h;
                const T nw = v > T(0) ? v : T(0);
                dj = nw - wb[j];
                wb[j] = nw;
            }
#pragma unroll
            for (int kk = j + 1; kk < CD_B; ++kk) gr[kk] = fma(dj, Gs[j * CD_B + kk], gr[kk]);
        }
        // 3. the lanes that own the block's components take the new values and store them
        if (q == 0) {
#pragma unroll
            for (int j = 0; j < CD_B; ++j) wn[g * CD_B + j] = wb[j];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < RPL; ++kk) {
            const int c = q + kk * L;
            if (kk < rpl && c >= c0 && c < c0 + CD_B) {
                const T v = wn[g * CD_B + (c - c0)];
                w[kk] = v;
                if (valid && c < a.R) Wm[(long)c * a.ws_r] = v;
            }
        }
        __syncthreads();
    }
    if (q == 0) sv[g] = valid ? viol : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < F; ++i) s += sv[i];
        a.part[blockIdx.x] = s;
    }
}

// G = sum_s partG[s] + l2 I (rows < Rp), P = sum_s partP[s] - l1 (rows < M), the slabs in the order s = 0 .. S-1; the
// diagonal 16 x 16 blocks and hess_t = G[t][t] go out as k_cd_gram_blocks leaves them for the activation side
template <typename T>
__global__ __launch_bounds__(256) void k_cdl_finish(const T* __restrict__ partG, long slabG, const T* __restrict__ partP,
                                                    long slabP, int S, int ld, int M, int R, int Rp, T l1, T l2,
                                                    T* __restrict__ G, T* __restrict__ P, T* __restrict__ Gb,
                                                    T* __restrict__ hess) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)(Rp + M) * ld) return;
    const int row = (int)(idx / ld), col = (int)(idx % ld);
    if (row < Rp) {
        const T* __restrict__ p = partG + (long)row * ld + col;
        T v = T(0);
        for (int s = 0; s < S; ++s) v += p[(long)s * 2 * slabG];
        if (row == col && row < R) v += l2;
        G[idx] = v;
        if (col < Rp && row / CD_B == col / CD_B) Gb[(long)(row / CD_B) * CD_B * CD_B + (row % CD_B) * CD_B + col % CD_B] = v;
        if (row == col) hess[row] = row < R ? v : T(0);
    } else {
        const int m = row - Rp;
        const T* __restrict__ p = partP + (long)m * ld + col;
        T v = T(0);
        for (int s = 0; s < S; ++s) v += p[(long)s * 2 * slabP];
        P[(long)m * ld + col] = v - l1;
    }
}

// out[0] = sum of the activation sweep's per-tile partials, out[1] = sum of the dictionary sweep's per-wavefront ones,
// each in a fixed order (256 strided sums, then a tree)
__global__ __launch_bounds__(256) void k_cdl_viol(const double* __restrict__ pa, int na, const double* __restrict__ pd,
                                                  int nd, double* __restrict__ out) {
    __shared__ double red[2][256];
    double sa = 0.0, sd = 0.0;
    for (int i = threadIdx.x; i < na; i += 256) sa += pa[i];
    for (int i = threadIdx.x; i < nd; i += 256) sd += pd[i];
    red[0][threadIdx.x] = sa;
    red[1][threadIdx.x] = sd;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = red[0][0];
        out[1] = red[1][0];
    }
}

template <typename T>
hipError_t launch_dict_sweep(const CdDictArgs<T>& a, hipStream_t s) {
    const int F = CD_WAVE / a.L;
    const dim3 grid((a.M + F - 1) / F), block(CD_WAVE);
    if (a.rpl <= 1) hipLaunchKernelGGL((k_cd_dict_sweep<T, 1>), grid, block, 0, s, a);
    else if (a.rpl <= 8) hipLaunchKernelGGL((k_cd_dict_sweep<T, 8>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((k_cd_dict_sweep<T, 16>), grid, block, 0, s, a);
    return hipGetLastError();
}

constexpr int CDL_RING = 64;        // device ring of per-iteration violation pairs

template <typename T> struct CdLearnWs {
    char* cd;               // the activation half's workspace (cd_workspace_bytes)
    size_t cd_bytes;
    T *Xt, *Ht, *partP, *partG, *G, *P, *Gb, *hess;
    double *dpart, *ring;
    size_t bytes;
};

// slabs of one contraction: S ranges of two slabs each, the last range's second slab cut to the one row that is written
size_t cdl_part_elems(int rows, int S, int ld) { return (size_t)(2 * S - 1) * learn_bin_tiles(rows) * 16 * ld + ld; }

template <typename T> CdLearnWs<T> carve_cd_learn(void* ws, int M, int R, int T_, int S) {
    CdLearnWs<T> w;
    Carver c = Carver::rounded(ws);                // ws == NULL: sizes only
    const int Mk = round_up(M, 16), ld = round_up(R, 128), Rp = round_up(R, CD_B);
    const CdGeometry gr = cd_geometry(R);          // the dictionary sweep's lane geometry comes from R as k_cd_sweep's from M
    w.cd_bytes = cd_workspace_bytes(M, R, T_, 1, (int)sizeof(T));
    w.cd = c.take<char>(w.cd_bytes);
    w.Xt = c.take<T>((size_t)T_ * Mk);
    w.Ht = c.take<T>((size_t)T_ * ld);
    w.partP = c.take<T>(cdl_part_elems(M, S, ld));
    w.partG = c.take<T>(cdl_part_elems(R, S, ld));
    w.G = c.take<T>((size_t)Rp * ld);
    w.P = c.take<T>((size_t)M * ld);
    w.Gb = c.take<T>((size_t)Rp * CD_B);
    w.hess = c.take<T>(Rp);
    w.dpart = c.take<double>((M + gr.F - 1) / gr.F);
    w.ring = c.take<double>(CDL_RING * 2);
    w.bytes = c.bytes();
    return w;
}

// S frame ranges for the two contractions over the frames (learn_splits, or what the caller forces)
size_t cd_learn_workspace_bytes(int M, int R, int T_, int S, int esize) {
    if (M < 1 || M > CD_MAX_M || R < 1 || R > CD_LEARN_MAX_R || T_ < 1 || S < 1 || S > LEARN_MAX_SPLITS) return 0;
    if (esize == 8) return carve_cd_learn<double>(nullptr, M, R, T_, S).bytes + 256;
    if (esize == 4) return carve_cd_learn<float>(nullptr, M, R, T_, S).bytes + 256;
    return 0;
}

// arguments already validated by evc_cd_learn; returns ST_OK, ST_WORKSPACE or a hipError_t
template <typename T>
int cd_learn(const T* X, int ldx, T* W, int ldw, T* H, int ldh, int M, int R, int T_, const evc_cd_learn_opts& o, int S,
             void* ws, size_t ws_bytes, int* n_iter_out, double* violation_out, hipStream_t s) {
    const CdLearnWs<T> w = carve_cd_learn<T>(ws, M, R, T_, S);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    const bool both = o.update == EVC_CDL_BOTH;
    const int Mk = round_up(M, 16), ld = round_up(R, 128), Rp = round_up(R, CD_B);
    const CdGeometry gr = cd_geometry(R);
    for (int i = 0; violation_out && i < 2 * o.max_iter; ++i) violation_out[i] = __builtin_nan("");
    if (n_iter_out) *n_iter_out = 0;
    if (o.max_iter == 0) return 0;

    CdArgs<T> a{};
    if (both) {
        const int st = cd_setup<T>(H, ldh, M, R, T_, nullptr, 1, fm, 1, 0.0, o.l1_h, o.l2_h, w.cd, w.cd_bytes, s, &a);
        if (st != 0) return st;
    }
    CdDictArgs<T> d;
    d.G = w.G; d.P = w.P; d.Gb = w.Gb; d.hess = w.hess; d.W = W;
    d.ws_m = fm ? 1 : ldw; d.ws_r = fm ? ldw : 1;
    d.part = w.dpart; d.ld = ld; d.M = M; d.R = R; d.Rp = Rp; d.L = gr.L; d.rpl = gr.mpl;
    const int n_waves = (M + gr.F - 1) / gr.F;
    const long slabP = (long)learn_bin_tiles(M) * 16 * ld, slabG = (long)learn_bin_tiles(R) * 16 * ld;

    HIP_TRY(copy2d<T>(X, ldx, T_, M, fm ? 0 : 1, w.Xt, Mk, T_, Mk, 0, s));
    if (!both) HIP_TRY(copy2d<T>(H, ldh, T_, R, fm ? 0 : 1, w.Ht, ld, T_, ld, 0, s));
    // only a call that wants neither the stop rule nor any figure back is a pure enqueue
    const bool sync = o.tol > 0.0 || n_iter_out || violation_out;
    if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
    int n_iter = 0;
    double vinit = 0.0;
    for (int it = 1; it <= o.max_iter; ++it) {
        if (both) {
            // activations: one sweep from the current H on the current W (the residual h W^T - x is formed afresh)
            const int st = cd_refresh<T>(a, W, ldw, X, ldx, 1, o.l2_h, s);
            if (st != 0) return st;
            HIP_TRY(launch_sweep<T>(a, 1, s));
            HIP_TRY(copy2d<T>(H, ldh, T_, R, fm ? 0 : 1, w.Ht, ld, T_, ld, 0, s));
        }
        // dictionary: the two contractions over the frames, their sums, the row sweeps
        HIP_TRY(dict_grad_kl<T>(w.Xt, Mk, w.Ht, ld, M, T_, S, w.partP, s));
        HIP_TRY(dict_grad_kl<T>(w.Ht, ld, w.Ht, ld, R, T_, S, w.partG, s));
        {
            const long n = (long)(Rp + M) * ld;
            hipLaunchKernelGGL(k_cdl_finish<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w.partG, slabG, w.partP,
                               slabP, S, ld, M, R, Rp, (T)o.l1_w, (T)o.l2_w, w.G, w.P, w.Gb, w.hess);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(launch_dict_sweep<T>(d, s));
        n_iter = it;
        if (!sync) continue;
        double* slot = w.ring + (size_t)(it % CDL_RING) * 2;
        hipLaunchKernelGGL(k_cdl_viol, dim3(1), dim3(256), 0, s, both ? a.part + a.n_tiles : nullptr, both ? a.n_tiles : 0,
                           w.dpart, n_waves, slot);
        HIP_TRY(hipGetLastError());
        double v[2];
        HIP_TRY(hipMemcpyAsync(v, slot, sizeof(v), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (violation_out) {
            violation_out[2 * (it - 1)] = v[0];
            violation_out[2 * (it - 1) + 1] = v[1];
        }
        const double viol = v[0] + v[1];
        if (it == 1) vinit = viol;
        if (vinit == 0.0 || viol / vinit <= o.tol) break;      // _nmf.py:513-519; the stopping iteration's updates stay
    }
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    if (n_iter_out) *n_iter_out = n_iter;
    return 0;
}

bool cd_learn_sizes_ok(int M, int R, int T, int dtype) {
    return M >= 1 && R >= 1 && T >= 1 && M <= CD_MAX_M && R <= CD_LEARN_MAX_R && (dtype == EVC_F64 || dtype == EVC_F32);
}

}  // namespace

}  // namespace evc

using namespace evc;

extern "C" {

size_t evc_cd_workspace_bytes(int M, int N, int T, int n_utt, int dtype) {
    if (dtype != EVC_F64 && dtype != EVC_F32) return 0;
    return cd_workspace_bytes(M, N, T, n_utt, dtype == EVC_F64 ? 8 : 4);
}

int evc_cd_solve(const void* A, int lda, const void* X, int ldx, void* H, int ldh, int M, int N, int T,
                 const int* utt_offsets, int n_utt, const evc_cd_opts* opts, void* workspace, size_t workspace_bytes,
                 int* n_iter_out, double* violation_out, evc_stream_t stream) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_cd_opts)) return ST_BADARG;
    const evc_cd_opts& o = *opts;
    HIP_TRY(solve_args_ok(M, N, T, n_utt, o.dtype, o.layout, A, workspace, lda, ldx, ldh, utt_offsets));
    if (o.max_iter < 0 || o.reserved != 0 || !X || !H) return ST_BADARG;
    if (o.init_mode != EVC_INIT_SKLEARN && o.init_mode != EVC_INIT_GIVEN) return ST_BADARG;
    if (!(o.tol >= 0.0) || !(o.l1 >= 0.0) || !(o.l2 >= 0.0)) return ST_BADARG;
    if (M > CD_MAX_M) return ST_UNSUPPORTED;
    if (workspace_bytes < evc_cd_workspace_bytes(M, N, T, n_utt, o.dtype)) return ST_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (o.dtype == EVC_F64)
        return cd_solve<double>(static_cast<const double*>(A), lda, static_cast<const double*>(X), ldx,
                                static_cast<double*>(H), ldh, M, N, T, utt_offsets, n_utt, o, workspace,
                                workspace_bytes, n_iter_out, violation_out, s, nullptr);
    return cd_solve<float>(static_cast<const float*>(A), lda, static_cast<const float*>(X), ldx, static_cast<float*>(H),
                           ldh, M, N, T, utt_offsets, n_utt, o, workspace, workspace_bytes, n_iter_out, violation_out, s,
                           nullptr);
}

int evc_cd_learn_splits(int M, int R, int T) {
    return cd_learn_sizes_ok(M, R, T, EVC_F64) ? learn_splits(M, R, T) : 0;
}

size_t evc_cd_learn_workspace_bytes(int M, int R, int T, int dtype) {
    if (!cd_learn_sizes_ok(M, R, T, dtype)) return 0;
    return cd_learn_workspace_bytes(M, R, T, learn_splits(M, R, T), dtype == EVC_F64 ? 8 : 4);
}

int evc_cd_learn(const void* X, int ldx, void* W, int ldw, void* H, int ldh, int M, int R, int T,
                 const evc_cd_learn_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out,
                 double* violation_out, evc_stream_t stream) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_cd_learn_opts)) return ST_BADARG;
    const evc_cd_learn_opts& o = *opts;
    int forced;
    HIP_TRY(learn_args_ok(M, R, T, o.dtype, o.layout, X, W, H, workspace, ldx, ldw, ldh, o.reserved, 0xff00, &forced));
    if (o.max_iter < 0 || (o.update != EVC_CDL_BOTH && o.update != EVC_CDL_DICT_ONLY)) return ST_BADARG;
    if (!(o.tol >= 0.0) || !(o.l1_h >= 0.0) || !(o.l2_h >= 0.0) || !(o.l1_w >= 0.0) || !(o.l2_w >= 0.0)) return ST_BADARG;
    if (M > CD_MAX_M || R > CD_LEARN_MAX_R) return ST_UNSUPPORTED;
    const int S = forced ? forced : learn_splits(M, R, T);
    if (workspace_bytes < cd_learn_workspace_bytes(M, R, T, S, o.dtype == EVC_F64 ? 8 : 4)) return ST_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (o.dtype == EVC_F64)
        return cd_learn<double>(static_cast<const double*>(X), ldx, static_cast<double*>(W), ldw, static_cast<double*>(H),
                                ldh, M, R, T, o, S, workspace, workspace_bytes, n_iter_out, violation_out, s);
    return cd_learn<float>(static_cast<const float*>(X), ldx, static_cast<float*>(W), ldw, static_cast<float*>(H), ldh, M, R,
                           T, o, S, workspace, workspace_bytes, n_iter_out, violation_out, s);
}

}  // extern "C"
