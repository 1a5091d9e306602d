// evc_deconv.hip - evc_deconv_solve and evc_deconv_synthesize: the activation solve with multi-frame exemplars (non-negative
// spectrogram deconvolution: an exemplar is a segment of `taps` consecutive aligned frames and one activation places the whole
// segment) and the synthesis from the parallel target segments.  DESIGN.md §5.14; the statement is in include/evc.h.
//
// Per iteration, with L = taps, utterance u's frames 0 .. T_u - 1 and EPS = 2^-23 in both element types:
//   V[:, t] = sum_{tau <= min(L-1, t)} A_tau H[:, t - tau]
//   Qn = X (Frobenius) | X / max(V, EPS) (KL);  Qd = V (Frobenius) | 1 (KL);  both 0 beyond the utterance's end
//   Num | Den [n, t] = sum_tau A_tau[:, n] . Qn | Qd [:, t + tau];  Den += l1 + l2 h, 0 -> EPS;  h <- h * (Num / Den)
// The time shift sits in both contractions, so no kernel of evc_beta.hip can express it (k_beta_sweep updates H in place one
// frame tile at a time and cannot read the neighbouring tiles).  Two launches per iteration over evc_beta_common.h's tiles of
// 16 frames (an utterance starts a tile of its own):
//   k_deconv_v<T>       a workgroup of four wavefronts owns a tile and forms V on the matrix cores (16x16x4) as beta_form_v
//                       does, with an outer tap loop and the frame index shifted back by the tap; frames before the
//                       utterance's start contribute 0.  It writes the packed images Qn and Qd [tile][MP][16] with exact zeros
//                       in the padding slots - that is what truncates Num and Den at the utterance's end - and, on a check,
//                       every frame's share of the error in float64.
//   k_deconv_update<T>  a workgroup loads its tile's images and the next tile's of the same utterance (zeros if there is
//                       none) into LDS: 32 frame columns, which is why taps <= 16; 131 072 bytes at MP = 256 in float64.  Per
//                       exemplar tile of 16 it accumulates Num | Den over the taps and the bins with the B operand read at
//                       column f + tau, then updates H in place.  The columns of the odd rows are rotated by 16 so that the
//                       two rows a group of 32 lanes reads in one LDS cycle fall into different banks at the row stride of 32.
// V passes through memory (M x T, small next to H): no workgroup reads activations another one writes in the same launch.
// The KL denominator is constant over the iterations; it is formed by the same contraction over an image of ones, which
// keeps one code path and the truncation for free at the price of the matrix work column sums per tail length would save.
// A check is k_deconv_v once more (its images serve the next iteration, so that one skips its own k_deconv_v) and
// k_deconv_check, k_beta_check's fixed-order per-utterance sum and stop rule.  The sums run in a fixed order - taps ascending,
// then exemplar chunks per wavefront, the four wavefronts in order - that depends on the tile's position in its utterance
// only: the same call gives the same bits, and a batch gives bitwise what one call per utterance gives.
//
// The tile table, the packed X, the start values, the stop state and the trace are evc_beta_solve's host steps (beta_begin,
// beta_start; evc_beta_common.h) on their own part of the workspace.
// evc_deconv_synthesize is the first contraction alone, reading B and H and writing Y in the caller's memory: one launch per
// utterance, a workgroup per (frame tile, group of 8 bin tiles).
#include "evc_deconv_plan.h"

namespace evc {

namespace {

template <typename T> struct DcVec4;
template <> struct DcVec4<double> { typedef f64x4 type; };
template <> struct DcVec4<float> { typedef f32x4 type; };

template <typename T> struct DcArgs {
    const T* Ap1;           // [taps][NP][MP] per tap: exemplars as rows, bins contiguous, zero-padded
    const T* Ap3;           // [taps][NP][MP] the same with the bins of every chunk of 16 permuted: slot 4 g + s = bin 4 s + g
    const T* Xp;            // [n_tiles][MP][16] frames of a tile, zero-padded
    T *Qn, *Qd;             // [n_tiles][MP][16] what k_deconv_v leaves for k_deconv_update
    T* H;
    long hs_t, hs_n;        // H(n, t) = H[t * hs_t + n * hs_n]
    const int4* tiles;      // {utterance, first frame, frames, first tile of the utterance}
    const int* stop;        // [n_utt] 0: running; else the iteration the utterance stopped at
    double* errf;           // [n_tiles * 16] per-frame share of the error
    int M, MP, N, NP, taps, kl, n_tiles;
    T l1, l2;
};

// One group of nb <= BT_GT bin tiles from bin tile bt0 on: Vs[(j * 16 + bin)][frame] = sum_tau sum_n D_tau(bin, n) H(n, t - tau)
// for the tile's 16 frame slots (0 in the padding), t - tau not before the utterance's start (`back` frames of the utterance
// lie before the tile); ends with a barrier.  PACKED: D is a [taps][NP][MP] image (no bounds); else D_tau(bin, n) =
// D[tau * ds_tap + bin * ds_m + n * ds_n] in the caller's memory, bin < Md and n < N.
template <typename T, bool PACKED>
__device__ __forceinline__ void deconv_form_v(const T* __restrict__ D, long ds_tap, long ds_m, long ds_n, int Md,
                                              const T* __restrict__ H, long hs_t, long hs_n, int N, int taps, int frame0,
                                              int frames, int back, int bt0, int nb, T* __restrict__ Vs) {
    typedef typename Mma<T>::acc_t acc_t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = lane & 15, g = lane >> 4;
    const int NC = (N + 15) / 16;
    acc_t acc[BT_GT];
#pragma unroll
    for (int j = 0; j < BT_GT; ++j) acc[j] = acc_t{0, 0, 0, 0};
#pragma unroll 1
    for (int tau = 0; tau < taps; ++tau) {
        const bool fvalid = f < frames && tau <= back + f;
        const T* Hf = H + (long)(frame0 + (fvalid ? f - tau : 0)) * hs_t;
        const T* Dt = D + (long)tau * ds_tap;
#pragma unroll 1
        for (int c = wave; c < NC; c += BT_WAVES) {
            const int n0 = c * 16 + g * 4;
            T h[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {          // clamped address, then select
                const int n = n0 + s;
                const T v = Hf[(long)(n < N ? n : N - 1) * hs_n];
                h[s] = (fvalid && n < N) ? v : T(0);
            }
#pragma unroll
            for (int j = 0; j < BT_GT; ++j)
                if (j < nb) {
                    const int bin = (bt0 + j) * 16 + f;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        T av;
                        if constexpr (PACKED) {
                            av = Dt[(long)(n0 + s) * ds_n + bin];
                        } else {
                            const int n = n0 + s;
                            const T v = Dt[(long)(bin < Md ? bin : Md - 1) * ds_m + (long)(n < N ? n : N - 1) * ds_n];
                            av = (bin < Md && n < N) ? v : T(0);
                        }
                        acc[j] = Mma<T>::mma(av, h[s], acc[j]);
                    }
                }
        }
    }
    // the four partial sums, added in wavefront order
#pragma unroll 1
    for (int w = 0; w < BT_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int j = 0; j < BT_GT; ++j)
                if (j < nb) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int idx = (j * 16 + Mma<T>::row(lane, r)) * BT_F + f;
                        Vs[idx] = w ? Vs[idx] + acc[j][r] : acc[j][r];
                    }
                }
        }
        __syncthreads();
    }
}

// V of the tile, then the images Qn | Qd; want_err: also errf[slot] = the frame's share of the error (k_beta_err's sums for
// beta = 2 and beta = 1)
template <typename T>
__global__ __launch_bounds__(BT_THREADS) void k_deconv_v(DcArgs<T> a, int want_err) {
    extern __shared__ __attribute__((aligned(16))) unsigned char deconv_lds[];
    const int tile = blockIdx.x;
    const int4 tl = a.tiles[tile];
    if (a.stop[tl.x] != 0) return;
    T* Vs = reinterpret_cast<T*>(deconv_lds);
    double* red = reinterpret_cast<double*>(deconv_lds + (size_t)a.MP * BT_F * sizeof(T));      // [16 parts][16 frames]
    const int back = tl.y - a.tiles[tl.w].y;
    const int MT = a.MP / 16;
#pragma unroll 1
    for (int t0 = 0; t0 < MT; t0 += BT_GT)
        deconv_form_v<T, true>(a.Ap1, (long)a.NP * a.MP, 1, a.MP, a.MP, a.H, a.hs_t, a.hs_n, a.N, a.taps, tl.y, tl.z, back, t0,
                               MT - t0 < BT_GT ? MT - t0 : BT_GT, Vs + (long)t0 * 16 * BT_F);
    const T* Xt = a.Xp + (long)tile * a.MP * BT_F;
    T* qn = a.Qn + (long)tile * a.MP * BT_F;
    T* qd = a.Qd + (long)tile * a.MP * BT_F;
    const T eps = (T)BETA_EPS;
    for (int e = threadIdx.x; e < a.MP * BT_F; e += BT_THREADS) {
        T n = T(0), d = T(0);
        if ((e >> 4) < a.M && (e & 15) < tl.z) {
            const T v = Vs[e], x = Xt[e];
            if (a.kl) {
                n = x / (v < eps ? eps : v);
                d = T(1);
            } else {
                n = x;
                d = v;
            }
        }
        qn[e] = n;
        qd[e] = d;
    }
    if (!want_err) return;
    const int f = threadIdx.x & 15, part = threadIdx.x >> 4;
    double s0 = 0.0;
    for (int m = part; m < a.M; m += 16) {
        const double x = (double)Xt[m * BT_F + f], v = (double)Vs[m * BT_F + f];
        if (a.kl) {
            const double vv = v < BETA_EPS ? BETA_EPS : v;
            s0 += v;
            if (x > BETA_EPS) s0 += x * log(x / vv) - x;
        } else {
            s0 += (x - v) * (x - v);
        }
    }
    red[part * 16 + f] = s0;
    __syncthreads();
    if (threadIdx.x < 16) {
        double t0 = 0.0;
        for (int p = 0; p < 16; ++p) t0 += red[p * 16 + f];
        a.errf[(long)tile * BT_F + f] = f < tl.z ? (a.kl ? t0 : 0.5 * t0) : 0.0;
    }
}

// LDS column of frame column `col` in a row of parity `odd`: the odd rows are rotated by half a row
__device__ __forceinline__ int dc_col(int col, int odd) { return (col + (odd << 4)) & (DC_COLS - 1); }

template <typename T>
__global__ __launch_bounds__(BT_THREADS) void k_deconv_update(DcArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char deconv_lds[];
    typedef typename Mma<T>::acc_t acc_t;
    typedef typename DcVec4<T>::type vec_t;
    const int tile = blockIdx.x;
    const int4 tl = a.tiles[tile];
    if (a.stop[tl.x] != 0) return;
    T* Qn = reinterpret_cast<T*>(deconv_lds);
    T* Qd = Qn + a.MP * DC_COLS;
    // this tile's images and the next tile's of the same utterance (tiles of an utterance are consecutive)
    {
        const bool has_next = tile + 1 < a.n_tiles && a.tiles[tile + 1].x == tl.x;
        const int img = a.MP * BT_F;
        const T* gn = a.Qn + (long)tile * img;
        const T* gd = a.Qd + (long)tile * img;
        for (int e = threadIdx.x; e < 2 * img; e += BT_THREADS) {
            const int second = e >= img ? 1 : 0, rem = e - second * img;
            const int row = rem >> 4, col = (rem & 15) + second * BT_F;
            T n = T(0), d = T(0);
            if (!second || has_next) {
                n = gn[e];
                d = gd[e];
            }
            const int idx = row * DC_COLS + dc_col(col, row & 1);
            Qn[idx] = n;
            Qd[idx] = d;
        }
    }
    __syncthreads();
    // Num | Den of an exemplar tile over the taps and the bins, then the update
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = lane & 15, g = lane >> 4;
    const bool fvalid = f < tl.z;
    T* Hf = a.H + (long)(tl.y + (fvalid ? f : 0)) * a.hs_t;
    const int NT = a.NP / 16, MC = a.MP / 16;
    const long tap_img = (long)a.NP * a.MP;
    const T eps = (T)BETA_EPS;
#pragma unroll 1
    for (int nt = wave; nt < NT; nt += BT_WAVES) {
        acc_t num = acc_t{0, 0, 0, 0}, den = acc_t{0, 0, 0, 0};
#pragma unroll 1
        for (int tau = 0; tau < a.taps; ++tau) {
            const T* Ar = a.Ap3 + tau * tap_img + (long)(nt * 16 + f) * a.MP + g * 4;
            const int col = dc_col(f + tau, g & 1);         // the rows a lane reads have its lane group's parity
            for (int c = 0; c < MC; ++c) {
                const vec_t av = *reinterpret_cast<const vec_t*>(Ar + c * 16);
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int row = c * 16 + s * 4 + g;
                    num = Mma<T>::mma(av[s], Qn[row * DC_COLS + col], num);
                    den = Mma<T>::mma(av[s], Qd[row * DC_COLS + col], den);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = nt * 16 + Mma<T>::row(lane, r);
            if (fvalid && n < a.N) {
                T* hp = Hf + (long)n * a.hs_n;
                const T h = *hp;
                T d = den[r] + a.l1;
                d = d + a.l2 * h;
                d = d == T(0) ? eps : d;
                *hp = h * (num[r] / d);
            }
        }
    }
}

// one block per utterance: err = sqrt(2 max(sum of the shares, 0)) in a fixed order; check c (0: the start); k_beta_check's
// sum and rule
__global__ __launch_bounds__(256) void k_deconv_check(const double* __restrict__ errf, const int* __restrict__ utt_tile0,
                                                      int* stop, double* einit, double* eprev, double* trace, int n_slots,
                                                      int c, int check_every, int stop_rule, double tol) {
    __shared__ double red[256];
    const int u = blockIdx.x;
    const long i0 = (long)utt_tile0[u] * BT_F, i1 = (long)utt_tile0[u + 1] * BT_F;
    if (stop[u] != 0 || i0 == i1) return;       // uniform per block
    double acc = 0.0;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) acc += errf[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double err = sqrt(2.0 * fmax(red[0], 0.0));
    trace[(long)u * n_slots + c] = err;
    if (c == 0) {
        einit[u] = err;
        eprev[u] = err;
        return;
    }
    if (stop_rule == EVC_STOP_SKLEARN && (eprev[u] - err) / einit[u] < tol) stop[u] = c * check_every;
    else eprev[u] = err;
}

// the two packed images of every tap (k_beta_pack_dict's, per tap)
template <typename T>
__global__ void k_deconv_pack_dict(const T* __restrict__ A, int lda, long tap_stride, int fm, int M, int N, int NP, int MP,
                                   int taps, T* __restrict__ Ap1, T* __restrict__ Ap3) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long img = (long)NP * MP;
    if (i >= img * taps) return;
    const T* At = A + (i / img) * tap_stride;
    const long k = i % img;
    const int n = (int)(k / MP), p = (int)(k % MP);
    const int m3 = (p & ~15) + (p & 3) * 4 + ((p >> 2) & 3);       // slot 4 g + s holds bin 4 s + g of its chunk
    T v1 = T(0), v3 = T(0);
    if (n < N) {
        if (p < M) v1 = fm ? At[(long)n * lda + p] : At[(long)p * lda + n];
        if (m3 < M) v3 = fm ? At[(long)n * lda + m3] : At[(long)m3 * lda + n];
    }
    Ap1[i] = v1;
    Ap3[i] = v3;
}

// Y(bin, t) = sum_tau B_tau(bin, :) . H(:, t - tau) for the frames [f0, f0 + Tu) of one utterance: blockIdx.x the frame
// tile, blockIdx.y the group of BT_GT bin tiles
template <typename T>
__global__ __launch_bounds__(BT_THREADS) void k_deconv_synth(const T* __restrict__ B, long bs_tap, long bs_m, long bs_n, int Mb,
                                                             int N, const T* __restrict__ H, long hs_t, long hs_n,
                                                             T* __restrict__ Y, long ys_t, long ys_m, int taps, int f0, int Tu) {
    __shared__ __attribute__((aligned(16))) T Vs[BT_GT * 16 * BT_F];
    const int back = blockIdx.x * BT_F;
    const int frames = Tu - back < BT_F ? Tu - back : BT_F;
    const int MT = (Mb + 15) / 16, bt0 = blockIdx.y * BT_GT;
    const int nb = MT - bt0 < BT_GT ? MT - bt0 : BT_GT;
    deconv_form_v<T, false>(B, bs_tap, bs_m, bs_n, Mb, H, hs_t, hs_n, N, taps, f0 + back, frames, back, bt0, nb, Vs);
    for (int e = threadIdx.x; e < nb * 16 * BT_F; e += BT_THREADS) {
        const int bin = bt0 * 16 + (e >> 4), f = e & 15;
        if (bin < Mb && f < frames) Y[(long)(f0 + back + f) * ys_t + (long)bin * ys_m] = Vs[e];
    }
}

unsigned dc_blocks_of(long n) { return (unsigned)((n + 255) / 256); }

template <typename T> size_t dc_lds_v(int MP) { return (size_t)MP * BT_F * sizeof(T) + 256 * sizeof(double); }
template <typename T> size_t dc_lds_update(int MP) { return (size_t)2 * MP * DC_COLS * sizeof(T); }

// arguments already validated by evc_deconv_solve; returns 0, -2 or a hipError_t
template <typename T>
int deconv_solve(const T* A, int lda, long tap_stride, const T* X, int ldx, T* H, int ldh, int M, int N, int T_,
                 const int* utt_offsets, int n_utt, const evc_deconv_opts& o, void* ws, size_t ws_bytes, int* n_iter_out,
                 double* err_out, hipStream_t s) {
    const int n_slots = 1 + (o.check_every > 0 ? o.iters / o.check_every : 0);
    const DcWs w = carve_deconv(ws, M, N, T_, n_utt, o.taps, o.dtype);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    BetaCtx<T> c;
    int st = beta_begin<T>(c, X, ldx, H, ldh, M, N, T_, utt_offsets, n_utt, o.layout, 2.0, o.l1, o.l2, 0.0, n_slots, w.beta_ws,
                           w.beta_bytes, s);
    if (st != 0) return st;
    const int n_tiles = c.n_tiles;
    DcArgs<T> a;
    a.Ap1 = reinterpret_cast<T*>(w.Ap1); a.Ap3 = reinterpret_cast<T*>(w.Ap3); a.Xp = c.w.Xp;
    a.Qn = reinterpret_cast<T*>(w.Qn); a.Qd = reinterpret_cast<T*>(w.Qd);
    a.H = H; a.hs_t = c.a.hs_t; a.hs_n = c.a.hs_n;
    a.tiles = c.w.tiles; a.stop = c.w.stop; a.errf = c.w.errf;
    a.M = M; a.MP = c.a.MP; a.N = N; a.NP = c.a.NP; a.taps = o.taps; a.kl = o.loss == EVC_LOSS_KL ? 1 : 0; a.n_tiles = n_tiles;
    a.l1 = (T)o.l1; a.l2 = (T)o.l2;
    if (n_tiles > 0) {
        hipLaunchKernelGGL(k_deconv_pack_dict<T>, dim3(dc_blocks_of((long)o.taps * a.NP * a.MP)), dim3(256), 0, s, A, lda,
                           tap_stride, c.fm, M, N, a.NP, a.MP, o.taps, reinterpret_cast<T*>(w.Ap1), reinterpret_cast<T*>(w.Ap3));
        HIP_TRY(hipGetLastError());
        // per function and process-wide: always the limit of DC_MAX_M, so that concurrent calls never shrink it under one another
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_deconv_update<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)dc_lds_update<T>(DC_MAX_M)));
    }
    if ((st = beta_start<T>(c, o.init_mode, o.init_value, s)) != 0) return st;
    auto form_v = [&](int want_err) -> int {
        hipLaunchKernelGGL(k_deconv_v<T>, dim3(n_tiles), dim3(BT_THREADS), dc_lds_v<T>(a.MP), s, a, want_err);
        return (int)hipGetLastError();
    };
    auto check = [&](int chk) -> int {
        HIP_TRY(form_v(1));
        hipLaunchKernelGGL(k_deconv_check, dim3(n_utt), dim3(256), 0, s, c.w.errf, c.w.utt_tile0, c.w.stop, c.w.einit, c.w.eprev,
                           c.w.trace, n_slots, chk, o.check_every, o.stop_rule, o.tol);
        return (int)hipGetLastError();
    };
    const bool checks = o.check_every > 0 && n_tiles > 0;
    bool v_fresh = false;       // the images of the current H are in place (a check has just formed them)
    if (checks) {
        HIP_TRY(check(0));
        v_fresh = true;
    }
    if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
    for (int it = 1; n_tiles > 0 && it <= o.iters; ++it) {
        if (!v_fresh) HIP_TRY(form_v(0));
        hipLaunchKernelGGL(k_deconv_update<T>, dim3(n_tiles), dim3(BT_THREADS), dc_lds_update<T>(a.MP), s, a);
        HIP_TRY(hipGetLastError());
        v_fresh = false;
        if (checks && it % o.check_every == 0) {
            HIP_TRY(check(it / o.check_every));
            v_fresh = true;
        }
    }
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    if (n_iter_out || err_out) {
        int* ni_h = static_cast<int*>(malloc(sizeof(int) * n_utt));
        if (!ni_h) return (int)hipErrorOutOfMemory;
        hipError_t e = hipMemcpyAsync(ni_h, c.w.stop, sizeof(int) * n_utt, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && err_out)
            e = hipMemcpyAsync(err_out, c.w.trace, sizeof(double) * n_utt * n_slots, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        for (int u = 0; e == hipSuccess && n_iter_out && u < n_utt; ++u) n_iter_out[u] = ni_h[u] ? ni_h[u] : o.iters;
        free(ni_h);
        HIP_TRY(e);
    }
    return 0;
}

template <typename T>
int deconv_synthesize(const T* B, int ldb, long tap_stride, const T* H, int ldh, T* Y, int ldy, int Mb, int N, int T_,
                      const int* utt_offsets, int n_utt, int taps, int layout, hipStream_t s) {
    const bool fm = layout == EVC_FRAME_MAJOR;
    const int groups = ((Mb + 15) / 16 + BT_GT - 1) / BT_GT;
    for (int u = 0; u < n_utt; ++u) {
        const int f0 = utt_offsets ? utt_offsets[u] : 0;
        const int tu = utt_offsets ? utt_offsets[u + 1] - f0 : T_;
        if (tu == 0) continue;
        hipLaunchKernelGGL(k_deconv_synth<T>, dim3((tu + BT_F - 1) / BT_F, groups), dim3(BT_THREADS), 0, s, B, tap_stride,
                           fm ? 1L : (long)ldb, fm ? (long)ldb : 1L, Mb, N, H, fm ? (long)ldh : 1L, fm ? 1L : (long)ldh, Y,
                           fm ? (long)ldy : 1L, fm ? 1L : (long)ldy, taps, f0, tu);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace

}  // namespace evc

extern "C" {

size_t evc_deconv_workspace_bytes(int M, int N, int T, int n_utt, int taps, int dtype) {
    return evc::deconv_workspace_bytes(M, N, T, n_utt, taps, dtype);
}

int evc_deconv_solve(const void* A, int lda, long tap_stride, const void* X, int ldx, void* H, int ldh, int M, int N, int T,
                     const int* utt_offsets, int n_utt, const evc_deconv_opts* opts, void* workspace, size_t workspace_bytes,
                     int* n_iter_out, double* err_out, evc_stream_t stream) {
    using namespace evc;
    HIP_TRY(deconv_args_check(A, lda, tap_stride, X, ldx, H, ldh, M, N, T, utt_offsets, n_utt, opts, workspace, workspace_bytes));
    const evc_deconv_opts& o = *opts;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (o.dtype == EVC_F64)
        return deconv_solve<double>(static_cast<const double*>(A), lda, tap_stride, static_cast<const double*>(X), ldx,
                                    static_cast<double*>(H), ldh, M, N, T, utt_offsets, n_utt, o, workspace, workspace_bytes,
                                    n_iter_out, err_out, s);
    return deconv_solve<float>(static_cast<const float*>(A), lda, tap_stride, static_cast<const float*>(X), ldx,
                               static_cast<float*>(H), ldh, M, N, T, utt_offsets, n_utt, o, workspace, workspace_bytes,
                               n_iter_out, err_out, s);
}

int evc_deconv_synthesize(const void* B, int ldb, long tap_stride, const void* H, int ldh, void* Y, int ldy, int Mb, int N, int T,
                          const int* utt_offsets, int n_utt, int taps, int layout, int dtype, evc_stream_t stream) {
    using namespace evc;
    HIP_TRY(deconv_synth_args_check(B, ldb, tap_stride, H, ldh, Y, ldy, Mb, N, T, utt_offsets, n_utt, taps, layout, dtype));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == EVC_F64)
        return deconv_synthesize<double>(static_cast<const double*>(B), ldb, tap_stride, static_cast<const double*>(H), ldh,
                                         static_cast<double*>(Y), ldy, Mb, N, T, utt_offsets, n_utt, taps, layout, s);
    return deconv_synthesize<float>(static_cast<const float*>(B), ldb, tap_stride, static_cast<const float*>(H), ldh,
                                    static_cast<float*>(Y), ldy, Mb, N, T, utt_offsets, n_utt, taps, layout, s);
}

}  // extern "C"
