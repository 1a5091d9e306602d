// evc_deconv_kernels.h - the kernels of the multi-frame activation half, as evc_deconv.hip describes them
// in its head: k_deconv_v, k_deconv_update, k_deconv_check, k_deconv_pack_dict, k_deconv_synth and deconv_form_v.  Two
// translation units include this file, evc_deconv.hip (evc_deconv_solve, evc_deconv_synthesize) and evc_deconv_learn.hip
// (evc_deconv_learn, whose activation half is these kernels on the current dictionary), each into an unnamed namespace of
// its own: both get the same device code from the same text.
#pragma once
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

}  // namespace

}  // namespace evc

