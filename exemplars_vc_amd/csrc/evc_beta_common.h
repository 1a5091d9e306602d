// Declarations shared by evc_beta.hip (evc_beta_solve), evc_beta_learn.hip (evc_beta_learn), evc_online.hip
// (evc_online_learn) and evc_transform.hip (evc_online_transform): the tile geometry, the power evaluation, the host steps of the activation half and the frame sums of
// the dictionary half.
#pragma once
#include "evc_internal.h"

namespace evc {

constexpr int BT_F = 16;            // frames per tile
constexpr int BT_WAVES = 4;
constexpr int BT_THREADS = 64 * BT_WAVES;
constexpr int BT_GT = 8;            // bin tiles per pass of phase 1 (accumulators held at once)
constexpr int BETA_MAX_M = 528;     // two LDS images of 528 x 16 float64: 135 168 of 163 840 bytes
constexpr int BETA_MAX_SLOTS = 4097;
constexpr int BETA_CHG_LDS = 4 * 2 * 16 * 8;    // the change variant of the sweep: [4 wavefronts][2][16 frames] float64 after Q1 | Q2
constexpr double BETA_EPS = 1.1920928955078125e-7;
constexpr double BETA_E64 = 2.220446049250313e-16;      // 2^-52, numpy's float64 epsilon (in both element types)
constexpr int BDG_MAX_R = 256;        // k_beta_dict_grad: 256 x 20 elements of W and 3 x 16 x 64 of partial sums, 64 KB of LDS in float64
constexpr int BDG_ROUTE_R = 64;       // the fused route is taken up to this R: measured, DESIGN.md §5.11
enum { ROUTE_AUTO = 0, ROUTE_FUSED = 1, ROUTE_UNFUSED = 2 };
enum { BETA_ERR_IS = 0, BETA_ERR_KL = 1, BETA_ERR_FROB = 2, BETA_ERR_GENERIC = 3 };

// x^e: e = k2 / 2 without pow when `general` is 0
struct PowSpec {
    double e;
    int k2;
    int general;
};

inline PowSpec pow_spec(double e) {
    PowSpec p;
    p.e = e;
    const double k = 2.0 * e;
    p.general = !(k >= -16.0 && k <= 16.0 && k == (double)(long)k);      // the range first: the cast is only defined inside it
    p.k2 = p.general ? 0 : (int)k;
    return p;
}

__device__ __forceinline__ double pow_t(double x, double e) { return pow(x, e); }
__device__ __forceinline__ float pow_t(float x, float e) { return powf(x, e); }

template <typename T>
__device__ __forceinline__ T pw(T x, const PowSpec& p) {
    if (p.general) return pow_t(x, (T)p.e);
    const int k = p.k2 < 0 ? -p.k2 : p.k2;
    T r = T(1), b = x;
    for (int n = k >> 1; n;) {
        if (n & 1) r *= b;
        n >>= 1;
        if (n) b *= b;
    }
    if (k & 1) r *= sqrt(x);
    return p.k2 < 0 ? T(1) / r : r;
}

template <typename T> struct BetaArgs {
    const T* Ap1;           // [NP][MP] exemplars as rows, bins contiguous, zero-padded
    const T* Ap3;           // [NP][MP] the same with the bins of every chunk of 16 permuted: slot 4 g + s = bin 4 s + g
    const T* Xp;            // [n_tiles][MP][16] frames of a tile, zero-padded
    T* H;
    long hs_t, hs_n;        // H(n, t) = H[t * hs_t + n * hs_n]
    const int4* tiles;      // {utterance, first frame, frames, first tile of the utterance: no beta kernel reads .w}
    const int* stop;        // [n_utt] 0: running; else the iteration the utterance stopped at
    double* errf;           // [n_tiles * 16] per-frame share of the divergence
    int M, MP, N, NP;
    int clamp_n, clamp_d;   // beta < 2, beta < 1
    int gamma_one, err_mode;
    PowSpec p1, p2, pg, pb; // beta - 2, beta - 1, gamma, beta
    T l1, l2;
    T flush;                // > 0: an updated activation below it is stored as 0 (evc_beta_learn, beta < 1); 0: off
    double beta;
    int tile0;              // workgroup 0's tile: 0, or the first tile of the one batch evc_online_learn launches over
    double* chg;            // [n_tiles * 16][2] per-frame shares of sum (h_new - h_old)^2 and sum h_new^2: written by the
                            // change variant of the sweep only (evc_online_transform); NULL elsewhere
};


template <typename T> struct BetaWs {
    T *Ap1, *Ap3, *Xp;
    double *errf, *h0, *einit, *eprev, *trace;
    int4* tiles;
    int *utt_tile0, *utt_frames, *stop;
    size_t bytes;
};

// one call's activation half: the kernel arguments, the carved workspace and the tile count
template <typename T> struct BetaCtx {
    BetaArgs<T> a;
    BetaWs<T> w;
    int n_tiles, n_utt, n_slots, fm;
    int utt0;               // first utterance of a call that runs over a range (evc_online_learn_fresh: one batch); else 0
};

// ----- device pieces of the factored sweep, shared by k_beta_sweep / k_beta_err (evc_beta.hip) and k_mum_sweep / k_mum_err
// (evc_mu_masked.hip); Args: BetaArgs<T> or MumArgs<T> (the fields H, hs_t, hs_n, Ap1, N, NP, MP) -----
template <typename T> struct Vec4;
template <> struct Vec4<double> { typedef f64x4 type; };
template <> struct Vec4<float> { typedef f32x4 type; };

// Vs[bin][frame] = (A H)[bin][frame] for the tile's 16 frame slots (0 in the padding); ends with a barrier
template <typename T, typename Args>
__device__ __forceinline__ void beta_form_v(const Args& a, const int4 tl, T* __restrict__ Vs) {
    typedef typename Mma<T>::acc_t acc_t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = lane & 15, g = lane >> 4;
    const bool fvalid = f < tl.z;
    const T* Hf = a.H + (long)(tl.y + (fvalid ? f : 0)) * a.hs_t;
    const int NC = a.NP / 16, MT = a.MP / 16;
#pragma unroll 1
    for (int t0 = 0; t0 < MT; t0 += BT_GT) {
        acc_t acc[BT_GT];
#pragma unroll
        for (int j = 0; j < BT_GT; ++j) acc[j] = acc_t{0, 0, 0, 0};
#pragma unroll 1
        for (int c = wave; c < NC; c += BT_WAVES) {
            const int n0 = c * 16 + g * 4;
            T h[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {          // clamped address, then select
                const int n = n0 + s;
                const T v = Hf[(long)(n < a.N ? n : a.N - 1) * a.hs_n];
                h[s] = (fvalid && n < a.N) ? v : T(0);
            }
            const T* Ab = a.Ap1 + (long)n0 * a.MP + t0 * 16 + f;
#pragma unroll
            for (int j = 0; j < BT_GT; ++j)
                if (t0 + j < MT) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) acc[j] = Mma<T>::mma(Ab[(long)s * a.MP + j * 16], h[s], acc[j]);
                }
        }
        // the four partial sums, added in wavefront order
#pragma unroll 1
        for (int w = 0; w < BT_WAVES; ++w) {
            if (wave == w) {
#pragma unroll
                for (int j = 0; j < BT_GT; ++j)
                    if (t0 + j < MT) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int idx = ((t0 + j) * 16 + Mma<T>::row(lane, r)) * BT_F + f;
                            Vs[idx] = w ? Vs[idx] + acc[j][r] : acc[j][r];
                        }
                    }
            }
            __syncthreads();
        }
    }
}

// gamma of the multiplicative update (sklearn _nmf.py:780-785)
inline double beta_gamma(double beta) { return beta < 1.0 ? 1.0 / (2.0 - beta) : beta > 2.0 ? 1.0 / (beta - 1.0) : 1.0; }

// ----- evc_beta.hip: the host steps of evc_beta_solve, in the order it takes them -----
size_t beta_workspace_bytes(int M, int N, int T_, int n_utt, int dtype);
// carves the workspace, stages the tile table, clears the stop state and the trace, packs X and fills the kernel
// arguments; returns 0, -2 or a hipError_t
template <typename T>
int beta_begin(BetaCtx<T>& c, const T* X, int ldx, T* H, int ldh, int M, int N, int T_, const int* utt_offsets, int n_utt,
               int layout, double beta, double l1, double l2, double flush, int n_slots, void* ws, size_t ws_bytes,
               hipStream_t s);
// the two packed images of the dictionary the sweeps stream (A addressed as in evc_beta_solve)
template <typename T> int beta_pack_dict(const BetaCtx<T>& c, const T* A, int lda, hipStream_t s);
// one multiplicative update of every running utterance's activations, in place
template <typename T> int beta_sweep(const BetaCtx<T>& c, hipStream_t s);
// check number `chk` (0: the start): every utterance's error into its trace slot, then the stop rule on the device
template <typename T>
int beta_check(const BetaCtx<T>& c, int chk, int check_every, int stop_rule, double tol, hipStream_t s);
// the read-back that ends a fixed-dictionary solve (evc_beta_solve, evc_online_transform, evc_deconv_solve): nothing when
// neither output is asked for (the call then stays asynchronous); else stop[] and `slots` trace values per utterance to the
// host (no trace copy when slots is 0), one synchronisation, and n_iter_out[u] = stop[u], or `iters` where u never stopped
template <typename T>
int beta_report(const BetaCtx<T>& c, int iters, int* n_iter_out, double* trace_out, int slots, hipStream_t s);
// its first half alone: every frame's share of the divergence into errf (evc_online_learn sums one batch's shares itself)
template <typename T> int beta_err(const BetaCtx<T>& c, hipStream_t s);
// the start of the activations: nothing for EVC_INIT_GIVEN, else every activation of utterance u at sqrt(mean(X_u) / N)
// (EVC_INIT_SKLEARN) or at init_value (EVC_INIT_CONST)
template <typename T> int beta_start(const BetaCtx<T>& c, int init_mode, double init_value, hipStream_t s);
// iteration `it` (1, 2, ...) of a solve that stops on the change of its activations (MiniBatchNMF._solve_W): the change
// variant of the sweep, which also leaves every frame's shares in c.a.chg, then per utterance ratio = ||H_new - H_old||_F /
// ||H_new||_F into trace slot it - 1 and, if tol > 0 and ratio <= tol, stop[u] = it - all on the device
template <typename T> int beta_sweep_change(const BetaCtx<T>& c, int it, double tol, hipStream_t s);
// the pieces evc_online_learn_fresh puts around that solve, over the range c describes (utterances [utt0, utt0 + n_utt), tiles
// [a.tile0, a.tile0 + n_tiles)): beta_h0 forms every utterance's start value sqrt(mean(X_u) / N) (once per call, over all
// utterances); beta_restart clears the range's stop words and, with `fill`, sets its columns of H to the start values; beta_flush
// stores 0 over every activation of the range below thr - a pass of its own after the solve, never BetaArgs.flush during it
template <typename T> int beta_h0(const BetaCtx<T>& c, hipStream_t s);
template <typename T> int beta_restart(const BetaCtx<T>& c, bool fill, hipStream_t s);
template <typename T> int beta_flush(const BetaCtx<T>& c, double thr, hipStream_t s);

// ----- evc_beta_learn.hip: the frame sums of the dictionary half, shared with evc_online_learn -----
// part[s][0 | 1][m][r] = Num | Den (before the penalties) of the dictionary update over the s-th of S contiguous ranges of
// the T_ frames given: Xt [>= T_][Mk], Ht [Tp][Np] and Am [Mj][Np] as make_dims pads them (frames as rows; Tp =
// frame_pad(T_)), Vt and Q2t [Tp][Mj] scratch of the unfused route.  fused: k_beta_dict_grad (R <= BDG_MAX_R), else the
// generic contraction, k_beta_dict_q and dict_grad.
template <typename T> struct BetaDictSums {
    const T *Xt, *Ht, *Am;
    T *Vt, *Q2t, *part;
    int M, R, T_, Tp, S;
    bool fused;
    double beta;
};
template <typename T> int beta_dict_sums(const BetaDictSums<T>& q, hipStream_t s);
// once per call, before the first beta_dict_sums: the fused kernel's LDS limit
template <typename T> int beta_dict_sums_prepare(bool fused);

}  // namespace evc
