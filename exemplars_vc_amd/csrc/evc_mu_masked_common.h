// Declarations shared by evc_mu_masked.hip (evc_mu_masked_solve, evc_mu_masked_learn) and evc_mu_stoch.hip
// (evc_mu_stoch_learn): the arguments of k_mum_sweep, numpy's maxima and the host steps of the activation half and of the
// unfused dictionary half that the mini-batch driver reuses unchanged.
#pragma once
#include "evc_beta_common.h"
#include "evc_mu_masked_plan.h"

namespace evc {

template <typename T> struct MumArgs {
    const T* Ap1;           // [NP][MP] exemplars as rows, bins contiguous, zero-padded
    const T* Ap3;           // [NP][MP] the same with the bins of every chunk of 16 permuted: slot 4 g + s = bin 4 s + g
    const T* Xp;            // [n_tiles][MP][16] frames of a tile, zero-padded
    const T* XMp;           // [n_tiles][MP][16] mask . X
    const T* Mp;            // [n_tiles][MP][16] mask
    T* H;
    long hs_t, hs_n;        // H(n, t) = H[t * hs_t + n * hs_n]
    const int4* tiles;      // {utterance, first frame, frames, -}
    const int* stop;        // [n_utt] 0: running; else the iteration the utterance stopped at
    double* errf;           // [n_tiles * 16] per-frame share of the error
    int M, MP, N, NP;
};

// one call's activation half: the kernel arguments, the carved workspace and the tile count
template <typename T> struct MumCtx {
    MumArgs<T> a;
    MumWs w;
    int n_tiles, n_utt, n_slots, fm;
};

// (max(v, lo) as numpy's maximum: a NaN passes)
template <typename T> __device__ __forceinline__ T max_nan(T v, T lo) { return !(v <= lo) ? v : lo; }
// (numpy's max: a NaN passes)
__device__ __forceinline__ double max_pass_nan(double a, double b) { return a != a ? a : b != b ? b : a > b ? a : b; }

// ----- evc_mu_masked.hip: the host steps evc_mu_stoch_learn shares with it -----
// once per call, before the first mum_sweep: k_mum_sweep's LDS limit
template <typename T> int mum_sweep_prepare();
// the two packed images of the dictionary k_mum_sweep streams, into c.w.Ap1 | c.w.Ap3 (c.a.M, MP, N, NP, c.fm, c.n_tiles)
template <typename T> int mum_pack_dict(const MumCtx<T>& c, const T* A, int lda, hipStream_t s);
// one multiplicative update of the activations of every tile whose utterance's stop word is 0, in place
template <typename T> int mum_sweep(const MumArgs<T>& a, int loss, int n_tiles, hipStream_t s);
// k_mum_dict_q: Q1t | Q2t [rows][ldq] from Vt and X, mask (NULL: 1) addressed as the caller's: l2 mask . X | mask . V,
// kl (mask . X) / (V + J) | mask; zero where m >= M or t >= T_
template <typename T>
int mum_dict_q(int loss, const T* X, int ldx, const T* mask, int ldm, int fm, const T* Vt, T* Q1t, T* Q2t, int ldq, int M, int T_,
               long rows, hipStream_t s);

}  // namespace evc
