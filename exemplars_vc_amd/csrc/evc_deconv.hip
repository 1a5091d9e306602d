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
// The kernels themselves are in evc_deconv_kernels.h, which evc_deconv_learn.hip includes too.
#include "evc_deconv_kernels.h"

namespace evc {

namespace {

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
    return beta_report<T>(c, o.iters, n_iter_out, err_out, n_slots, s);
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
