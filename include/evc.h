/*
 * evc.h - C ABI of libevc_hip.so: the MI355X (gfx950) exemplar-NMF activation solver.
 *
 * The reference (entn-at/exemplars_vc) is pure Python and has no FFI of its own; the
 * boundary of its hot path is three plain-Python call surfaces.  This header is the
 * native boundary those surfaces bind to (see INTEGRATION.md for the ctypes stubs):
 *
 *   evc_nmf_solve   replaces the multiplicative-update loop behind
 *                     - _factorize()                    04_align_n_nmf.py:194-215
 *                       (sklearn _fit_multiplicative_update, _nmf.py:731-893,
 *                        _multiplicative_update_w beta=2 branch, _nmf.py:526-556,612-631)
 *                     - pymf NMF._update_h / factorize  pymf/nmf.py:66-70, pymf/base.py:208-270
 *                     - nmf_tool NMF.NMF (mu, initW)    nmf_tool/nmf.py:36-40,57-67
 *   evc_synthesize  replaces np.matmul(H.T, B) in convert()  04_align_n_nmf.py:371-373,391
 *   evc_nmf_convert both of the above back to back (factorize() + convert(), :452-455)
 *   evc_griffin_lim replaces reconstruct_signal_griffin_lim()  zz_audio_utilities.py:258-292
 *   evc_stft        replaces librosa.core.stft(...) of 04_align_n_nmf.py:422
 *   evc_mfcc        replaces lbr.feature.mfcc(audiodatum, sr=sr, n_fft=frame_length, hop_length=hop_length) of
 *                   _extract_features()  01_make_dict_parallel.py:96-104 - the features the DTW below aligns - for all
 *                   utterances of a speaker in one call, with the STFT frames of 03_a_b_r_parallel.py:103 as a by-product
 *   evc_dtw_align   replaces _dtw_alignment() / dtw_alignment()  01_make_dict_parallel.py:215-249
 *   evc_dtw_path_rows, evc_dtw_gather_rows  replace align_sp_ap_f0() + the stacking  04_align_n_nmf.py:100-169,230-246
 *   evc_residual    replaces sklearn _beta_divergence(beta=2, square_root=True)
 *                   (_nmf.py:85-135) and pymf frobenius_norm (pymf/base.py:144-165)
 *   evc_cd_solve    replaces the coordinate-descent loop behind _factorize() of 04_align_n_nmf_pytorch.py:189-210
 *                   (sklearn solver='cd', update_H=False: _fit_coordinate_descent, _nmf.py:496-521,
 *                    _update_coordinate_descent, :376-404, _cdnmf_fast.pyx)
 *   evc_nmf_learn   replaces the multiplicative-update loop that also learns the dictionary: sklearn
 *                   _fit_multiplicative_update with update_H=True (_nmf.py:731-893; beta = 2, or beta = 1 with
 *                   evc_learn_opts.loss = EVC_LOSS_KL: _nmf.py:556-606, 634-728) and pymf's default
 *                   factorize(compute_w=True) (pymf/nmf.py:66-76, pymf/base.py:238-270); evc_learn_workspace_bytes and
 *                   evc_learn_splits size and describe it
 *   evc_cd_learn    replaces the coordinate-descent loop that also learns the dictionary: sklearn's default solver,
 *                   NMF(n_components=...).fit_transform(...) of 05_conversion.py:100-106 (solver='cd', update_H=True:
 *                   _fit_coordinate_descent, _nmf.py:496-521, both calls of _update_coordinate_descent, :376-404);
 *                   evc_cd_learn_workspace_bytes and evc_cd_learn_splits size and describe it
 *   evc_beta_solve  replaces the multiplicative-update loop behind _factorize(X, W, beta_loss=...) of 04_align_n_nmf.py:194-215
 *                   for the losses evc_nmf_solve does not serve: beta_loss = 'itakura-saito' or any float (sklearn
 *                   _multiplicative_update_w, _nmf.py:556-631, and _beta_divergence, :85-189, with update_H=False);
 *                   evc_beta_workspace_bytes sizes it
 *   evc_beta_learn  replaces the multiplicative-update loop that also learns the dictionary under the losses evc_nmf_learn
 *                   does not serve: sklearn _fit_multiplicative_update with update_H=True and beta_loss = 'itakura-saito'
 *                   or any float (_nmf.py:526-893); evc_beta_learn_workspace_bytes, evc_beta_learn_splits and
 *                   evc_beta_learn_route size and describe it
 *   evc_online_learn  replaces MiniBatchNMF(init='custom', fresh_restarts=False).fit_transform(X, W=W, H=H): the mini-batch
 *                   learner for any beta_loss (sklearn _minibatch_step, _multiplicative_update_h with A, B and rho,
 *                   _minibatch_convergence); evc_online_workspace_bytes and evc_online_splits size and describe it
 *   evc_online_transform  replaces MiniBatchNMF.transform(X) with a dictionary learned online (sklearn _solve_W,
 *                   _nmf.py:2046-2071): the activation solve that stops on the change of its activations, checked every
 *                   iteration on the device; evc_online_transform_workspace_bytes sizes it
 *   evc_online_learn_fresh  replaces MiniBatchNMF(init='custom', fresh_restarts=True).fit_transform(X, W=W, H=H) and, one
 *                   step at a time, MiniBatchNMF.partial_fit: evc_online_learn whose every step solves its batch's
 *                   activations afresh (_solve_W) and whose fit ends with that solve over all frames;
 *                   evc_online_fresh_workspace_bytes sizes it
 *   evc_deconv_solve  has no counterpart in the reference, whose README cites the method and switches to a "simpler version
 *                   of exemplar-based method" first: the activation solve with multi-frame exemplars (non-negative spectrogram deconvolution, Wu et
 *                   al.), X[:, t] ~ sum_tau A_tau H[:, t - tau]; with one tap it is scikit-learn's fixed-dictionary
 *                   multiplicative update.  evc_deconv_workspace_bytes sizes it, evc_deconv_synthesize forms
 *                   Y[:, t] = sum_tau B_tau H[:, t - tau] from the parallel target segments
 *   evc_deconv_learn  is evc_deconv_solve's learning counterpart, convolutive NMF (NMFD): both factors of
 *                   X ~ sum_tau W_tau shift_tau(H) by multiplicative updates; with one tap it is scikit-learn's
 *                   _fit_multiplicative_update with update_H=True, as evc_nmf_learn.  evc_deconv_learn_workspace_bytes
 *                   and evc_deconv_learn_splits size and describe it
 *   evc_semi_solve  replaces pymf's SNMF(data, num_bases).factorize(compute_w=False) (pymf/snmf.py:66-85,
 *                   pymf/base.py:208-270): semi-NMF activations, signed data and dictionary, non-negative activations -
 *                   the solve for the signed mel-cepstra of the dictionary build; evc_semi_workspace_bytes sizes it
 *   evc_convex_learn  replaces pymf's CNMF(data, num_bases).factorize() (pymf/cnmf.py:97-175): convex NMF,
 *                   X ~ (X G) H with G, H >= 0 and signed X - the atoms are non-negative combinations of the exemplars
 *                   themselves, which compacts a signed parallel dictionary; evc_convex_workspace_bytes sizes it,
 *                   evc_convex_splits tells the k-ranges of its Gram sweeps
 *   evc_prox_solve  replaces deComP's lasso.solve / nnls.solve with method ista, fista, ista_pos, fista_pos
 *                   (decomp/lasso.py:97-189, 274-297, 388-415): L1-penalised activations by proximal gradient, signed or
 *                   non-negative, with exact zeros; evc_prox_workspace_bytes sizes it
 *   evc_prox_masked_solve  the same solves with deComP's 2-D `mask` (missing data: a weight per bin of every frame,
 *                   lasso.py:306-328, 418-445) on a factored sweep without the N x N Gram matrix; a NULL mask is the unmasked
 *                   problem on that sweep, for M << N; evc_prox_masked_workspace_bytes sizes it
 *   evc_prox_learn  replaces deComP's dictionary_learning.solve(method='block_cd') (decomp/dictionary_learning.py:114-168):
 *                   online sparse dictionary learning (Mairal et al.) - per mini-batch evc_prox_solve's lasso, the forgetting
 *                   update of two sufficient statistics and one block-coordinate sweep over the atoms with |d_j| <= 1;
 *                   evc_prox_learn_workspace_bytes sizes it, evc_prox_learn_block tells the sweep's block width
 *   evc_prox_masked_learn  the same learning with deComP's `mask` (dictionary_learning.py:171-231): evc_prox_masked_solve's
 *                   lasso, one Gram statistic per bin and a Jacobi update of all atoms from the old dictionary;
 *                   evc_prox_masked_learn_workspace_bytes sizes it
 *   evc_mu_masked_solve  replaces the activation half of deComP's nmf.solve(method='mu', likelihood='l2' | 'kl', mask=...)
 *                   (decomp/nmf_methods/grads.py:77-84, 108-115, 143-150): multiplicative updates with a weight per bin of
 *                   every frame (missing data), the dictionary fixed, on a factored sweep with the weights applied between
 *                   its two contractions; a NULL mask is the unmasked update; evc_mu_masked_workspace_bytes sizes it
 *   evc_mu_masked_learn  replaces deComP's nmf.solve(method='mu', likelihood='l2' | 'kl', mask=...) itself (decomp/nmf.py:16-80,
 *                   nmf_methods/batch_mu.py, utils/normalize.py): batch NMF with a weight per entry and unit-norm atoms - per
 *                   iteration evc_mu_masked_solve's update, the same update of the dictionary and its normalisation;
 *                   evc_mu_masked_learn_workspace_bytes and evc_mu_masked_learn_splits size and describe it
 *   evc_mu_stoch_learn  replaces deComP's nmf.solve(minibatch=bs, method='asg-mu' | 'gsg-mu' | 'asag-mu' | 'gsag-mu' | 'svrmu' |
 *                   'svrmu-acc') (nmf_methods/serizel.py, nmf_methods/kasai.py): mini-batch NMF - per step evc_mu_masked_solve's
 *                   update on the batch's frames, a fused masked dictionary gradient and the method's dictionary update, the
 *                   stop decided on the device; evc_mu_stoch_learn_workspace_bytes, evc_mu_stoch_learn_route and
 *                   evc_mu_stoch_learn_splits size and describe it
 *   evc_kmeans      replaces pymf's Kmeans(data, num_bases).factorize() (pymf/kmeans.py:57-83, pymf/dist.py:54-127): k-means
 *                   on the device - the assignment on the matrix cores with the argmin fused into its epilogue, deterministic
 *                   means, the stop decided on the device; CNMF's default start and a vector-quantised parallel codebook;
 *                   evc_kmeans_workspace_bytes sizes it, evc_kmeans_splits tells the centre ranges of its assignment
 *
 * Conventions
 *   Math (BASELINE.json north_star): X is M x T (bins x frames), A is M x N (source
 *   exemplar dictionary), B is Mb x N (parallel target dictionary), H is N x T, Y = B H.
 *   All pointers are DEVICE pointers unless marked "host".  Nothing here allocates,
 *   frees or throws; every function returns a status (0 ok; -1 invalid argument, -2 workspace
 *   too small, -3 unsupported combination, -4 cooperative launch timed out twice (not reachable:
 *   the redo is not cooperative); >0 a hipError_t value).  Work is enqueued on `stream`.
 *   Host synchronisation - exactly these cases, nothing else waits:
 *     (1) n_iter_out / err_out / rmse_out non-NULL: the call returns after copying them back;
 *     (2) evc_nmf_solve / evc_nmf_convert on the float64 fused path (M <= 32) when several workgroups
 *         share a frame tile and exchange partial sums inside a launch (k_fused_all for N > 512,
 *         the cooperative k_fused_res launch for one or two utterances): one round trip at the end
 *         of the call reads the flag that tells whether a workgroup gave up waiting for its peers (then
 *         the solve is redone without any exchange).  EVC_FLAG_NO_EXCHANGE keeps such a call fully
 *         asynchronous (at about half the speed for a lone utterance, ~10 % less for large batches);
 *     (3) evc_nmf_solve / evc_nmf_convert on the task-queue kernels for wide spectra (k_fused_wide: float32,
 *         32 < M <= 208, from one utterance (43 frame tiles) on; k_fused_wide64: float64,
 *         144 < M <= 528, inside the batch windows of use_wide (csrc/evc_solve_plan.h), which keep M <= 176 out:
 *         the same round trip, taken BEFORE anything is written to H or Y, so that a solve whose wait ran out is
 *         redone on the two-contraction path from the untouched inputs (evc_solve_info.redo = 1).  Round 3 delivered
 *         NaN under status 0 there.  EVC_FLAG_NO_EXCHANGE routes away from these kernels too.  Batches of up to ~5
 *         utterances run these kernels on a static schedule (one task per workgroup and iteration) that needs all its
 *         workgroups resident at once, like k_fused_all's exchange: two such solves started concurrently on two streams
 *         can starve each other until the bounded waits run out (seconds) and both are redone - give concurrent
 *         small solves EVC_FLAG_NO_EXCHANGE (the compat layer's side streams do).  Larger batches draw tasks from a
 *         queue and depend on nobody's residency;
 *     (4) evc_cd_solve: n_iter_out / violation_out non-NULL (the call returns after copying them back).  Its kernels
 *         never exchange data between workgroups inside a launch and assume nothing about residency: concurrent
 *         coordinate-descent solves on several streams are safe.
 *     (5) evc_nmf_learn: with check_every = 0 and NULL n_iter_out / err_out the call is fully asynchronous.  Otherwise the
 *         host reads one double (the error) at each check that is evaluated and decides the stop there; checks are
 *         evaluated when err_out is non-NULL or tol > 0.  Its own kernels never exchange data between workgroups inside a
 *         launch, and its activation step runs with EVC_FLAG_NO_EXCHANGE: concurrent calls on several streams are safe.
 *         evc_deconv_learn follows the same rule with its own kernels.
 *     (6) evc_cd_learn: only with tol == 0 and NULL n_iter_out / violation_out is the call a pure enqueue of max_iter
 *         iterations.  Otherwise the host reads the iteration's two violations (two doubles) after every iteration and
 *         decides the stop there.  None of its kernels exchanges data between workgroups inside a launch, uses atomics or
 *         assumes residency: concurrent calls on several streams are safe.
 *     (7) evc_mfcc: never.  The call is a pure enqueue; no scalar comes back to the host (the per-utterance maximum of
 *         the decibel clamp is formed on the device from per-workgroup partial maxima, without atomics).
 *     (8) evc_beta_solve: n_iter_out / err_out non-NULL (the call returns after copying them back); otherwise the call is
 *         a pure enqueue: the per-utterance stop state lives on the device.  None of its kernels exchanges data between
 *         workgroups inside a launch, uses float atomics or assumes residency: concurrent calls on several streams are safe.
 *     (9) evc_beta_learn: with check_every = 0 and NULL n_iter_out / err_out the call is a pure enqueue.  Otherwise the
 *         host reads one double (the error) at each check that is evaluated and decides the stop there, as in case (5);
 *         checks are evaluated when err_out is non-NULL or tol > 0.  None of its kernels exchanges data between workgroups
 *         inside a launch, uses float atomics or assumes residency: concurrent calls on several streams are safe, and the
 *         same call gives the same bits every time.
 *     (10) evc_online_learn: with tol == 0, max_no_improvement < 0 and NULL n_iter_out, n_steps_out and trace_out the call
 *         is a pure enqueue of max_iter passes.  Otherwise the host reads three doubles after every step (the batch cost
 *         and the two sums of squares of the dictionary's change ratio) and decides the stop there.  None of its kernels
 *         exchanges data between workgroups inside a launch, uses float atomics or assumes residency: concurrent calls on
 *         several streams are safe, and the same call gives the same bits every time.
 *     (11) evc_online_transform: n_iter_out / change_out non-NULL (the call returns after copying them back); otherwise the
 *         call is a pure enqueue of max_iter iterations: the change ratio is formed and the stop decided on the device, per
 *         utterance, without a host round trip.  None of its kernels exchanges data between workgroups inside a launch, uses
 *         float atomics or assumes residency: concurrent calls on several streams are safe, and the same call gives the
 *         same bits every time.
 *     (12) evc_online_learn_fresh: as case (10) - with tol == 0, max_no_improvement < 0 and NULL n_iter_out, n_steps_out and
 *         trace_out the call is a pure enqueue (every solve runs its full count); otherwise the host reads three doubles
 *         after every step.  The solves inside a step and the one that ends the fit stop on the device, as in case (11).
 *     (13) evc_deconv_solve: n_iter_out / err_out non-NULL (the call returns after copying them back); otherwise the call
 *         is a pure enqueue: the errors are summed and the stop decided on the device, per utterance.  evc_deconv_synthesize
 *         never waits.  None of their kernels exchanges data between workgroups inside a launch, uses float atomics or
 *         assumes residency: concurrent calls on several streams are safe, and the same call gives the same bits every time.
 *   No global mutable state: calls on distinct streams/devices are independent and the
 *   caller's current device (hipSetDevice) is honoured.  Nothing is read from the process environment.
 *   Host arrays (utt_offsets, frame_offsets, a_offsets / b_offsets, sample_offsets) are consumed before the call returns: they are
 *   copied to the device by hipMemcpyAsync from pageable memory, which HIP stages at enqueue time; keep them valid
 *   until the call returns, not longer.
 *   k_fused_all's exchange carries its arrival flag in the lowest mantissa bit of every partial sum it publishes
 *   (readers clear it): each partial V' is truncated by at most one ulp; infinities pass unchanged, and so do NaNs (a
 *   partial sum is a result of arithmetic, i.e. a quiet NaN, which stays a NaN without bit 0).  So does k_fused_wide on its
 *   static schedule with reduce slices (float32, batches of up to ~5 utterances; evc_solve_info.variant bit 2): every
 *   partial sum and summed slice is rounded to an even significand (half to even: at most one float32 ulp);
 *   infinities and NaNs are not rounded (0x7FFFFFFF would carry into the sign bit) and stay what they are.
 *   A NaN or infinity in a frame of X stays in that frame's column.  The other frames' results are bitwise those of the
 *   same call without it in k_fused_wide and k_fused_wide64; in the fused float64 kernels for M <= 32 the frames that
 *   share its frame tile of 16 may take the IEEE division instead of the shared reciprocal (<= 2 ulp apart, see
 *   EVC_FLAG_EXACT_DIV).
 */
#ifndef EVC_H
#define EVC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVC_VERSION 100 /* 0.1.0 */

/* hipStream_t, spelled without the HIP headers so that C callers can include this file. */
typedef struct ihipStream_t* evc_stream_t;

/* element type of every matrix in a call (the arithmetic is carried out in the same type) */
enum { EVC_F64 = 0, EVC_F32 = 1 };

/* storage order of the caller's matrices
 *   FRAME_MAJOR : the reference scripts' orientation (frames / exemplars as rows):
 *                 X[t*ldx+m]  A[n*lda+m]  B[n*ldb+mb]  H[t*ldh+n]  Y[t*ldy+mb]
 *                 (X = `X` T x M, A = `W` N x M of _factorize; H = sklearn's W, T x N)
 *   BIN_MAJOR   : the north_star / pymf / nmf_tool orientation (bins as rows):
 *                 X[m*ldx+t]  A[m*lda+n]  B[mb*ldb+n] H[n*ldh+t]  Y[mb*ldy+t]          */
enum { EVC_FRAME_MAJOR = 0, EVC_BIN_MAJOR = 1 };

/* how the denominator D = A^T A H (+ l1) is guarded, and the multiply/divide order
 *   ADD          H <- (H*P) / (D + eps)            pymf nmf.py:68-70      (eps = 1e-9)
 *   ZERO_REPLACE D[D==0] = eps; H <- H * (P/D)     sklearn _nmf.py:620-629 (eps = 1.1920929e-7)
 *   NONE         H <- H * P / D                    nmf_tool nmf.py:39
 *   CLAMP        H <- H * (P / max(D, eps))        deComP batch_mu.py:8-26 (eps = 1e-15)   */
enum { EVC_EPS_ADD = 0, EVC_EPS_ZERO_REPLACE = 1, EVC_EPS_NONE = 2, EVC_EPS_CLAMP = 3 };

/* which algebra evaluates the denominator
 *   GRAM      G = A^T A and P = A^T X once, then G H per iteration (sklearn's hoisting)
 *   FACTORED  A^T (A H) per iteration: 4MN instead of 2N^2 flop per frame-iteration
 *   LITERAL   G and P recomputed in every iteration, as pymf/nmf_tool literally do
 *   AUTO      FACTORED                                                                    */
enum { EVC_ALGO_GRAM = 0, EVC_ALGO_FACTORED = 1, EVC_ALGO_LITERAL = 2, EVC_ALGO_AUTO = 3 };

/* initial activations
 *   GIVEN    H holds H0 on entry (pymf / nmf_tool: random, caller-seeded)
 *   SKLEARN  every entry of utterance u starts at sqrt(mean(X_u) / N)  (_nmf.py:1228-1231)
 *   CONST    every entry starts at init_value                                              */
enum { EVC_INIT_GIVEN = 0, EVC_INIT_SKLEARN = 1, EVC_INIT_CONST = 2 };

/* stopping rule, evaluated per utterance every `check_every` iterations on
 * err = ||X_u - A H_u||_F
 *   NONE     errors are recorded (if check_every > 0) but never stop the loop
 *   SKLEARN  stop when (err_prev - err) / err_at_init < tol       (_nmf.py:871-884)
 *   PYMF     from the third recorded error on, stop when |err - err_prev| / T_u < tol
 *            (pymf/base.py:189-206,266-270)
 *   DECOMP   evc_prox_solve only, on the change of the activations instead of the error: at iterations
 *            i = 0, check_every, 2 check_every, ... stop when max(|X_new - X_old| - tol_n) < 0 over the
 *            utterance's frames and all exemplars (deComP lasso.py:293, check_every = 10)     */
enum { EVC_STOP_NONE = 0, EVC_STOP_SKLEARN = 1, EVC_STOP_PYMF = 2, EVC_STOP_DECOMP = 3 };

/* divergence minimised by the multiplicative update
 *   FROBENIUS  H <- H (.) A^T X (/) (A^T A H)                       (what the scripts force, :210)
 *   KL         H <- H (.) A^T (X (/) max(A H, eps)) (/) colsum(A)   generalised Kullback-Leibler: the
 *              default of _factorize's signature (04_align_n_nmf.py:194), sklearn _nmf.py:556-606;
 *              requires EVC_EPS_ZERO_REPLACE (sklearn's guards) and l1 == 0; the residual reported
 *              to the stopping rule is sqrt(2 KL(X || A H)) (_nmf.py:136-160)                      */
enum { EVC_LOSS_FROBENIUS = 0, EVC_LOSS_KL = 1 };

/* evc_solve_opts.reserved
 *   NO_FUSED         the generic two-contraction path instead of the fused persistent kernels (M <= 32)
 *   EXACT_DIV        correctly rounded quotients in the fused float64 kernels (always on with EVC_STOP_PYMF;
 *                    else a shared / refined reciprocal, <= 2 ulp)
 *   NO_EXCHANGE      no kernel in which workgroups exchange data inside a launch (k_fused_all with more than one member,
 *                    cooperative k_fused_res, the task queues k_fused_wide / k_fused_wide64): the call is then fully
 *                    asynchronous (see "Host synchronisation" above); a latency / determinism knob
 *   NO_ALL_RESIDENT  keep k_fused_all out (k_fused_res, with its cooperative launch for few frame tiles)
 *   PAIR_TILES       tuning / experiments: k_fused_xy (two frame tiles per member, exchange phases inside the sweeps)
 *                    instead of k_fused_all where both apply; measured slower (profiles/r04_xy_notes.md)
 *   NO_LONE_BIN      A/B and tests: M = 25 with 2, 4 or 8 members (N = 1024, 2048, 4096) runs k_fused_all's own 15-MFMA
 *                    unit instead of k_fused_lone's 14 (bin 24 folded into the denominators' start value: the same sums with
 *                    bin 24 added first, so results differ in the last bits; C2 +1.5 %, profiles/lone_bin_README.md).
 *                    evc_solve_info reports EVC_KERNEL_FUSED_ALL either way; no other shape is affected
 *   NO_RANGE_HOIST   A/B and tests: k_fused_all / k_fused_lone with 1, 2, 4 or 8 members (N <= 4096, Frobenius) test every
 *                    unit's denominators for the fast quotients' range, as every other kernel does, instead of deciding
 *                    it once per sweep from bounds on V and on the member's dictionary (mu_tile_hoisted,
 *                    evc_fused_common.h).  Results are bit for bit the same either way
 *   NO_QUAD_ROWS     A/B and tests: the shapes of k_fused_lone (M = 25; 2, 4 or 8 members) run that kernel, not k_fused_quad,
 *                    which computes bins 16 .. 24 of V' with twelve v_mfma_f64_4x4x4_4b_f64 per unit instead of a second
 *                    16-row tile (9 real rows) of four v_mfma_f64_16x16x4_f64 (profiles/quad_rows_README.md).  The same
 *                    products grouped the same way; evc_solve_info reports EVC_KERNEL_FUSED_ALL either way */
enum { EVC_FLAG_NO_FUSED = 1, EVC_FLAG_EXACT_DIV = 2, EVC_FLAG_NO_EXCHANGE = 4, EVC_FLAG_NO_ALL_RESIDENT = 16, EVC_FLAG_PAIR_TILES = 32,
       EVC_FLAG_NO_LONE_BIN = 64, EVC_FLAG_NO_RANGE_HOIST = 128, EVC_FLAG_NO_QUAD_ROWS = 1 << 20 };

struct evc_solve_info;
struct evc_dict;
typedef struct evc_solve_opts {
    int struct_bytes;  /* sizeof(evc_solve_opts), for forward compatibility */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int algo;          /* EVC_ALGO_* */
    int iters;         /* maximum number of multiplicative updates (>= 0) */
    int eps_mode;      /* EVC_EPS_* */
    int init_mode;     /* EVC_INIT_* */
    int check_every;   /* 0: never evaluate the residual; k>0: every k iterations */
    int stop_rule;     /* EVC_STOP_* */
    int reserved;      /* flags, 0 = defaults: an OR of EVC_FLAG_* (below); bits 8..15: tuning only - M <= 32: 1 | 2 force
                          the general streamed kernel with that many frame tiles per workgroup; M > 32: that many exemplar
                          ranges per frame group in k_fused_wide / k_fused_wide64, whatever the batch size; bits 16..19,
                          tuning only: k_fused_wide with 4 | 8 wavefronts per workgroup, k_fused_wide64 with at least 3 | 4 | 5 | 7 | 8
                          whole bin tiles per wavefront (the narrowest instance that holds M); other values: status -1; with
                          a prepared dictionary whose images do not fit the override: status -3 */
    int loss;          /* EVC_LOSS_* */
    int test_abort_at; /* 0 in production.  Tests only: k > 0 pretends, in front of the k-th launch of the iteration
                          loop, that a workgroup gave up waiting for its peers (the abort flag is raised as a timed-out
                          wait would raise it); -1: the call starts with the flag raised.  The solve then takes the
                          documented redo path and evc_solve_info.redo reports 1. */
    double eps;        /* guard value for eps_mode */
    double l1;         /* added to the denominator (sklearn l1_reg_W = M*alpha_W*l1_ratio) */
    double tol;        /* threshold of stop_rule */
    double init_value; /* EVC_INIT_CONST */
    /* optional hipEvent_t pair recorded on `stream` immediately before / after the launches of
     * the iteration loop (the dominant kernel); NULL = not recorded.  Used by bench.py to time
     * that kernel live with HIP events. */
    void* ev_loop_start;
    void* ev_loop_stop;
    /* optional evc_solve_info* (host, caller-owned, struct_bytes set by the caller; NULL = not wanted): filled before the
     * call returns with what the library actually ran.  No extra synchronisation: `redo` is known from the round trip an
     * exchanging solve performs anyway. */
    struct evc_solve_info* info;
    /* optional prepared dictionary (host struct filled by evc_dict_prepare; NULL = import A / B from the caller's
     * matrices on every call, as the reference's scripts effectively do).  With a prepared dictionary the A and B
     * arguments of evc_nmf_solve / evc_nmf_convert are ignored (may be NULL); M, Mb, N, dtype, loss and layout-independent
     * options must match what it was prepared for, else the call returns -1. */
    const struct evc_dict* dict;
} evc_solve_opts;

/* the kernel that carried the iteration loop of a solve */
enum {
    EVC_KERNEL_NONE = 0,
    EVC_KERNEL_GEMM_NT = 1,     /* generic path, k_gemm_nt x2 per iteration (float64, M > 32; GRAM / LITERAL) */
    EVC_KERNEL_GEMM2 = 2,       /* generic path, k_gemm2 x2 per iteration (float32) */
    EVC_KERNEL_FUSED_MU = 3,    /* k_fused_mu: fused FACTORED, everything streamed (M <= 32) */
    EVC_KERNEL_FUSED_RES = 4,   /* k_fused_res: half of H register-resident (members > 1: its cooperative launch) */
    EVC_KERNEL_FUSED_ALL = 5,   /* k_fused_all: H and P register-resident, `members` workgroups per frame tile */
    EVC_KERNEL_FUSED_WIDE = 6,  /* k_fused_wide: fused FACTORED for float32, 32 < M <= 208: task queue over (frame group, exemplar range) */
    EVC_KERNEL_FUSED_WIDE64 = 7, /* k_fused_wide64: the same for float64, 144 < M <= 528 (bins split over a workgroup's wavefronts) */
    EVC_KERNEL_FUSED_XY = 8     /* k_fused_xy: H and P register-resident, `members` workgroups per PAIR of frame tiles, the
                                   exchange phases inside the sweeps (round 4; on request only: EVC_FLAG_PAIR_TILES) */
};

typedef struct evc_solve_info {
    int struct_bytes;  /* in: sizeof(evc_solve_info) */
    int kernel;        /* EVC_KERNEL_* of the (last) attempt whose results were delivered */
    int members;       /* workgroups / tasks sharing one frame tile or frame group (1: no sharing) */
    int launches;      /* kernel launches of the iteration loop (all attempts) */
    int redo;          /* 1: an exchange wait ran out and the solve was redone on kernels without exchange */
    int exchange;      /* 1: the delivered results come from a kernel whose workgroups exchange partial sums in a launch */
    int prepared;      /* 1: the dictionary came from an evc_dict_prepare image (no per-call import / packing) */
    int variant;       /* k_fused_all: bit 0: its last launch formed Y = B H itself (evc_nmf_convert: no second pass over the
                          activations); bit 1, with bit 0 only: that launch still stored the packed activations (a
                          reader followed).  0 for every other solve on that kernel.
                          The instance and schedule of the task-queue kernels (0 for every other kernel):
                          bit 0: static schedule (workgroup b runs task b of every iteration; else a ticket queue);
                          bit 1: reduce slices (reduce tasks sum the partial V' of a frame group);
                          bit 2: tagged hand-offs (the epoch bit rides in the data; k_fused_wide only);
                          bits 8..15: k_fused_wide: wavefronts per workgroup (4 | 8); k_fused_wide64: whole bin tiles per
                                      wavefront (3 | 4 | 5 | 7 | 8);
                          bits 16..23: bin tiles of 16 the instance holds (k_fused_wide: MT = 4 | 6 | 8 | 10 | 13;
                                       k_fused_wide64: 4 x tiles per wavefront + 1)
                          The block shapes of the two contraction kernels (EVC_KERNEL_GEMM_NT, EVC_KERNEL_GEMM2; a redone
                          solve reports the kernel it was redone on).  Block codes, frames x rows of the other operand:
                          0 none, 1 64 x 64, 2 64 x 128, 3 128 x 64, 4 128 x 128, 5 128 x 128 with deep k-slabs (k_gemm2,
                          diagnostic builds only):
                          bits 0..3: the update contraction (the one whose epilogue is the multiplicative update);
                          bits 4..7: V = H Am^T of the iteration loop (0 for GRAM and LITERAL, which form none there);
                          bits 8..13: the number of k-ranges that product was split into (1: no split);
                          bits 16..19: the numerator P = X A (0 under the Kullback-Leibler loss, which has none) */
} evc_solve_info;

/* A dictionary imported once.  The reference builds A and B once per run (04_align_n_nmf.py:230-246,350-361) and the
 * dictionary is fixed across utterances; every evc_nmf_solve / evc_nmf_convert call nevertheless has to bring the caller's
 * matrices into the layouts its kernels read (zero-padded transposes, MFMA operand fragments, KL column scaling, row
 * sums).  evc_dict_prepare does that once into caller-owned device memory; calls that pass the handle
 * in evc_solve_opts.dict skip it (results are bitwise those of the unprepared call).  The struct is plain host data:
 * copyable, nothing to free besides `mem`, which the caller owns and must keep alive and unmodified while it is used. */
typedef struct evc_dict {
    int struct_bytes;  /* sizeof(evc_dict), set by evc_dict_prepare */
    int magic;
    int M, Mb, N;      /* Mb = 0: no target dictionary B was given (evc_nmf_convert then needs its B argument) */
    int dtype, loss, reserved;
    double eps;        /* KL: the guard the column sums were formed with (must equal evc_solve_opts.eps) */
    void* mem;         /* device memory, evc_dict_bytes() bytes, 256-byte aligned */
    size_t bytes;
} evc_dict;

int evc_version(void);
const char* evc_strerror(int status);

/* bytes of device memory a prepared dictionary of this size needs (0: invalid arguments) */
size_t evc_dict_bytes(int M, int Mb, int N, int dtype, int loss);
/* Import A (M x N) and, if B != NULL, B (Mb x N), both in `layout`, into `mem` and fill *dict.  Asynchronous on `stream`
 * (the handle may be used by later calls on the same stream at once).  eps: the KL guard (ignored for Frobenius).
 * The image serves every algebra and kernel route of evc_nmf_solve / evc_nmf_convert (the Gram matrix of
 * EVC_ALGO_GRAM / LITERAL is still formed per call). */
int evc_dict_prepare(const void* A, int lda, const void* B, int ldb, int M, int Mb, int N, int layout, int dtype,
                     int loss, double eps, void* mem, size_t mem_bytes, evc_dict* dict, evc_stream_t stream);

/* number of GPUs visible to the library (hipGetDeviceCount); <0 on failure */
int evc_device_count(void);

/* Bytes of device workspace evc_nmf_solve / evc_nmf_convert / evc_residual need for a problem of
 * this size.  Mb: bins of the target dictionary B for evc_nmf_convert, 0 otherwise.
 * n_utt is the number of utterances the T frames are split into (>= 1). */
size_t evc_workspace_bytes(int M, int Mb, int N, int T, int n_utt, int dtype, int algo);

/* Solve X ~ A H for H >= 0 with A fixed: `iters` multiplicative updates
 *   H <- H (.) A^T X (/) guard(A^T A H + l1).
 *
 * The T frames are the concatenation of n_utt utterances; utt_offsets (host, n_utt+1
 * ascending ints, utt_offsets[0]=0, utt_offsets[n_utt]=T) delimits them, NULL means one
 * utterance.  Utterances only matter for EVC_INIT_SKLEARN and for the stopping rule, both
 * of which the reference applies per call, i.e. per utterance: frames of a stopped
 * utterance are frozen while the others go on.
 *
 * n_iter_out (host, n_utt ints or NULL): updates applied to each utterance.
 * err_out    (host, n_utt * (1 + iters/check_every) doubles or NULL): per utterance, the
 *            residual at init followed by the residual at each check that was evaluated
 *            (unevaluated slots are NaN).
 * When both are NULL the call is fully asynchronous.                                    */
int evc_nmf_solve(const void* A, int lda, const void* X, int ldx, void* H, int ldh,
                  int M, int N, int T,
                  const int* utt_offsets, int n_utt,
                  const evc_solve_opts* opts,
                  void* workspace, size_t workspace_bytes,
                  int* n_iter_out, double* err_out,
                  evc_stream_t stream);

/* evc_nmf_solve followed by Y = B H in one launch sequence: factorize() + convert() of
 * 04_align_n_nmf.py:218-333,336-393 (the __main__ sequence :452-455).  The synthesis reads the
 * activations in the solver's own tile layout, so H is not re-read in the caller's layout; H may be
 * NULL when only Y is wanted (not with EVC_INIT_GIVEN).  B: Mb x N target exemplars, Y: Mb x T,
 * both in opts->layout.  Workspace: evc_workspace_bytes(M, Mb, N, T, ...). */
int evc_nmf_convert(const void* A, int lda, const void* X, int ldx, const void* B, int ldb,
                    void* H, int ldh, void* Y, int ldy,
                    int M, int Mb, int N, int T,
                    const int* utt_offsets, int n_utt,
                    const evc_solve_opts* opts,
                    void* workspace, size_t workspace_bytes,
                    int* n_iter_out, double* err_out,
                    evc_stream_t stream);

/* Y = B H  (04_align_n_nmf.py:391: np.matmul(H.T, B) in FRAME_MAJOR orientation). */
int evc_synthesize(const void* B, int ldb, const void* H, int ldh, void* Y, int ldy,
                   int Mb, int N, int T, int layout, int dtype, evc_stream_t stream);

/* err2_out[t] (device, T values of `dtype`... always double) = sum_m (X[m,t] - (A H)[m,t])^2.
 * The Frobenius residual of a set of frames is sqrt of the sum of its entries.
 * workspace: evc_workspace_bytes(M, 0, N, T, 1, dtype, EVC_ALGO_GRAM) suffices.            */
int evc_residual(const void* A, int lda, const void* X, int ldx, const void* H, int ldh,
                 int M, int N, int T, int layout, int dtype,
                 double* err2_out, void* workspace, size_t workspace_bytes,
                 evc_stream_t stream);

/* STFT front end - the feature extraction that feeds the path when the scripts run on STFT features:
 * librosa.core.stft(y, n_fft=400, hop_length=80, window='hann') at 04_align_n_nmf.py:422 and
 * 03_a_b_r_parallel.py:103 (librosa is a third-party dependency absent here; its published algorithm
 * is restated: frames centred by reflect-padding n_fft/2 samples, periodic Hann window, rfft).  float64.
 *   x      : n_samples doubles (device)
 *   re, im : n_frames x (fft_size/2 + 1), rows are time slices (device) - i.e. the transposed `.T`
 *            the scripts store; n_frames = evc_stft_frames(n_samples, fft_size, hop, center)
 *   center : 1 = librosa's default (reflect padding), 0 = frames start at sample 0            */
int evc_stft_frames(long n_samples, int fft_size, int hop, int center);
size_t evc_stft_workspace_bytes(long n_samples, int fft_size, int hop, int center);
int evc_stft(const void* x, long n_samples, int fft_size, int hop, int center, void* re, int ldre,
             void* im, int ldim, void* workspace, size_t workspace_bytes, evc_stream_t stream);

/* MFCC alignment features - what the dictionary build aligns by DTW: lbr.feature.mfcc(y, sr=16000, n_fft=400,
 * hop_length=80) at 01_make_dict_parallel.py:96-104,358-359, with librosa's defaults for everything else (librosa is
 * absent here; its published algorithm is restated, parity with the package is unpinned).  float64 throughout:
 *   frames   the STFT exactly as evc_stft computes it; power P[t][k] = re^2 + im^2, k < nb = fft_size / 2 + 1
 *   mel      n_mels triangular filters on the Slaney scale (mel(f) = f / (200/3) below 1000 Hz, 15 + ln(f / 1000) /
 *            (ln(6.4) / 27) above) between fmin and fmax, each scaled by 2 / (its width in Hz); Mel = P w^T.  The
 *            filterbank is sparse (394 non-zero weights at sr 16000, fft_size 400, n_mels 128) and is kept
 *            row-compressed: first bin, bin count and weights per filter, summed in ascending bin order
 *   dB       10 log10(max(amin, Mel)), then max(dB, max over the WHOLE UTTERANCE of dB - top_db)
 *   DCT      orthonormal DCT-II over the mel axis, the first n_mfcc coefficients
 * One call takes a batch of utterances:
 *   x              : the samples of all utterances (device doubles); utterance u owns x[sample_offsets[u] ..
 *                    sample_offsets[u + 1] - 1]
 *   sample_offsets : host, n_utt + 1 longs, ascending, sample_offsets[0] >= 0
 *   mfcc           : device, frames as rows with row stride ldc >= n_mfcc - the layout evc_dtw_align takes.  Utterance u
 *                    owns the rows from sum over v < u of evc_stft_frames(L_v, fft_size, hop, center) on; an utterance
 *                    without samples (or, with center = 0, shorter than fft_size) has no frames
 *   re, im         : device or NULL (not wanted): the STFT of the same rows, row strides ldre, ldim >= nb
 * The call is fully asynchronous (no host synchronisation, nothing read back) and deterministic: the same call gives
 * bitwise the same output every time.  The number of kernel launches does not depend on n_utt: the utterances are laid
 * out as one strided frame matrix (every utterance reflect-padded on its own) and S = frames W_f runs on the matrix
 * cores in chunks of 8192 rows, so the workspace holds
 *     8 * (J1 * K1 + 8192 * J1 + 8 * min(8192, 128 * floor(255 / (J1 / 64))) * J1     table, one chunk of S, its k-slabs
 *          + hop * R + K1 + R * n_mels + R / 32 + 2 * nb + n_mfcc * n_mels + 3 * n_utt / 2 + 3 * n_mels / 2) bytes
 * up to rounding, with K1 = round_up(fft_size, 16), J1 = round_up(2 * nb, 64) and R = sum over the utterances of
 * round_up(frames_u + ceil(fft_size / hop), 32) rows: only the padded samples and the decibel values grow with the
 * batch, the contraction's buffers do not (at most 128 MiB of k-slabs).
 * Status -1: wrong struct_bytes, sr < 1, fft_size odd or < 2, hop < 1, n_mels < 1, n_mfcc outside 1 .. n_mels, not
 * 0 <= fmin < fmax <= sr / 2, amin <= 0, n_utt < 0, descending or negative offsets, ldc < n_mfcc, ldre / ldim < nb, a NULL
 * pointer that is needed; -3: n_mels > EVC_MFCC_MAX_MELS or fft_size > EVC_MFCC_MAX_FFT (what the LDS tiles of the two
 * kernels hold); -2: workspace too small.  n_utt = 0 or a call without any frame: status 0, nothing is launched.
 * Non-finite samples (librosa refuses them): the outputs of such an utterance are unspecified, the other utterances
 * of the call are unaffected. */
enum { EVC_MFCC_MAX_MELS = 256, EVC_MFCC_MAX_FFT = 8192 };
typedef struct evc_mfcc_opts {
    int struct_bytes;  /* sizeof(evc_mfcc_opts) */
    int sr;            /* sampling rate in Hz (the script: 16000) */
    int fft_size;      /* even, >= 2 (the script: 400) */
    int hop;           /* >= 1 (the script: 80) */
    int n_mels;        /* librosa: 128 */
    int n_mfcc;        /* librosa: 20 */
    int center;        /* 1: librosa's default (reflect padding), 0: frames start at sample 0 */
    int reserved;      /* 0 */
    double fmin;       /* librosa: 0 */
    double fmax;       /* 0: sr / 2 (librosa's default) */
    double amin;       /* librosa: 1e-10 */
    double top_db;     /* librosa: 80; < 0: no clamp */
} evc_mfcc_opts;
/* bytes of workspace evc_mfcc needs (0: invalid arguments) */
size_t evc_mfcc_workspace_bytes(const long* sample_offsets, int n_utt, const evc_mfcc_opts* opts);
int evc_mfcc(const void* x, const long* sample_offsets, int n_utt, const evc_mfcc_opts* opts, void* mfcc, int ldc,
             void* re, int ldre, void* im, int ldim, void* workspace, size_t workspace_bytes, evc_stream_t stream);

/* Griffin-Lim phase reconstruction - the back end that follows the path when the scripts run on
 * STFT magnitudes: reconstruct_signal_griffin_lim(), zz_audio_utilities.py:258-292 (with its
 * stft_for_reconstruction / istft_for_reconstruction, :181-218), called from synthesize2(),
 * 04_align_n_nmf.py:182-191.  float64.
 *   mag : T x (fft_size/2 + 1) magnitudes, rows are time slices, row stride ldm (device)
 *   x   : T*hop + fft_size samples (device); in: the initial signal (the reference draws
 *         np.random.randn), out: the reconstruction after `iters` iterations
 *   rmse_out (host, iters doubles or NULL): the per-iteration RMSE the reference prints; non-NULL
 *         makes the call synchronous.   fft_size must be even. */
size_t evc_griffin_lim_workspace_bytes(int T, int fft_size, int hop, int iters);
int evc_griffin_lim(const void* mag, int ldm, int T, int fft_size, int hop, int iters, void* x,
                    void* workspace, size_t workspace_bytes, double* rmse_out, evc_stream_t stream);
/* The same for a batch of utterances in one call (the reference reconstructs one file per call of
 * synthesize2(), 04_align_n_nmf.py:182-191; a batch fills the GPU, one 688-frame utterance does not).
 *   frame_offsets : host, n_utt + 1 ints, frame_offsets[0] = 0: utterance u owns rows frame_offsets[u] ..
 *                   frame_offsets[u+1]-1 of `mag` (T_u frames)
 *   x             : the signals back to back: utterance u's T_u*hop + fft_size samples start at sample
 *                   hop*frame_offsets[u] + u*fft_size (device; in: initial signals, out: reconstructions)
 *   rmse_out      : host, n_utt x iters doubles ([u][iteration]) or NULL; non-NULL makes the call synchronous
 * Every utterance's result equals that of a call of its own up to the summation order of the contractions
 * (the split of the 400-deep sums over workgroups depends on the number of rows). */
size_t evc_griffin_lim_batch_workspace_bytes(const int* frame_offsets, int n_utt, int fft_size, int hop,
                                             int iters);
int evc_griffin_lim_batch(const void* mag, int ldm, const int* frame_offsets, int n_utt, int fft_size, int hop,
                          int iters, void* x, void* workspace, size_t workspace_bytes, double* rmse_out,
                          evc_stream_t stream);

/* Dynamic-time-warping alignment of parallel utterance pairs - the step that builds the parallel
 * dictionary: _dtw_alignment(), 01_make_dict_parallel.py:215-228, i.e. the third-party call
 * dtw(feat_A.T, feat_B.T, dist=lambda x, y: sum(np.square(x - y))) (accumulated cost with steps
 * (i-1,j-1), (i-1,j), (i,j-1); trace-back with ties to the diagonal, then to i-1).  float64.
 *   A, B      : frames as rows (row strides lda, ldb), D features each; pair p owns rows
 *               a_offsets[p] .. a_offsets[p+1]-1 of A and b_offsets[p] .. of B (host arrays, n_pairs+1)
 *   path_a/b  : device int arrays of sum_p (Ta_p + Tb_p) entries; pair p's path starts at
 *               a_offsets[p] + b_offsets[p] and has path_len[p] (device, n_pairs) entries
 *   total     : device, n_pairs doubles or NULL: accumulated cost of the last cell
 *   D         : 1 .. 512 features (larger: -3);  n_pairs : 1 .. 65535 (larger: -3)
 * Frames per utterance are limited by the LDS border buffers of the tiled wavefront (7680).  A pair with an empty
 * utterance gets path_len 0 and total 0.
 * Non-finite features, or features whose squared differences overflow: the path of such a pair is unspecified, but it is
 * a valid warping path - from (0, 0) to (Ta-1, Tb-1) in steps of (1,1), (1,0), (0,1), hence at most Ta + Tb - 1 entries -
 * that stays inside the pair's part of the path buffers; its `total` is unspecified.  The other pairs of the call are
 * bitwise unaffected. */
size_t evc_dtw_workspace_bytes(const int* a_offsets, const int* b_offsets, int n_pairs);
int evc_dtw_align(const void* A, int lda, const int* a_offsets, const void* B, int ldb,
                  const int* b_offsets, int D, int n_pairs, int* path_a, int* path_b, int* path_len,
                  double* total, void* workspace, size_t workspace_bytes, evc_stream_t stream);


/* Gather of the aligned frames - align_sp_ap_f0(), 04_align_n_nmf.py:100-169, and the stacking of the aligned frames
 * into the dictionary, :230-246,320-324,350-361: the dictionary's rows are the frames the DTW paths name, pair after
 * pair.  With these two calls the paths evc_dtw_align left on the device are consumed there: the feature frames make no
 * round trip through the host, only the number of rows N (one int) comes back, because N sizes the dictionary.
 *
 * evc_dtw_path_rows: row_start[p] = first dictionary row of pair p (exclusive scan of path_len), row_start[n_pairs] = N.
 *   path_len   : device, n_pairs ints (evc_dtw_align)          row_start : device, n_pairs + 1 ints
 *   n_rows_out : host int or NULL; non-NULL makes the call synchronous (it returns N)
 * evc_dtw_gather_rows: dst[row_start[p] + k][c] = op(src[src_offsets[p] + path[pair_offsets[p] + k]][c * elem_stride])
 *   for k < path_len[p], c < cols.
 *   src          : frames as rows, row stride ld_src (elements); elem_stride = 2 picks the real parts of an interleaved
 *                  complex matrix (the script's np.abs(real(stft)), :320-324, with op = EVC_GATHER_ABS: the sign bit
 *                  cleared as np.abs does it, so -0 becomes +0 and a NaN keeps its payload)
 *   path         : device, path_a or path_b of evc_dtw_align;  pair_offsets : device, n_pairs ints, a_offsets[p] + b_offsets[p]
 *   src_offsets  : device, n_pairs ints, first row of pair p's utterance in src
 *   dst          : N x cols, row stride ld_dst;  dtype: EVC_F64 | EVC_F32 (src and dst alike) */
enum { EVC_GATHER_COPY = 0, EVC_GATHER_ABS = 1 };
int evc_dtw_path_rows(const int* path_len, int n_pairs, int* row_start, int* n_rows_out, evc_stream_t stream);
int evc_dtw_gather_rows(const void* src, long ld_src, int elem_stride, const int* path, const int* path_len,
                        const int* src_offsets, const int* pair_offsets, const int* row_start, int n_pairs, int cols,
                        int op, void* dst, long ld_dst, int dtype, evc_stream_t stream);

/* Coordinate descent - scikit-learn's solver='cd' with the dictionary fixed (update_H=False, shuffle=False), Frobenius
 * loss: for every frame the components t = 0..N-1 are visited in order and
 *     grad = (A^T A h)_t + l2 h_t - (A^T x)_t + l1,  h_t <- max(h_t - grad / (|a_t|^2 + l2), 0)
 * (components with |a_t|^2 + l2 == 0 are left alone); the sum over frames and components of the projected gradient
 * |pg| (pg = min(grad, 0) where h_t == 0, else grad) is the iteration's violation.  Per utterance, after every iteration:
 * stop when violation_init (that of iteration 1) == 0, when violation / violation_init <= tol, or at max_iter
 * (_nmf.py:496-521); the stopping iteration's update is kept.  float32 inputs are solved in float32 (the violation is
 * summed in float64 for both types); the quotient is the IEEE division.  One kernel launch per iteration (k_cd_sweep)
 * plus one that judges the last; no inter-workgroup exchange.  A frame's arithmetic does not depend on the other frames
 * of the call: a batch of utterances gives bitwise the activations of one call per utterance.
 *   M      : 1 .. 1024 bins (larger: -3)
 *   layout : EVC_FRAME_MAJOR | EVC_BIN_MAJOR, as for evc_nmf_solve (A, X, H and their leading dimensions)
 *   init   : EVC_INIT_SKLEARN - H starts at 0, what sklearn's cd starts from whatever H was passed (_nmf.py:1229-1233);
 *            EVC_INIT_GIVEN   - H holds the start on entry (a warm start)
 *   l1, l2 : already scaled: sklearn's l1_reg_W = M alpha_W l1_ratio and l2_reg_W = M alpha_W (1 - l1_ratio)
 *   n_iter_out    : host, n_utt ints or NULL: iterations run per utterance (an utterance without frames: 1)
 *   violation_out : host, n_utt x max_iter doubles ([u][i]) or NULL: violation of every iteration, NaN after the stop
 * When both are NULL the call is fully asynchronous. */
typedef struct evc_cd_opts {
    int struct_bytes;  /* sizeof(evc_cd_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int init_mode;     /* EVC_INIT_SKLEARN (zeros) | EVC_INIT_GIVEN */
    int max_iter;      /* >= 0 */
    int reserved;      /* 0 */
    double tol;        /* >= 0 */
    double l1, l2;     /* >= 0 */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_cd_opts;
/* bytes of workspace evc_cd_solve needs (0: invalid arguments) */
size_t evc_cd_workspace_bytes(int M, int N, int T, int n_utt, int dtype);
int evc_cd_solve(const void* A, int lda, const void* X, int ldx, void* H, int ldh, int M, int N, int T,
                 const int* utt_offsets, int n_utt, const evc_cd_opts* opts, void* workspace, size_t workspace_bytes,
                 int* n_iter_out, double* violation_out, evc_stream_t stream);

/* Multiplicative updates of BOTH factors, X ~ W H (Frobenius, or Kullback-Leibler on the SKLEARN surface): X is M x T, W is M x R (addressed like A of evc_nmf_solve:
 * FRAME_MAJOR W[r*ldw+m], BIN_MAJOR W[m*ldw+r]), H is R x T (addressed like H of evc_nmf_solve).  W and H hold the start on
 * entry and are updated in place.  The dictionary update is evaluated factored, V = W H, Num = X H^T, Den = V H^T (6MRT
 * flop; the R x R Gram matrix of H is never formed); the activation update is one iteration of evc_nmf_solve.
 *   SKLEARN  per iteration H first, then W:  Den[Den == 0] = 1.1920929e-7; W <- W * (Num / Den);  H by EVC_EPS_ZERO_REPLACE
 *            (sklearn's W is H^T here, its H is W^T).  err = ||X - W H||_F at the start and after every `check_every`
 *            iterations; stop when (err_prev - err) / err_at_start < tol (tol = 0 never stops)
 *   PYMF     per iteration W first, then H:  W <- (W * Num) / (Den + 1e-9), then every column divided by its Euclidean
 *            norm (a column of zeros becomes NaN, exactly as in pymf: not guarded);  H by EVC_EPS_ADD 1e-9.  From the
 *            third evaluated error on, stop when |err - err_prev| / T < tol (pymf: check_every = 1, tol = machine epsilon;
 *            the caller truncates its `ferr` as pymf/base.py:266-270 does)
 *   loss = EVC_LOSS_KL (SKLEARN surface only; with PYMF: -3, pymf has no such update): scikit-learn's beta_loss =
 *            'kullback-leibler' with update_H=True.  Per iteration H first, by one iteration of evc_nmf_solve with
 *            EVC_LOSS_KL (EVC_EPS_ZERO_REPLACE, eps 1.1920929e-7), then W with the new H:  V = W H;
 *            Q = X / max(V, 1.1920929e-7);  Num[m][r] = sum_t Q[m][t] H[r][t];  s_r = sum_t H[r][t], s_r == 0 -> 1.0
 *            (_nmf.py:679-680: 1, not eps);  W <- W * (Num / s_r)  (2MRT flop for Num; Q takes V's place in the workspace).
 *            err = sqrt(2 KL(X || W H)) as _beta_divergence(beta=1, square_root=True) computes it (a sum of per-frame terms
 *            that rounding leaves below zero is taken as zero); the checks and the stop are those of the Frobenius loss.
 *            evc_learn_workspace_bytes and evc_learn_splits do not depend on the loss.
 * Num and Den (Kullback-Leibler: Num and s_r) are sums over the frames, taken in evc_learn_splits(M, R, T) contiguous frame ranges whose partial sums are
 * added in ascending order: the count depends on the sizes only, and the same call gives bitwise the same W and H every time.
 *   M : 1 .. 1056, R : 1 .. 4096 (larger: -3);  T >= 1
 *   n_iter_out : host int or NULL: iterations carried out
 *   err_out    : host, 1 + iters / check_every doubles or NULL: the error at the start, then at every check (NaN where not
 *                evaluated)
 * Host synchronisation: case (5) of the list at the top. */
enum { EVC_LEARN_SKLEARN = 0, EVC_LEARN_PYMF = 1 };
typedef struct evc_learn_opts {
    int struct_bytes;  /* sizeof(evc_learn_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int surface;       /* EVC_LEARN_* */
    int iters;         /* >= 0 */
    int check_every;   /* 0: the error is never evaluated; k > 0: at the start and every k iterations */
    int reserved;      /* 0; bits 8..15, tuning and tests: that many frame ranges (1 .. 64) instead of evc_learn_splits();
                          anything else: status -1 */
    int loss;          /* EVC_LOSS_* (0 = Frobenius: the slot was padding before it had a name); anything else: -1 */
    double tol;        /* >= 0 */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_learn_opts;
/* bytes of workspace evc_nmf_learn needs (0: invalid arguments); room for 64 frame ranges is included */
size_t evc_learn_workspace_bytes(int M, int R, int T, int dtype);
/* frame ranges the dictionary update's sums over the frames are split into (0: invalid arguments) */
int evc_learn_splits(int M, int R, int T);
int evc_nmf_learn(const void* X, int ldx, void* W, int ldw, void* H, int ldh, int M, int R, int T,
                  const evc_learn_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out, double* err_out,
                  evc_stream_t stream);

/* Coordinate descent on BOTH factors, X ~ W H: scikit-learn's solver='cd' (its default) with update_H=True, shuffle=False
 * (_fit_coordinate_descent, _nmf.py:496-521).  X is M x T, W is M x R, H is R x T, all addressed as in evc_nmf_learn
 * (sklearn's W is H^T here, its H is W^T); W and H hold the start on entry and are updated in place.  Per iteration:
 *   activations  one sweep of evc_cd_solve's kernel from the current H on the current W (EVC_INIT_GIVEN; penalties l1_h,
 *                l2_h).  With max_iter = 1 the activations are bitwise those of evc_cd_solve(max_iter = 1, EVC_INIT_GIVEN,
 *                tol = 0) on the same inputs;
 *   dictionary   G = H H^T with l2_w added on the diagonal, P = X H^T - l1_w; for every bin row w of W the components
 *                t = 0 .. R-1 in order:  grad = G[t,:] . w - P[m][t];  w_t <- max(w_t - grad / G[t][t], 0)  (IEEE division;
 *                skipped where G[t][t] == 0);  its violation is the sum of |pg|, pg = min(grad, 0) where w_t == 0, else grad.
 *                G and P are sums over the frames, taken in evc_cd_learn_splits(M, R, T) contiguous frame ranges whose
 *                partial sums are added in ascending order;
 *   stop         violation = the sum of the two halves'; stop when violation_init (that of iteration 1) == 0, when
 *                violation / violation_init <= tol, or at max_iter.  The stopping iteration's updates are kept.
 * float32 inputs are solved in float32; every violation is summed in float64, in a fixed order.  The same call gives
 * bitwise the same W and H every time.
 *   M : 1 .. 1024, R : 1 .. 1024 (larger: -3);  T >= 1;  max_iter = 0 returns the start
 *   n_iter_out    : host int or NULL: iterations carried out
 *   violation_out : host, max_iter x 2 doubles or NULL: [i][0] the activation half's violation of iteration i + 1 (0 with
 *                   EVC_CDL_DICT_ONLY), [i][1] the dictionary half's; NaN after the stop
 * Host synchronisation: case (6) of the list at the top. */
enum { EVC_CDL_BOTH = 0, EVC_CDL_DICT_ONLY = 1 };
typedef struct evc_cd_learn_opts {
    int struct_bytes;  /* sizeof(evc_cd_learn_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int max_iter;      /* >= 0 */
    int update;        /* EVC_CDL_BOTH; EVC_CDL_DICT_ONLY: the activations stay fixed, only the dictionary half runs (and
                          only its violation counts) */
    int reserved;      /* 0; bits 8..15, tests and tuning: that many frame ranges (1 .. 64) instead of
                          evc_cd_learn_splits(), as in evc_learn_opts; more ranges than that need more workspace (below);
                          anything else: status -1 */
    double tol;        /* >= 0 */
    double l1_h, l2_h; /* >= 0; activations: sklearn's l1_reg_W, l2_reg_W (already scaled by the number of bins) */
    double l1_w, l2_w; /* >= 0; dictionary:  sklearn's l1_reg_H, l2_reg_H (already scaled by the number of frames) */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_cd_learn_opts;
/* bytes of workspace evc_cd_learn needs at evc_cd_learn_splits(M, R, T) frame ranges (0: invalid arguments).  Every forced
 * range beyond that count needs 2 * 16 * (round_up(ceil(M / 16), 4) + round_up(ceil(R / 16), 4)) * round_up(R, 128) more
 * elements (-2 otherwise). */
size_t evc_cd_learn_workspace_bytes(int M, int R, int T, int dtype);
/* frame ranges the sums over the frames (G and P) are split into (0: invalid arguments) */
int evc_cd_learn_splits(int M, int R, int T);
int evc_cd_learn(const void* X, int ldx, void* W, int ldw, void* H, int ldh, int M, int R, int T,
                 const evc_cd_learn_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out,
                 double* violation_out, evc_stream_t stream);

/* Multiplicative updates of the activations under any beta-divergence, the dictionary fixed: scikit-learn's
 * non_negative_factorization(X, H=A, init='custom', update_H=False, solver='mu', beta_loss=beta) for beta_loss =
 * 'itakura-saito' (beta = 0) or any float.  With EPS = 1.1920929e-7 (2^-23, in both element types), per iteration and frame:
 *     V  = A h;   Vd = V with values below EPS raised to EPS if beta < 1;   Vn = the same if beta < 2
 *     Q1 = x * Vn^(beta-2);   Q2 = Vd^(beta-1);   Num = A^T Q1;   Den = A^T Q2 + l1 + l2 h,  Den == 0 -> EPS
 *     h <- h * (Num / Den)^gamma,   gamma = 1/(2-beta) if beta < 1, 1/(beta-1) if beta > 2, else 1
 * beta = 1 and beta = 2 are accepted and run this generic statement; their results agree with evc_nmf_solve's
 * (EVC_LOSS_KL, and EVC_LOSS_FROBENIUS with EVC_EPS_ZERO_REPLACE) to rounding, not bitwise.
 * The error of utterance u (T_u frames), at the start and after every `check_every` iterations, is sklearn's
 * _beta_divergence(..., square_root=True) = sqrt(2 max(res, 0)): only entries with X > EPS enter the sums marked *, and
 * there V below EPS counts as EPS:
 *     beta = 0     res = sum* X/V - M T_u - sum* log(X/V)                       (M T_u counts every entry, as sklearn does)
 *     beta = 1     res = sum* (X log(X/V) - X) + sum_all V
 *     beta = 2     res = sum_all (X - V)^2 / 2
 *     otherwise    res = (sum* X^beta - beta sum* X V^(beta-1) + (beta-1) sum_all V^beta) / (beta (beta-1))
 * EVC_STOP_SKLEARN stops an utterance at a check when (err_prev - err) / err_at_start < tol; its frames are frozen while
 * the others go on.  EVC_INIT_SKLEARN starts every activation of utterance u at sqrt(mean(X_u) / N).
 * One kernel launch per iteration (k_beta_sweep): a workgroup owns 16 frames of one utterance, forms V = A H on the matrix
 * cores, turns it into Q1 | Q2 in LDS and forms Num | Den per exemplar tile; V, Q1, Q2, Num and Den never reach memory.
 * H is written once per iteration and read 1 + ceil(ceil(M / 16) / 8) times (twice up to M = 128, 6 times at M = 513).
 * float32 inputs are solved in float32; the error is summed in float64 for both types, per utterance in a fixed order (no
 * float atomics): the same call gives bitwise the same output every time.  A frame's arithmetic does not depend on the other
 * frames of the call: a batch of utterances gives bitwise the activations of one call per utterance, and a NaN or infinity
 * in a frame of X stays in that frame's column (the other frames are bitwise those of the call without it; only the
 * start of EVC_INIT_SKLEARN, the utterance's mean, carries it to the utterance's other frames, as in scikit-learn).
 * Exponents that are multiples of 1/2 (beta = 0, 0.5, 1.5, 3, ...) are evaluated with products, square roots and one
 * division, the power first and the reciprocal last (beta = 0: Q1 = x * (1 / (V V)), one rounding away from sklearn's
 * x * (1 / V)^2); the general float beta calls pow.
 *   M      : 1 .. 528 bins (larger: -3);  any N >= 1, T >= 0 (an utterance may be empty: nothing is done for it, its n_iter
 *            is `iters` and its errors stay NaN);  iters = 0 leaves the start in H
 *   beta   : any finite value (NaN, infinity: -1)
 *   l1, l2 : already scaled: sklearn's l1_reg_W = M alpha_W l1_ratio and l2_reg_W = M alpha_W (1 - l1_ratio)
 *   layout, utt_offsets, n_utt : as for evc_nmf_solve
 *   n_iter_out : host, n_utt ints or NULL: updates applied to each utterance
 *   err_out    : host, n_utt * (1 + iters / check_every) doubles or NULL, laid out like evc_nmf_solve's: per utterance the
 *                error at the start, then at each check that was evaluated (NaN where not; all NaN with check_every = 0);
 *                at most 4097 slots per utterance (more: -1)
 * Status -1 / -3 / -2 are returned before any device work.  Host synchronisation: case (8) of the list at the top. */
typedef struct evc_beta_opts {
    int struct_bytes;  /* sizeof(evc_beta_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int iters;         /* maximum number of multiplicative updates (>= 0) */
    int init_mode;     /* EVC_INIT_GIVEN | EVC_INIT_SKLEARN | EVC_INIT_CONST */
    int check_every;   /* 0: the error is never evaluated; k > 0: at the start and every k iterations */
    int stop_rule;     /* EVC_STOP_NONE | EVC_STOP_SKLEARN */
    int reserved;      /* 0 */
    double beta;       /* the divergence: 0 Itakura-Saito, 1 Kullback-Leibler, 2 Frobenius, or any finite value */
    double tol;        /* >= 0: threshold of stop_rule */
    double l1, l2;     /* >= 0 */
    double init_value; /* EVC_INIT_CONST */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_beta_opts;
/* bytes of workspace evc_beta_solve needs (0: invalid arguments, M > 528 among them) */
size_t evc_beta_workspace_bytes(int M, int N, int T, int n_utt, int dtype);
int evc_beta_solve(const void* A, int lda, const void* X, int ldx, void* H, int ldh, int M, int N, int T,
                   const int* utt_offsets, int n_utt, const evc_beta_opts* opts, void* workspace, size_t workspace_bytes,
                   int* n_iter_out, double* err_out, evc_stream_t stream);

/* Multiplicative updates of BOTH factors under any beta-divergence, X ~ W H: scikit-learn's
 * non_negative_factorization(init='custom', update_H=True, solver='mu', beta_loss=beta) for beta_loss = 'itakura-saito'
 * (beta = 0) or any float (_fit_multiplicative_update, _nmf.py:731-893).  X is M x T, W is M x R, H is R x T, all addressed
 * as in evc_nmf_learn (sklearn's W is H^T here, its H is W^T); W and H hold the start on entry and are updated in place.
 * With EPS = 1.1920929e-7 (2^-23) and E64 = 2.220446e-16 (2^-52), both in both element types, per iteration:
 *   activations  one iteration of evc_beta_solve's statement on the current W with l1_h and l2_h (the same kernel; its
 *                packed dictionary images are rebuilt from W every iteration); then, if beta < 1, H[H < E64] = 0.  With
 *                iters = 1 and beta >= 1 the activations are bitwise those of evc_beta_solve(iters = 1, EVC_INIT_GIVEN);
 *   dictionary   with the new H:  V = W H;  Vn = V with values below EPS raised to EPS if beta < 2;  Vd = the same if
 *                beta < 1;  Q1 = X * Vn^(beta-2);  Q2 = Vd^(beta-1);  Num = Q1 H^T;  Den = Q2 H^T + l1_w + l2_w W,
 *                Den == 0 -> EPS;  W <- W * (Num / Den)^gamma;  then, if beta <= 1, W[W < E64] = 0
 *                (gamma and the evaluation of the powers as in evc_beta_solve);
 *   error        evc_beta_solve's formulas with one utterance, over the whole matrix, at the start and after every
 *                `check_every` iterations; stop when (err_prev - err) / err_at_start < tol (tol = 0 never stops).
 * beta = 1 and beta = 2 are accepted and run this generic statement: they agree with evc_nmf_learn to rounding, not bitwise
 * (at beta = 1 the two flushes above are scikit-learn's, which evc_nmf_learn omits).
 * Num and Den are sums over the frames, taken in evc_beta_learn_splits(M, R, T) contiguous frame ranges whose partial sums
 * are added in ascending order: the count depends on the sizes only.  Two routes form them (evc_beta_learn_route): a fused
 * kernel for small R that forms V, Q1 and Q2 in registers and never writes them (k_beta_dict_grad), and for any R the
 * generic contraction for V, an element-wise kernel for Q1 and Q2 and evc_nmf_learn's split-T contraction.  float32 inputs
 * are solved in float32; the error is summed in float64 in a fixed order.
 *   M : 1 .. 528 (k_beta_sweep's limit; larger: -3 - stacked WORLD spectra at 1026 bins are not served), R : 1 .. 4096
 *       (larger: -3);  T >= 1;  iters = 0 returns the start, and its error if asked for
 *   beta : any finite value (NaN, infinity: -1);  tol and the four penalties >= 0 (negative or NaN: -1)
 *   l1_h, l2_h, l1_w, l2_w : already scaled, as in evc_cd_learn_opts
 *   n_iter_out : host int or NULL: iterations carried out
 *   err_out    : host, 1 + iters / check_every doubles or NULL, laid out like evc_nmf_learn's; at most 4097 slots (more: -1)
 * Status -1 / -3 / -2 are returned before any device work.  Host synchronisation: case (9) of the list at the top. */
typedef struct evc_beta_learn_opts {
    int struct_bytes;  /* sizeof(evc_beta_learn_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int iters;         /* >= 0 */
    int check_every;   /* 0: the error is never evaluated; k > 0: at the start and every k iterations */
    int reserved;      /* 0; tests and tuning: bits 8..15 that many frame ranges (1 .. 64) instead of evc_beta_learn_splits(),
                          bits 16..17 the dictionary route, 1 = fused (R > 256, which it does not hold: -3), 2 = unfused;
                          anything else: status -1 */
    double beta;       /* the divergence: 0 Itakura-Saito, 1 Kullback-Leibler, 2 Frobenius, or any finite value */
    double tol;        /* >= 0 */
    double l1_h, l2_h; /* >= 0; activations: sklearn's l1_reg_W, l2_reg_W (already scaled by the number of bins) */
    double l1_w, l2_w; /* >= 0; dictionary:  sklearn's l1_reg_H, l2_reg_H (already scaled by the number of frames) */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_beta_learn_opts;
/* bytes of workspace evc_beta_learn needs (0: invalid arguments, M > 528 among them); room for 64 frame ranges is included */
size_t evc_beta_learn_workspace_bytes(int M, int R, int T, int dtype);
/* frame ranges the dictionary half's sums over the frames are split into (0: invalid arguments) */
int evc_beta_learn_splits(int M, int R, int T);
/* the dictionary route a call with reserved = 0 takes: 1 = fused, 2 = unfused (0: invalid arguments); sizes only */
int evc_beta_learn_route(int M, int R, int T);
int evc_beta_learn(const void* X, int ldx, void* W, int ldw, void* H, int ldh, int M, int R, int T,
                   const evc_beta_learn_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out, double* err_out,
                   evc_stream_t stream);

/* Mini-batch (online) dictionary learning under any beta-divergence, X ~ W H: scikit-learn 1.7.2's
 * MiniBatchNMF(init='custom', fresh_restarts=False, beta_loss=beta).fit_transform(X, W=..., H=...) (_nmf.py: _fit_transform,
 * _minibatch_step, _multiplicative_update_h(..., A, B, rho), _minibatch_convergence).  X is M x T, W is M x R, H is R x T, all
 * addressed as in evc_beta_learn (sklearn's W is H^T here, its H is W^T); W and H hold the start on entry and are updated in
 * place.  acc_a and acc_b are the M x R accumulators A and B of the online update, addressed like W with the leading
 * dimension ld_acc, caller-owned: with resume = 0 the call sets A = W, B = 1 first; with resume = 1 they hold a previous
 * call's state.
 * Batches are contiguous ranges of bs = min(batch_size, T) frames, taken in order and cycled (sklearn's gen_batches: the
 * last of a pass may be short; nothing is shuffled).  rho = forget_factor ^ (bs / T); EPS, E64, gamma and the evaluation of
 * the powers as in evc_beta_learn.  Step k = 1, 2, ... on batch b of T_b frames:
 *   activations  one iteration of evc_beta_solve's statement on the batch's columns of H with the current W, l1_h and l2_h;
 *                then, if beta < 1, H_b[H_b < E64] = 0
 *   cost         (res + l1_h sum H_b + T_b l1_w sum W + l2_h sum H_b^2 + T_b l2_w sum W^2) / T_b with res =
 *                _beta_divergence(X_b, H_b, W, beta), neither square-rooted nor clamped at 0, W still the step's start;
 *                every sum in float64 in a fixed order
 *   dictionary   with the new H_b, Num and Den over the batch's frames exactly as evc_beta_learn's dictionary half forms
 *                them, in evc_online_splits(M, R, T_b) frame ranges, Den including T_b l1_w + T_b l2_w W, Den == 0 -> EPS;
 *                P = W^(1/gamma);  A <- rho A + Num P;  B <- rho B + Den;  W <- (A / B)^gamma;  then, if beta <= 1,
 *                W[W < E64] = 0
 *   convergence  on the host, as _minibatch_convergence: step 1 is ignored; from step 2 on ewa = cost the first time, else
 *                ewa (1 - a) + cost a with a = min(T_b / (T + 1), 1); stop if tol > 0 and ||W_new - W_old||_F / ||W_new||_F
 *                <= tol; otherwise, if ewa < ewa_min (or there is none yet) it is stored and the counter reset, else the
 *                counter counts, and the loop stops once max_no_improvement >= 0 and the counter has reached it.  The
 *                stopping step's updates are kept.
 * beta = 1 and beta = 2 run this generic statement (to rounding, not bitwise, against sklearn's special cases).  The fused /
 * unfused route of the frame sums follows evc_beta_learn_route.  The batch cycle and the convergence state restart with
 * every call: with the stop rules off, a call of p passes followed by a resume = 1 call of q passes gives bitwise the W, H, A
 * and B of one call of p + q passes.
 * transform (MiniBatchNMF._solve_W, the fixed-dictionary solve that stops on the change of its activations) is served by
 * evc_online_transform below; fresh_restarts=True and partial_fit (both put that solve inside the step) by
 * evc_online_learn_fresh.  Out of scope in all three: sparse X; shuffled batches.
 *   M : 1 .. 528, R : 1 .. 4096 (larger: -3);  T >= 1;  max_iter = 0 returns the start (and sets A and B when resume = 0)
 *   l1_h, l2_h : already scaled by the number of bins, as in evc_beta_learn_opts
 *   l1_w, l2_w : PER FRAME (sklearn's alpha_H * l1_ratio and alpha_H * (1 - l1_ratio)): the call multiplies them by T_b
 *   n_iter_out, n_steps_out : host ints or NULL: ceil(n_steps / ceil(T / bs)) and the steps carried out
 *   trace_out  : host, max_iter * ceil(T / bs) x 2 doubles or NULL: [k][0] the batch cost of step k + 1, [k][1] its change
 *                ratio ||W_new - W_old|| / ||W_new||; NaN after the stop
 * Status -1 (wrong struct_bytes, NaN or infinite beta, negative or NaN tol or penalties, forget_factor outside (0, 1],
 * batch_size < 1, max_iter < 0, max_iter * ceil(T / bs) beyond an int, resume not 0 or 1, missing pointers, bad leading
 * dimensions), -3 and -2 are returned before any device work.  Host synchronisation: case (10) of the list at the top. */
typedef struct evc_online_opts {
    int struct_bytes;        /* sizeof(evc_online_opts) */
    int dtype;               /* EVC_F64 | EVC_F32 */
    int layout;              /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int batch_size;          /* >= 1; clipped to T */
    int max_iter;            /* passes over the frames, >= 0 */
    int max_no_improvement;  /* < 0: off */
    int resume;              /* 0: A = W, B = 1 are set by the call; 1: acc_a / acc_b hold a previous call's state */
    int reserved;            /* 0; tests and tuning: bits 8..15 that many frame ranges (1 .. 64) per batch, bits 16..17 the
                                route, as in evc_beta_learn_opts; anything else: status -1 */
    double beta;             /* the divergence: 0 Itakura-Saito, 1 Kullback-Leibler, 2 Frobenius, or any finite value */
    double tol;              /* >= 0; 0: the change of W never stops the loop */
    double forget_factor;    /* in (0, 1] */
    double l1_h, l2_h;       /* >= 0; activations, already scaled by the number of bins */
    double l1_w, l2_w;       /* >= 0; dictionary, PER FRAME: multiplied by the batch's frame count */
    void* ev_loop_start;     /* optional hipEvent_t pair recorded around the launches of the step loop, as in */
    void* ev_loop_stop;      /* evc_solve_opts; NULL = not recorded */
} evc_online_opts;
/* bytes of workspace evc_online_learn needs (0: invalid arguments, M > 528 among them); room for 64 frame ranges is included,
 * and about 32 KB per batch of a pass (the activation half keeps its per-utterance state per batch) */
size_t evc_online_workspace_bytes(int M, int R, int T, int batch_size, int dtype);
/* frame ranges the dictionary half's sums over a batch of batch_frames frames are split into (0: invalid arguments);
 * evc_beta_learn_splits(M, R, batch_frames): a short last batch has its own count */
int evc_online_splits(int M, int R, int batch_frames);
int evc_online_learn(const void* X, int ldx, void* W, int ldw, void* H, int ldh, void* acc_a, void* acc_b, int ld_acc, int M,
                     int R, int T, const evc_online_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out,
                     int* n_steps_out, double* trace_out, evc_stream_t stream);

/* The activation solve of the mini-batch estimator: scikit-learn 1.7.2's MiniBatchNMF.transform(X), that is
 * MiniBatchNMF._solve_W(X, components_, transform_max_iter) (_nmf.py:2046-2071), with the dictionary W (M x R) fixed.  X is
 * M x T, H is R x T, all addressed as in evc_beta_solve (W is its A; sklearn's W is H^T here, its H is W^T).  One utterance is
 * one transform call.  Per utterance u:
 *   start      every activation at sqrt(mean(X_u) / R) (EVC_INIT_SKLEARN, what scikit-learn does; EVC_INIT_GIVEN and
 *              EVC_INIT_CONST as in evc_beta_solve)
 *   iteration  one multiplicative update, evc_beta_solve's statement with l1 and l2 (the same kernel and the same stored
 *              values: EPS, gamma and the evaluation of the powers as there); nothing is flushed to 0
 *   check      after EVERY iteration ratio = ||H_new - H_old||_F / ||H_new||_F over the utterance's frames, both sums of squares
 *              in float64 in a fixed order; if tol > 0 and ratio <= tol the utterance stops and keeps that update (a NaN
 *              ratio, 0 / 0 among them, compares false and never stops, as in numpy)
 * The ratio is formed and the stop decided on the device: per iteration one sweep launch, which also leaves every frame's
 * shares of the two sums, and one small launch that sums them per utterance; a stopped utterance's frames are frozen while
 * the others go on.  With tol = 0 the activations are bitwise those of evc_beta_solve with the same start, `max_iter`
 * iterations and check_every = 0.  A batch of utterances gives bitwise the activations, counts and ratios of one call per
 * utterance; a NaN or infinity in a frame of X stays in that frame's column, except through the utterance's start value and
 * its stop decision.  float32 inputs are solved in float32; the ratio is float64 for both types.
 *   M      : 1 .. 528 bins (larger: -3);  any R >= 1, T >= 0 (an utterance may be empty: nothing is done for it, its n_iter
 *            is max_iter and its ratios stay NaN);  max_iter = 0 leaves the start in H
 *   max_iter : 0 .. 4097, evc_beta_solve's slot limit (more: -1)
 *   l1, l2 : already scaled, as evc_beta_opts has them: sklearn's l1_reg_W = M alpha_W l1_ratio, l2_reg_W = M alpha_W (1 - l1_ratio)
 *   n_iter_out : host, n_utt ints or NULL: the iteration each utterance stopped at, or max_iter
 *   change_out : host, n_utt * max_iter doubles or NULL: [u][i] the ratio of iteration i + 1; NaN after the stop
 * Status -1 / -3 / -2 are returned before any device work.  Host synchronisation: case (11) of the list at the top. */
typedef struct evc_transform_opts {
    int struct_bytes;  /* sizeof(evc_transform_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int max_iter;      /* maximum number of multiplicative updates, 0 .. 4097 */
    int init_mode;     /* EVC_INIT_SKLEARN | EVC_INIT_GIVEN | EVC_INIT_CONST */
    int reserved;      /* 0 */
    double beta;       /* the divergence: 0 Itakura-Saito, 1 Kullback-Leibler, 2 Frobenius, or any finite value */
    double tol;        /* >= 0; 0: never stops */
    double l1, l2;     /* >= 0 */
    double init_value; /* EVC_INIT_CONST */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_transform_opts;
/* bytes of workspace evc_online_transform needs (0: invalid arguments, M > 528 among them) */
size_t evc_online_transform_workspace_bytes(int M, int R, int T, int n_utt, int dtype);
int evc_online_transform(const void* W, int ldw, const void* X, int ldx, void* H, int ldh, int M, int R, int T,
                         const int* utt_offsets, int n_utt, const evc_transform_opts* opts, void* workspace,
                         size_t workspace_bytes, int* n_iter_out, double* change_out, evc_stream_t stream);

/* evc_online_learn with scikit-learn's fresh restarts: MiniBatchNMF(init='custom', fresh_restarts=True,
 * fresh_restarts_max_iter=fresh_max_iter, transform_max_iter=final_max_iter).fit_transform(X, W=..., H=...) (_nmf.py:2082-2083,
 * :2307-2308).  Arguments, batches, rho, accumulators, cost, dictionary half, convergence rule, statuses and outputs are
 * evc_online_learn's; the caller's H is ignored as a start (as in scikit-learn) and receives the result.  What differs,
 * step k on batch b:
 *   activations  evc_online_transform's solve on the batch as one utterance against the current W: every activation of the
 *                batch starts at sqrt(mean(X_b) / R), up to fresh_max_iter updates with l1_h and l2_h, stopped on the device
 *                once tol > 0 and ||H_new - H_old||_F / ||H_new||_F <= tol over the batch; nothing is flushed during the
 *                solve (an entry flushed mid-solve could never recover); then, if beta < 1, H_b[H_b < E64] = 0 in a pass
 *                of its own
 * and after the loop, if final_max_iter > 0, one such solve over ALL frames as one utterance (start sqrt(mean(X) / R), the
 * ratio over all frames, up to final_max_iter updates, no flush) against the final W: the H the call returns.
 * One step with batch_size >= T, max_iter = 1, final_max_iter = 0, max_no_improvement < 0 and resume = 1 from the second call
 * on is MiniBatchNMF.partial_fit on that chunk (forget_factor then is scikit-learn's rho itself: the exponent is 1).
 *   fresh_max_iter : 1 .. 4097;  final_max_iter : 0 .. 4097 (outside: -1)
 * Host synchronisation: case (12) of the list at the top. */
typedef struct evc_online_fresh_opts {
    int struct_bytes;        /* sizeof(evc_online_fresh_opts) */
    int dtype;               /* the next seven as in evc_online_opts */
    int layout;
    int batch_size;
    int max_iter;
    int max_no_improvement;
    int resume;
    int reserved;
    int fresh_max_iter;      /* updates of a step's activation solve at most (sklearn's fresh_restarts_max_iter) */
    int final_max_iter;      /* updates of the solve over all frames that ends the fit (sklearn's transform_max_iter); 0: none */
    double beta;             /* as in evc_online_opts */
    double tol;              /* >= 0; stops the loop on the change of W AND every activation solve on the change of H; 0: neither */
    double forget_factor;
    double l1_h, l2_h;
    double l1_w, l2_w;
    void* ev_loop_start;
    void* ev_loop_stop;
} evc_online_fresh_opts;
/* bytes of workspace evc_online_learn_fresh needs (0: invalid arguments): evc_online_learn's plus the final solve's */
size_t evc_online_fresh_workspace_bytes(int M, int R, int T, int batch_size, int dtype);
int evc_online_learn_fresh(const void* X, int ldx, void* W, int ldw, void* H, int ldh, void* acc_a, void* acc_b, int ld_acc,
                           int M, int R, int T, const evc_online_fresh_opts* opts, void* workspace, size_t workspace_bytes,
                           int* n_iter_out, int* n_steps_out, double* trace_out, evc_stream_t stream);

/* The activation solve with multi-frame exemplars (non-negative spectrogram deconvolution): exemplar n is a segment of `taps`
 * consecutive aligned frames, tap tau of the dictionary is the M x N matrix A_tau of the segments' frames tau, and one
 * activation places the whole segment.  Utterance u has frames 0 .. T_u - 1 (utt_offsets as in evc_beta_solve); nothing crosses
 * an utterance boundary.  With L = taps and EPS = 1.1920929e-7 (2^-23, in both element types), one iteration is
 *     V[:, t]   = sum_{tau <= min(L-1, t)} A_tau H[:, t - tau]
 *     Frobenius : Q = X;                Num[n, t] = sum_{tau: t + tau < T_u} A_tau[:, n] . Q[:, t + tau]
 *                                       Den[n, t] = sum_{tau: t + tau < T_u} A_tau[:, n] . V[:, t + tau]
 *     KL        : Q = X / max(V, EPS);  Num as above;  Den[n, t] = sum_{tau: t + tau < T_u} sum_m A_tau[m, n]
 *     Den += l1 + l2 h;  Den == 0 -> EPS;  h <- h * (Num / Den)
 * With one tap this is scikit-learn's multiplicative update with the dictionary fixed (update_H=False, beta_loss 2 or 1).
 * The error of utterance u, at the start and after every `check_every` iterations, is evc_beta_solve's for beta = 2 and
 * beta = 1: ||X - V||_F, or sqrt(2 max(sum* (X log(X / max(V, EPS)) - X) + sum_all V, 0)) with sum* over the entries with
 * X > EPS.  EVC_STOP_SKLEARN stops an utterance at a check when (err_prev - err) / err_at_start < tol; its frames are frozen
 * while the others go on.  EVC_INIT_SKLEARN starts every activation of utterance u at sqrt(mean(X_u) / N).
 * Two launches per iteration over tiles of 16 frames (an utterance starts a tile of its own): k_deconv_v forms V on the
 * matrix cores and writes the images Qn = Q and Qd (V, or 1 under KL: the constant denominator is the same contraction over
 * ones), exact zeros beyond the utterance's end - that is what truncates the sums; k_deconv_update loads its tile's and the
 * next tile's images (32 frame columns, hence at most 16 taps), forms Num | Den per exemplar tile and updates H in place.  V
 * passes through memory, so no workgroup reads activations another one writes in the same launch.  A check is k_deconv_v once
 * more, leaving every frame's share of the error in float64, and a per-utterance sum in a fixed order (no float atomics): the
 * same call gives bitwise the same output every time, and a batch gives bitwise the activations, counts and errors of one
 * call per utterance.  A NaN in a frame spreads over its own utterance (the model couples neighbouring frames) and leaves
 * every other utterance bitwise unchanged.  float32 inputs are solved in float32; the errors are float64 for both types.
 *   A, lda, tap_stride : tap tau is the matrix at A + tau * tap_stride elements, addressed with lda and layout exactly like
 *            evc_beta_solve's A (tap_stride >= 0; taps may overlap in memory)
 *   M : 1 .. 256 bins, taps : 1 .. 16 (larger: -3);  any N >= 1, T >= 0 (an utterance may be empty: nothing is done for it, its
 *            n_iter is `iters` and its errors stay NaN);  iters = 0 leaves the start in H
 *   l1, l2 : >= 0, added to the denominator as in evc_beta_solve
 *   n_iter_out, err_out : host, as in evc_beta_solve (at most 4097 error slots per utterance; more: -1)
 * Status -1 (wrong struct_bytes, NaN or negative tol or penalties, taps < 1, bad enums, too many error slots), then -3 (beyond
 * the limits), then -2 (workspace too small), all before any device work.  Host synchronisation: case (13) of the list at
 * the top. */
typedef struct evc_deconv_opts {
    int struct_bytes;  /* sizeof(evc_deconv_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int loss;          /* EVC_LOSS_FROBENIUS | EVC_LOSS_KL */
    int taps;          /* frames per exemplar, 1 .. 16 */
    int iters;         /* maximum number of multiplicative updates (>= 0) */
    int init_mode;     /* EVC_INIT_GIVEN | EVC_INIT_SKLEARN | EVC_INIT_CONST */
    int check_every;   /* 0: the error is never evaluated; k > 0: at the start and every k iterations */
    int stop_rule;     /* EVC_STOP_NONE | EVC_STOP_SKLEARN */
    int reserved;      /* 0 */
    double tol;        /* >= 0: threshold of stop_rule */
    double l1, l2;     /* >= 0 */
    double init_value; /* EVC_INIT_CONST */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_deconv_opts;
/* bytes of workspace evc_deconv_solve needs (0: invalid or unsupported arguments, M > 256 and taps > 16 among them) */
size_t evc_deconv_workspace_bytes(int M, int N, int T, int n_utt, int taps, int dtype);
int evc_deconv_solve(const void* A, int lda, long tap_stride, const void* X, int ldx, void* H, int ldh, int M, int N, int T,
                     const int* utt_offsets, int n_utt, const evc_deconv_opts* opts, void* workspace, size_t workspace_bytes,
                     int* n_iter_out, double* err_out, evc_stream_t stream);
/* Y[:, t] = sum_{tau <= min(taps - 1, t)} B_tau H[:, t - tau] per utterance, on the matrix cores: B_tau (Mb x N) at
 * B + tau * tap_stride elements, B, H and Y addressed as in evc_synthesize, one launch per utterance that has frames, straight
 * from and to the caller's memory (no workspace).  Mb : 1 .. 1056, taps : 1 .. 16 (larger: -3); invalid arguments: -1. */
int evc_deconv_synthesize(const void* B, int ldb, long tap_stride, const void* H, int ldh, void* Y, int ldy, int Mb, int N, int T,
                          const int* utt_offsets, int n_utt, int taps, int layout, int dtype, evc_stream_t stream);

/* Convolutive NMF (NMFD): the multi-frame model of evc_deconv_solve learnt in BOTH factors, X ~ sum_tau W_tau shift_tau(H), one
 * dictionary of R components and L = taps taps for all utterances.  X is M x T, W_tau M x R, H R x T; utterance u owns the
 * frames utt_offsets[u] .. utt_offsets[u + 1] - 1 and nothing crosses an utterance boundary.  EPS = 2^-23 in both element
 * types.  With Hs_tau[r, t] = H[r, t - tau] where t - tau lies in t's utterance, else 0, one iteration is scikit-learn's order:
 *   1. activations: one iteration of evc_deconv_solve's statement with A_tau = W_tau and the penalties l1_h, l2_h (with
 *      iters = 1 H is bitwise evc_deconv_solve's after one iteration from the same start);
 *   2. dictionary, every tap from the same V[:, t] = sum_tau W_tau Hs_tau[:, t] of the new H:
 *        Frobenius : Num_tau = X Hs_tau^T, Den_tau = V Hs_tau^T, Den == 0 -> EPS, W_tau <- W_tau * (Num_tau / Den_tau)
 *        KL        : Q = X / max(V, EPS), Num_tau = Q Hs_tau^T, s_tau[r] = sum_t Hs_tau[r, t], s == 0 -> 1,
 *                    W_tau <- W_tau * (Num_tau / s_tau[r])
 *      (the multiplicative update of the stacked M x LR dictionary under the stacked shifted activations: the error never
 *      rises; no flush of tiny entries, no dictionary penalties, no normalisation).
 * EVC_DCL_DICT_ONLY skips step 1: H is only read (target taps fitted to target frames under the source's activations).
 * The error is one value for the call - ||X - V||_F, or sqrt(2 max(sum* (X log(X / max(V, EPS)) - X) + sum V, 0)) with sum*
 * over the entries with X > EPS - evaluated at the start and after every check_every iterations, summed from per-frame shares
 * in float64 in a fixed order; the loop stops when (err_prev - err) / err_at_start < tol (tol = 0: never).
 * Kernels: the activation half is k_deconv_v + k_deconv_update on the current W (its two packed tap images are repacked every
 * iteration); V, Q and the error shares come from k_deconv_v (EVC_DCL_DICT_ONLY: from k_deconv_learn_v, which forms V in groups
 * of 8 bin tiles straight from the caller's W, so that M may reach 1056); k_deconv_dict_grad contracts k_deconv_v's tile images
 * with the shifted, masked rows of H on the matrix cores over S ranges of frame tiles and leaves one slab of sums per range and
 * tap; k_deconv_dict_apply adds the slabs in the order s = 0 .. S-1 and updates the caller's W_tau in place.  No exchange
 * between workgroups inside a launch, no float atomics, no residency assumption: the same call gives bitwise the same W and H.
 *   X, H, W : addressed as in evc_nmf_learn; tap tau of W is the matrix at W + tau * tap_stride elements.  W and H hold the
 *            start on entry and are updated in place (EVC_DCL_DICT_ONLY: H is untouched).  The taps are written, so they must
 *            not overlap: with taps > 1, a tap_stride smaller than one tap's extent is -1
 *   taps : 1 .. 16;  R : 1 .. 4096;  M : 1 .. 256 (EVC_DCL_BOTH) or 1 .. 1056 (EVC_DCL_DICT_ONLY);  beyond: -3.  T >= 1 in all;
 *            single utterances may be empty (nothing is done for them)
 *   n_iter_out : host, the iterations carried out;  err_out : host, 1 + iters / check_every doubles, NaN where not evaluated
 *            (at most 4097 slots; more: -1)
 * S = evc_deconv_learn_splits(...) depends on the sizes only; the slabs of one launch stay within 128 MiB: S drops, down to 1,
 * when taps * M * R is large, and beyond that the taps are contracted and applied a few at a time.
 * Status: every -1 first, then -3, then -2, all before any device work.  Host synchronisation: as evc_nmf_learn's, case (5) of
 * the list at the top - one double is read back per evaluated check; without checks the call is a pure enqueue. */
enum { EVC_DCL_BOTH = 0, EVC_DCL_DICT_ONLY = 1 };
typedef struct evc_deconv_learn_opts {
    int struct_bytes;  /* sizeof(evc_deconv_learn_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int loss;          /* EVC_LOSS_FROBENIUS | EVC_LOSS_KL */
    int taps;          /* frames per component, 1 .. 16 */
    int iters;         /* maximum number of iterations (>= 0) */
    int check_every;   /* 0: the error is never evaluated; k > 0: at the start and every k iterations */
    int update;        /* EVC_DCL_BOTH | EVC_DCL_DICT_ONLY */
    int reserved;      /* 0; bits 8..15: forced number of frame ranges 1..64 (tests and tuning; lowered to what the slab cap
                          allows); anything else: -1 */
    double tol;        /* >= 0 */
    double l1_h, l2_h; /* >= 0: the activation half's penalties */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_deconv_learn_opts;
/* bytes of workspace evc_deconv_learn needs (0: invalid or unsupported arguments: wherever the call would return -1 or -3 for
 * these sizes) */
size_t evc_deconv_learn_workspace_bytes(int M, int R, int T, int n_utt, int taps, int update, int dtype);
/* frame ranges of the dictionary half's sums, 1 .. 64: a function of the sizes only (0: invalid sizes) */
int evc_deconv_learn_splits(int M, int R, int T, int n_utt, int taps);
int evc_deconv_learn(const void* X, int ldx, void* W, int ldw, long tap_stride, void* H, int ldh, int M, int R, int T,
                     const int* utt_offsets, int n_utt, const evc_deconv_learn_opts* opts, void* workspace,
                     size_t workspace_bytes, int* n_iter_out, double* err_out, evc_stream_t stream);

/* Semi-NMF activations with the dictionary fixed (Ding, Li and Jordan 2010; pymf snmf.py:66-85 with compute_w=False): X (M x T)
 * and A (M x N) are SIGNED, only H (N x T, a non-negative start) is constrained.  With pos(m) = (|m| + m) / 2 and
 * neg(m) = (|m| - m) / 2, formed as written (absolute value, add, halve; a NaN propagates), per iteration:
 *     P  = A^T X (N x T);   G = A^T A (N x N)          - both fixed while A is: formed once per call
 *     H1 = pos(P) + neg(G) H;   H2 = (neg(P) + pos(G) H) + eps
 *     H  <- H * sqrt(H1 / H2)
 * neg(G) H and pos(G) H are two sums of non-negative products of their own (never (|G| H -+ G H) / 2): H1 stays >= 0, exact
 * zeros stay exact, H1 == 0 gives H = 0, which is absorbing.  eps = 0 is accepted and may give 0 / 0 = NaN, as in pymf.
 * The error of utterance u (T_u frames), at the start and after every `check_every` iterations, is ||X_u - A H_u||_F.
 * EVC_STOP_PYMF stops an utterance at check c >= 3 when |err_c - err_(c-1)| / T_u < tol (pymf: check_every = 1,
 * tol = 2.22e-16: base.py:189-206, 266-270); its frames are frozen while the others go on.
 * One kernel launch per iteration (k_semi_sweep): a workgroup owns 128 exemplar rows x 64 frames (64 rows where that
 * would leave compute units empty: decided from N and T alone, and no output's bits depend on it), streams G and H over all
 * of N in ascending order through LDS, splits every fragment of G into pos and neg in registers and feeds two accumulators
 * per output on the matrix cores; the update is its epilogue.  H' goes to a second buffer and the two swap; whatever the
 * parity of `iters`, the result ends in H with the caller's strides and nothing outside H's N x T elements is written.
 * The order of every sum depends on N only: no split over k, no float atomics, no exchange between workgroups, no
 * residency assumption.  The same call gives the same bits; a batch gives bitwise the activations, counts and errors of one
 * call per utterance; a NaN or infinity in a frame of X stays in that frame's column (a NaN in A reaches every activation).
 * float32 inputs are solved in float32; the errors are summed in float64, per utterance in a fixed order.
 *   M      : 1 .. 1056 bins, N : 1 .. 16384 exemplars (larger: -3); T >= 0 (an utterance may be empty: nothing is done for
 *            it, its n_iter is `iters` and its errors stay NaN);  iters = 0 leaves the start in H
 *   init_mode : EVC_INIT_GIVEN (H holds the start) | EVC_INIT_CONST (every activation starts at init_value)
 *   layout, leading dimensions, utt_offsets, n_utt, n_iter_out, err_out : as for evc_beta_solve (at most 4097 error slots per
 *            utterance; more: -1)
 * The workspace holds G (round_up(N, 128)^2 elements: 2 GiB at N = 16384 in float64), P, the second H, A H at a check, the
 * stop state and the error trace: ask evc_semi_workspace_bytes.
 * Status -1 / -3 / -2 are returned before any device work.  Host synchronisation: as evc_beta_solve, case (8) of the list at
 * the top: n_iter_out / err_out non-NULL (the call returns after copying them back); otherwise the call is a pure enqueue,
 * the stop is decided on the device; concurrent calls on several streams are safe. */
typedef struct evc_semi_opts {
    int struct_bytes;  /* sizeof(evc_semi_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int iters;         /* maximum number of updates (>= 0) */
    int init_mode;     /* EVC_INIT_GIVEN | EVC_INIT_CONST */
    int check_every;   /* 0: the error is never evaluated; k > 0: at the start and every k iterations */
    int stop_rule;     /* EVC_STOP_NONE | EVC_STOP_PYMF */
    int reserved;      /* 0 */
    double eps;        /* >= 0, added to H2 (pymf: 1e-9) */
    double tol;        /* >= 0: threshold of stop_rule */
    double init_value; /* EVC_INIT_CONST */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_semi_opts;
/* bytes of workspace evc_semi_solve needs (0: invalid or unsupported arguments, M > 1056 and N > 16384 among them) */
size_t evc_semi_workspace_bytes(int M, int N, int T, int n_utt, int dtype);
int evc_semi_solve(const void* A, int lda, const void* X, int ldx, void* H, int ldh, int M, int N, int T,
                   const int* utt_offsets, int n_utt, const evc_semi_opts* opts, void* workspace, size_t workspace_bytes,
                   int* n_iter_out, double* err_out, evc_stream_t stream);

/* Convex NMF (Ding, Li and Jordan 2010; pymf cnmf.py:97-175): X ~ (X G) H with X (M x T) SIGNED, G (T x R) and H (R x T)
 * non-negative, so that the R atoms W = X G are non-negative combinations of the T exemplars (columns of X) themselves.
 * With pos(m) = (|m| + m) / 2 and neg(m) = (|m| - m) / 2, formed as written, and K = X^T X (T x T, once per call), per
 * iteration:
 *     Np = pos(K) G;  Nn = neg(K) G                                                  (T x R each; Gram sweep 1)
 *     update H:  Sp = G^T Np;  Sn = G^T Nn  (R x R);
 *                Ha = Np + H^T Sn;  Hb = (Nn + H^T Sp) + eps;  H^T <- H^T * sqrt(Ha / Hb)
 *     update G (with the new H; Np, Nn of the old G):  C = H H^T  (R x R);
 *                Wa = pos(K) H^T + Nn C;  Wb = (neg(K) H^T + Np C) + eps;  G <- G * sqrt(Wa / Wb)      (Gram sweep 2)
 * pymf's T x T product H^T G^T is never formed: H^T (G^T Nn) has an R x R matrix in the middle, and every term is a sum of
 * non-negative products.  pos(K) B and neg(K) B are two sums of non-negative products of their own (never
 * (|K| B -+ K B) / 2): exact zeros of G and H stay exact.  eps = 0 is accepted and may give 0 / 0 = NaN, as in pymf.
 * The error, at the start and after every `check_every` iterations, is ||X - (X G) H||_F (float64 residuals, a fixed
 * summation order); from the third evaluated error after the start on, the loop stops when |err - err_prev| / T < tol,
 * decided on the device (pymf: check_every = 1, tol = 2.22e-16; base.py:189-206, cnmf.py:172-175; tol = 0 never stops, a
 * NaN error compares false and runs on).  The stopping iteration's updates are kept.
 * k_convex_sweep forms [pos(K) B, neg(K) B] for B = G and B = H^T: a workgroup of W wavefronts owns 16 W rows x 64 columns,
 * streams K (symmetric: rows read as columns) and B over k ascending through LDS, splits every fragment of K in registers
 * and feeds two accumulators per output on the matrix cores.  Where R is too small to fill the chip k is split into S
 * contiguous ranges (at most 16, of at least 64 exemplars) whose partial sums go to the workspace and are added in ascending
 * order, and where that is not enough the row blocks narrow (W = 8, 4, 2): W and S are functions of (T, R) alone
 * (evc_convex_splits tells S), there are no float atomics, and the same call gives the same bits every time.  With S = 1 sweep 2's epilogue applies the update of G (each element is
 * read and written by one lane, and the sweep streams H^T, never G, so G is updated where it stands).
 *   X, H, W : addressed as in evc_nmf_learn (W is M x R); G is T x R, a row per exemplar: G[t * ldg + r], ldg >= R
 *   G, H    : the non-negative start on entry, updated in place; nothing outside their logical elements is written
 *   W       : NULL, or receives X G of the returned G (iters = 0: the only thing written)
 *   M : 1 .. 1056, T : 1 .. 16384, R : 1 .. min(T, 1024) (larger: -3)
 *   n_iter_out : host int or NULL: iterations carried out
 *   err_out    : host, 1 + iters / check_every doubles or NULL (at most 4097 slots; more: -1): the error at the start, then at
 *                every check (NaN where not evaluated)
 * float32 inputs are learnt in float32; the errors are summed in float64.  The workspace holds K (round_up(T, 128)^2
 * elements: 2 GiB at T = 16384 in float64), four T x R and two R x R arrays, the k-ranges' partial sums and the check's
 * products: ask evc_convex_workspace_bytes (a forced S beyond evc_convex_splits needs 2 T R elements more per range).
 * The three R x R products that contract over all of T (G^T Np, G^T Nn, H H^T) are split over k as well, into ranges that
 * depend on (T, R) alone and are added in ascending order.
 * Status -1 / -3 / -2 are returned before any device work.  Host synchronisation: as evc_semi_solve. */
enum { EVC_CONVEX_BOTH = 0, EVC_CONVEX_H_ONLY = 1, EVC_CONVEX_G_ONLY = 2 };
typedef struct evc_convex_opts {
    int struct_bytes;  /* sizeof(evc_convex_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int iters;         /* >= 0 */
    int check_every;   /* 0: the error is never evaluated; k > 0: at the start and every k iterations */
    int update;        /* EVC_CONVEX_* */
    int reserved;      /* 0; bits 8..15, tuning and tests: that many k-ranges (1 .. 16) instead of evc_convex_splits();
                          bits 16..23, likewise: 8, 4 or 2 wavefronts (128, 64 or 32 rows) per workgroup of the sweeps;
                          anything else: status -1 */
    double tol;        /* >= 0 */
    double eps;        /* >= 0, added to Hb and Wb (pymf: 1e-9) */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_convex_opts;
/* bytes of workspace evc_convex_learn needs (0: invalid or unsupported sizes, wherever the call would return -1 or -3) */
size_t evc_convex_workspace_bytes(int M, int R, int T, int dtype);
/* k-ranges the Gram sweeps are split into, 1 .. 16: a function of the sizes only (0: invalid or unsupported sizes) */
int evc_convex_splits(int R, int T);
int evc_convex_learn(const void* X, int ldx, void* G, int ldg, void* H, int ldh, void* W, int ldw, int M, int R, int T,
                     const evc_convex_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out, double* err_out,
                     evc_stream_t stream);

/* Sparse activations by proximal gradient (ISTA / FISTA; deComP lasso.py:97-189, 228-256, 274-297, 331-357, 388-415 and
 * math_utils/eigen.py:9-20):   min_h  1/2 ||x - A h||^2 + sum_n lambda_n h_n,   h >= 0 (EVC_PROX_POSITIVE) or h signed
 * (EVC_PROX_SIGNED), every frame on its own.  X (M x T) and A (M x N) may be signed.  Once per call, on the device:
 *     G = A^T A (N x N);   P = A^T X (N x T)
 *     normalize != 0 (deComP):  d_n = sqrt(G_nn);  G <- G / (d d^T);  P_n <- P_n / d_n;  lambda_n = alpha M / d_n;
 *                               tol_n = tol d_n;  the start is multiplied by d_n and the result divided by it at the end
 *     normalize == 0:           the problem as given: lambda_n = alpha, tol_n = tol, d = 1
 *     L = max_n sum_k |G_kn| (Gershgorin; a device reduction in a fixed order), or `lipschitz` when that is > 0;
 *     s = 1 / L;  thr_n = s lambda_n
 * Per iteration i = 0, 1, ..., with W_0 = X_0 (the start):
 *     V     = W + s (P - G W)
 *     X_new = max(V - thr, 0)                      (EVC_PROX_POSITIVE)
 *           = sign(V) max(|V| - thr, 0)            (EVC_PROX_SIGNED)
 *     W'    = X_new + c_i (X_new - X_old)
 * c_i = 0 (EVC_PROX_ISTA);  (beta_i - 1) / beta_(i+1) with beta_(i+1) = (1 + sqrt(1 + 4 beta_i^2)) / 2, beta_0 = 1
 * (EVC_PROX_FISTA);  i / (i + 3) (EVC_PROX_NESTEROV, deComP's acc_ista) - computed on the host in double precision.
 * A NaN propagates through the thresholds as numpy's maximum does.  Activations that the threshold cuts are exactly 0.
 * At iterations with i % check_every == 0 the statistic max(|X_new - X_old| - tol_n) over the utterance's frames and all n
 * is recorded in change_out; under EVC_STOP_DECOMP the utterance stops when it is < 0 (a NaN compares false: it runs on).
 * The result of a stopped utterance is X_new of that iteration; its frames are frozen while the others run on, and its
 * n_iter is i + 1, the updates applied (deComP returns i).  deComP takes the maximum over the whole call: ours equals one
 * deComP call per utterance.
 * One kernel launch per iteration (k_prox_sweep): a workgroup owns 128 exemplar rows x 64 frames (64 rows where that
 * would leave compute units empty: decided from N and T alone, and no output's bits depend on it), streams G and W over
 * all of N in ascending order through LDS into one accumulator per output on the matrix cores; the threshold, the momentum
 * and the per-frame share of the stop statistic are its epilogue.  X is updated in place in H with the caller's strides, W
 * alternates between two workspace buffers.  No split over k, no float atomics, no exchange between workgroups, no
 * residency assumption: the same call gives the same bits; a batch gives bitwise the activations, counts and statistics of
 * one call per utterance; a NaN or infinity in a frame of X stays in that frame's column (a NaN in A reaches every
 * activation).  float32 inputs are solved in float32.
 *   M      : 1 .. 1056 bins, N : 1 .. 16384 exemplars (larger: -3); T >= 0 (an empty utterance: nothing is done for it, its
 *            n_iter is `iters`);  iters = 0 leaves the start in H (EVC_INIT_CONST: init_value), neither scaled nor unscaled
 *   init_mode : EVC_INIT_GIVEN (H holds the start) | EVC_INIT_CONST (every activation starts at init_value; deComP: 0)
 *   layout, leading dimensions, utt_offsets, n_utt, n_iter_out : as for evc_semi_solve
 *   change_out : NULL or [n_utt][slots] doubles, slots = (iters - 1) / check_every + 1 (0 when iters or check_every is 0;
 *            at most 4097, more: -1): the statistic of every check that was evaluated, NaN elsewhere
 * The workspace holds G (round_up(N, 128)^2 elements), P, the two W buffers, the per-exemplar vectors, the per-frame shares
 * of the statistic and the stop state: ask evc_prox_workspace_bytes.
 * Status -1 / -3 / -2 are returned before any device work.  Host synchronisation: as evc_semi_solve. */
enum { EVC_PROX_POSITIVE = 0, EVC_PROX_SIGNED = 1 };
enum { EVC_PROX_ISTA = 0, EVC_PROX_FISTA = 1, EVC_PROX_NESTEROV = 2 };
typedef struct evc_prox_opts {
    int struct_bytes;  /* sizeof(evc_prox_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int iters;         /* maximum number of updates (>= 0; deComP: maxiter) */
    int mode;          /* EVC_PROX_POSITIVE | EVC_PROX_SIGNED */
    int momentum;      /* EVC_PROX_ISTA | EVC_PROX_FISTA | EVC_PROX_NESTEROV */
    int normalize;     /* 0 | 1: solve in deComP's unit-norm scaling of the exemplars */
    int check_every;   /* 0: the change is never evaluated; k > 0: at iterations 0, k, 2k, ... (deComP: 10) */
    int stop_rule;     /* EVC_STOP_NONE | EVC_STOP_DECOMP */
    int init_mode;     /* EVC_INIT_GIVEN | EVC_INIT_CONST */
    int reserved;      /* 0 */
    int reserved2;     /* 0 */
    double alpha;      /* >= 0: the penalty (normalize: per bin, as deComP's 1 / (2 M) scaling of the squared error) */
    double tol;        /* >= 0: threshold of stop_rule */
    double init_value; /* EVC_INIT_CONST */
    double lipschitz;  /* > 0: used as L instead of the Gershgorin bound; 0: the bound */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_prox_opts;
/* bytes of workspace evc_prox_solve needs (0: invalid or unsupported arguments, M > 1056 and N > 16384 among them) */
size_t evc_prox_workspace_bytes(int M, int N, int T, int n_utt, int dtype);
int evc_prox_solve(const void* A, int lda, const void* X, int ldx, void* H, int ldh, int M, int N, int T,
                   const int* utt_offsets, int n_utt, const evc_prox_opts* opts, void* workspace, size_t workspace_bytes,
                   int* n_iter_out, double* change_out, evc_stream_t stream);

/* evc_prox_solve with a weight per bin of every frame (missing data; deComP lasso.py:120-189, 259-271, 306-328, 418-445),
 * on a factored sweep that never forms A^T A:
 *     min_h  1/2 sum_m mask_m (x_m - (A h)_m)^2 + sum_n lambda_n h_n      per frame, mask >= 0 (a zero: the bin is missing)
 * `mask` has X's dtype, layout and shape (M x T) with its own leading dimension ldm; NULL means every weight is 1 - the
 * unmasked problem of evc_prox_solve on the factored sweep, which does 4 M N flop per frame and iteration instead of
 * 2 N^2.  Once per call, on the device:
 *     normalize != 0 (deComP):  d_n = sqrt(sum_m A_mn^2) from the UNMASKED A;  A <- A / d;  tol_n = tol d_n;
 *                               cnt_t = sum_m mask_mt (M without a mask);  lambda_tn = (alpha / d_n) cnt_t;
 *                               the start is multiplied by d_n and the result divided by it at the end
 *     normalize == 0:           the problem as given: d = 1, lambda_tn = alpha (no cnt_t), tol_n = tol
 *     wbar_m = the mean (EVC_PROX_LIP_MEAN, deComP) or the maximum (EVC_PROX_LIP_MAX) of mask_mt over the utterance's frames;
 *     L_u = max_n sum_k | sum_m A_mk wbar_m A_mn | (Gershgorin), or `lipschitz` when that is > 0;  s_u = 1 / L_u
 *     P = A^T (mask . X)
 * The mean is deComP's choice and no upper bound of a single frame's curvature A^T diag(mask_t) A; the maximum is one.
 * Per iteration i, with W_0 = X_0:
 *     R = mask . (A W);   V = W + s_u (P - A^T R);   X_new = threshold(V, s_u lambda_tn);   W' = X_new + c_i (X_new - X_old)
 * Thresholds, momentum schedules, the statistic max(|X_new - X_old| - tol_n) at i % check_every == 0, the freezing of
 * stopped utterances, n_iter = i + 1 and the NaN rules are evc_prox_solve's.  wbar, s and the statistic are per utterance:
 * a call equals one deComP call per utterance.  An utterance whose mask is all zero has L = 0 and gets what that arithmetic
 * gives (NaN), inside that utterance only.  Negative weights are not looked for.
 * Two launches per iteration on k_prox_sweep's slab loop (16-deep k-slabs double-buffered in LDS, 16x16x4 MFMAs, one
 * accumulator per output, k ascending over the whole contraction): k_prox_resid contracts over N and stores R (M x T),
 * k_prox_back contracts over M and carries evc_prox_solve's epilogue.  Every reduction - cnt, wbar, the column sums, their
 * maximum, the statistic - runs in an order fixed by the sizes and by a frame's position inside its utterance: no float
 * atomics, no split contractions; a batch gives bitwise the activations, counts and statistics of one call per
 * utterance, and a NULL mask the bits of a mask of ones.  A NaN in a frame of X stays in that frame's column; a NaN in a
 * frame of the mask does too when `lipschitz` is given (through wbar it reaches its utterance's step, as in deComP).
 *   sizes, layouts, leading dimensions, utt_offsets, init_mode, n_iter_out, change_out : as for evc_prox_solve
 * The workspace holds the scaled dictionary in both orientations (zero-padded), P, the two W buffers, R and mask . X
 * (M x T each), per utterance the column sums (N) and wbar (M), and the per-frame state: it grows as N (M + T) and holds
 * nothing N x N.  Ask evc_prox_masked_workspace_bytes.
 * Status -1 / -3 / -2 are returned before any device work.  Host synchronisation: as evc_semi_solve. */
enum { EVC_PROX_LIP_MEAN = 0, EVC_PROX_LIP_MAX = 1 };
typedef struct evc_prox_masked_opts {
    int struct_bytes;  /* sizeof(evc_prox_masked_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int iters;         /* maximum number of updates (>= 0; deComP: maxiter) */
    int mode;          /* EVC_PROX_POSITIVE | EVC_PROX_SIGNED */
    int momentum;      /* EVC_PROX_ISTA | EVC_PROX_FISTA | EVC_PROX_NESTEROV */
    int normalize;     /* 0 | 1: solve in deComP's unit-norm scaling of the exemplars */
    int check_every;   /* 0: the change is never evaluated; k > 0: at iterations 0, k, 2k, ... (deComP: 10) */
    int stop_rule;     /* EVC_STOP_NONE | EVC_STOP_DECOMP */
    int init_mode;     /* EVC_INIT_GIVEN | EVC_INIT_CONST */
    int reserved;      /* 0 */
    int reserved2;     /* 0 */
    int lip_weights;   /* EVC_PROX_LIP_MEAN | EVC_PROX_LIP_MAX: the per-bin weights of the Gershgorin bound */
    int reserved3;     /* 0 */
    double alpha;      /* >= 0: the penalty (normalize: per valid bin, as deComP's 1 / (2 cnt_t) scaling of the squared error) */
    double tol;        /* >= 0: threshold of stop_rule */
    double init_value; /* EVC_INIT_CONST */
    double lipschitz;  /* > 0: used as L for every utterance, the bound is not computed; 0: the bound */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_prox_masked_opts;
/* bytes of workspace evc_prox_masked_solve needs (0: invalid or unsupported arguments, M > 1056 and N > 16384 among them) */
size_t evc_prox_masked_workspace_bytes(int M, int N, int T, int n_utt, int dtype);
int evc_prox_masked_solve(const void* A, int lda, const void* X, int ldx, const void* mask, int ldm, void* H, int ldh, int M,
                          int N, int T, const int* utt_offsets, int n_utt, const evc_prox_masked_opts* opts, void* workspace,
                          size_t workspace_bytes, int* n_iter_out, double* change_out, evc_stream_t stream);

/* Sparse dictionary learning, X ~ D H with sparse H and atoms of norm <= 1: Mairal et al.'s online dictionary learning as
 * deComP's dictionary_learning.solve(method='block_cd') runs it (dictionary_learning.py:114-168; utils/data.py:101-121;
 * utils/normalize.py).  X is M x T, D is the M x N dictionary (atoms as columns; deComP's D is its transpose), H is N x T
 * (deComP's x is its transpose); layouts and leading dimensions as in evc_prox_solve, D addressed like its A.  D and H hold
 * the start on entry and are updated in place.  `stats` is the N x (N + M) matrix [S | Q] of the two sufficient statistics,
 * row-major with the leading dimension ld_stats >= N + M, in the call's dtype, and *count_io the number of steps so far:
 * both caller-owned, as acc_a / acc_b of evc_online_learn.  resume = 0: the call first divides every atom of D by its
 * Euclidean norm (a zero atom becomes NaN, as numpy's 0 / 0), zeroes `stats` and *count_io; resume = 1: nothing is touched.
 * Epoch e = 0 .. epochs - 1 has floor(T / bs) batches, bs = batch_size; batch b takes the frames
 * order[e][b bs .. (b + 1) bs) (order == NULL: the identity), and the last T mod bs frames of the row are not touched in that
 * epoch.  One step on the batch's frames F:
 *   lasso       evc_prox_solve's statement on X[:, F] and H[:, F] as ONE utterance with the current D: normalize = 1, alpha,
 *               tol = lasso_tol, iters = lasso_iters, check_every = lasso_check_every, EVC_STOP_DECOMP, EVC_INIT_GIVEN, mode,
 *               momentum, the Gershgorin step.  The batch's columns are gathered into the workspace and the result is
 *               scattered back; the frames are never moved.
 *   statistics  theta = count bs + 1, beta = (theta - bs) / theta in double precision on the host;
 *               S <- beta S + H_F H_F^T;  Q <- beta Q + H_F X_F^T
 *   sweep       for k = 0 .. N - 1 in order, D_cur holding the new atoms j < k and the old atoms j >= k:
 *               u = (Q[k, :] - sum_j S[k, j] d_j) / (S[k, k] + 1e-15) + d_k;   d_k <- u / sqrt(max(|u|^2, 1))
 *   stop        stat = max |D_new - D|, recorded in trace_out; count += 1; stat < tol ends the call (a NaN compares false and
 *               runs on).  The stopping step's D and H are kept.
 * Kernels: k_plearn_stats forms beta [S | Q] + H_F [H_F; X_F]^T in one launch on the matrix cores, frames ascending in
 * LDS-staged slabs, the decay in the epilogue.  The sweep is blocked and right-looking with nb = 32, 16, 8 or 4 atoms per
 * block (from M and the dtype alone): Rm = Q - S D^T once per step, then one launch of k_plearn_block per block, in which
 * every workgroup redoes the block's nb sequential atom updates (the same instructions in the same order) and then takes
 * the block's changes off its own rows of Rm behind the block; workgroup 0 alone stores the new atoms.  ceil(N / nb)
 * dependent launches instead of N, no exchange between workgroups inside a launch, no residency assumption, no float
 * atomics: the same call gives the same bits, and with tol = 0 a call of p epochs followed by a resume = 1 call of q epochs
 * on the remaining rows of `order` gives bitwise the D, H, stats and count of one call of p + q epochs.
 *   M : 1 .. 1056, N : 1 .. 4096 (larger: -3);  T >= 1;  1 <= batch_size <= T;  epochs >= 0 (0: the start after the
 *       resume = 0 preparation)
 *   order : NULL or host int[epochs][T], every row a permutation of 0 .. T - 1 (anything else: -1)
 *   n_epochs_out, n_steps_out : host ints or NULL: e + 1 of the stopping step (else `epochs`), and the steps carried out
 *   trace_out : host, epochs * floor(T / bs) doubles or NULL: stat of every step, NaN after the stop
 * Ask evc_prox_learn_workspace_bytes for the workspace (the gathered batch, Rm, a copy of D, the lasso's workspace).
 * Status -1 / -3 / -2 are returned before any device work.  Host synchronisation: one read of one double per step when
 * tol > 0 or trace_out is given, as evc_online_learn for its convergence; else the call is a pure enqueue. */
typedef struct evc_prox_learn_opts {
    int struct_bytes;        /* sizeof(evc_prox_learn_opts) */
    int dtype;               /* EVC_F64 | EVC_F32 */
    int layout;              /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int batch_size;          /* 1 .. T */
    int epochs;              /* passes over the frames, >= 0 (deComP: maxiter - 1) */
    int lasso_iters;         /* updates of a step's lasso, >= 0 (deComP: 10) */
    int lasso_check_every;   /* as evc_prox_opts.check_every (deComP: 10) */
    int mode;                /* EVC_PROX_POSITIVE | EVC_PROX_SIGNED */
    int momentum;            /* EVC_PROX_ISTA | EVC_PROX_FISTA | EVC_PROX_NESTEROV */
    int resume;              /* 0: D is normalised, stats and count are zeroed by the call; 1: they hold a previous call's state */
    int reserved;            /* 0; measurement only: bit 0 the steps run without their lasso, bit 1 without their statistics,
                                bit 2 without their sweep (and then without a stop statistic); anything else: status -1 */
    int reserved2;           /* 0 */
    double alpha;            /* >= 0: the lasso's penalty, per bin */
    double tol;              /* >= 0: the call stops when max |D_new - D| < tol; 0: never */
    double lasso_tol;        /* >= 0: the lasso's stop threshold (deComP: 1e-5) */
    void* ev_loop_start;     /* optional hipEvent_t pair recorded around the launches of the step loop, as in */
    void* ev_loop_stop;      /* evc_solve_opts; NULL = not recorded */
} evc_prox_learn_opts;
/* bytes of workspace evc_prox_learn needs (0: invalid or unsupported arguments, M > 1056, N > 4096 and batch_size > T among them) */
size_t evc_prox_learn_workspace_bytes(int M, int N, int T, int batch_size, int dtype);
/* atoms per block of the sweep for M bins: 32, 16, 8 or 4 (0: invalid arguments) */
int evc_prox_learn_block(int M, int dtype);
int evc_prox_learn(const void* X, int ldx, void* D, int ldd, void* H, int ldh, void* stats, int ld_stats, long long* count_io,
                   const int* order, int M, int N, int T, const evc_prox_learn_opts* opts, void* workspace,
                   size_t workspace_bytes, int* n_epochs_out, int* n_steps_out, double* trace_out, evc_stream_t stream);

/* evc_prox_learn with a weight per bin of every frame (missing data): deComP's dictionary_learning.solve(..., mask=), its
 * solve_cd_mask (dictionary_learning.py:171-231).  X, D, H, layouts, leading dimensions, batches, `order`, *count_io, resume,
 * the outputs and the host synchronisation are evc_prox_learn's.  `mask` has X's dtype, layout and shape (M x T) with its own
 * leading dimension ldm, weights >= 0 (a zero: the bin is missing; negative weights are not looked for); NULL is status -1 -
 * a caller without a mask wants evc_prox_learn, which is another algorithm.  With a mask the Gram statistic is one N x N
 * matrix PER BIN: `stats_s` holds M planes of N rows, plane m at stats_s + m N ld_s, row-major with ld_s >= N; `stats_q` is
 * N x M, row-major with ld_q >= M; both caller-owned, in the call's dtype, zeroed by a resume = 0 call.
 * One step on the batch's frames F:
 *   lasso       evc_prox_masked_solve's statement on X[:, F], mask[:, F] and H[:, F] as ONE utterance with the current D:
 *               normalize = 1, EVC_PROX_LIP_MEAN (deComP's step), EVC_STOP_DECOMP, EVC_INIT_GIVEN; alpha, tol = lasso_tol,
 *               iters = lasso_iters, check_every = lasso_check_every, mode and momentum from the options
 *   statistics  theta = count bs + 1, beta = (theta - bs) / theta in double precision on the host;
 *               S_m[k][j] <- beta S_m[k][j] + sum_{t in F} (H[k][t] mask[m][t]) H[j][t]  for every bin m
 *               Q <- beta Q + H_F (mask_F . X_F)^T
 *   atoms       every atom from the OLD dictionary (a Jacobi step, as dictionary_learning.py:218 contracts with D, not D_new):
 *               G[k][m] = sum_j S_m[k][j] d_j[m];  a_k = sum_m (S_m[k][k] + 1e-15), m ascending - ONE scalar per atom, deComP's
 *               (line 219), mirrored and not corrected;  u = (Q[k, :] - G[k, :]) / a_k + d_k;  d_k <- u / sqrt(max(|u|^2, 1))
 *   stop        stat = max |D_new - D|, recorded in trace_out; count += 1; stat < tol ends the call (a NaN runs on)
 * A frame whose mask is all zero runs with threshold 0; a bin missing in a whole batch is fine; a batch whose mask is all
 * zero has L = 0 and gets what evc_prox_masked_solve documents for that (NaN), and the dictionary becomes NaN.
 * Kernels: k_pmlearn_stats - a workgroup owns one bin and one panel of 64 rows of its plane and walks the panel's column tiles
 * in ascending j: per tile the frames ascending in LDS-staged slabs of 16 (float32: 32), the left operand multiplied by the bin's weights
 * as it is staged, 16x16x4 MFMAs, one chain per output; the epilogue applies the decay, stores the tile, multiplies it by
 * d_j[m] into per-row running sums (one fixed lane reduce at the end gives G[k][m]) and stores the diagonal entries.  The
 * tensor is read once and written once per step.  k_pmlearn_q forms Q, k_pmlearn_atoms updates all atoms in one launch, one
 * workgroup per atom.  No exchange between workgroups, no residency assumption, no float atomics: the same call gives the
 * same bits, and with tol = 0 a call of p epochs followed by a resume = 1 call of q epochs on the remaining rows of `order`
 * gives bitwise the D, H, stats_s, stats_q and count of one call of p + q epochs.
 *   M : 1 .. 1056, N : 1 .. 1024, M N^2 <= 2^28 elements (larger: -3);  T, batch_size, epochs, order, n_epochs_out,
 *       n_steps_out, trace_out : as for evc_prox_learn
 * Ask evc_prox_masked_learn_workspace_bytes for the workspace (the gathered batch [H_F | X_F | mask_F], G, the diagonals, a
 * copy of D, the shares, the epoch's order row, the lasso's workspace).  Status -1 / -3 / -2 are returned before any device
 * work. */
typedef struct evc_prox_masked_learn_opts {
    int struct_bytes;        /* sizeof(evc_prox_masked_learn_opts) */
    int dtype;               /* EVC_F64 | EVC_F32 */
    int layout;              /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int batch_size;          /* 1 .. T */
    int epochs;              /* passes over the frames, >= 0 (deComP: maxiter - 1) */
    int lasso_iters;         /* updates of a step's lasso, >= 0 (deComP: 10) */
    int lasso_check_every;   /* as evc_prox_opts.check_every (deComP: 10) */
    int mode;                /* EVC_PROX_POSITIVE | EVC_PROX_SIGNED */
    int momentum;            /* EVC_PROX_ISTA | EVC_PROX_FISTA | EVC_PROX_NESTEROV */
    int resume;              /* 0: D is normalised, the statistics and count are zeroed by the call; 1: they hold a previous call's state */
    int reserved;            /* 0; measurement only, as evc_prox_learn_opts.reserved: bit 0 the steps run without their lasso,
                                bit 1 without their statistics, bit 2 without their atom update (and then without a stop
                                statistic); anything else: status -1 */
    int reserved2;           /* 0 */
    double alpha;            /* >= 0: the lasso's penalty, per valid bin */
    double tol;              /* >= 0: the call stops when max |D_new - D| < tol; 0: never */
    double lasso_tol;        /* >= 0: the lasso's stop threshold (deComP: 1e-5) */
    void* ev_loop_start;     /* optional hipEvent_t pair recorded around the launches of the step loop, as in */
    void* ev_loop_stop;      /* evc_solve_opts; NULL = not recorded */
} evc_prox_masked_learn_opts;
/* bytes of workspace evc_prox_masked_learn needs (0: invalid or unsupported arguments, M > 1056, N > 1024, M N^2 > 2^28 and
 * batch_size > T among them) */
size_t evc_prox_masked_learn_workspace_bytes(int M, int N, int T, int batch_size, int dtype);
int evc_prox_masked_learn(const void* X, int ldx, const void* mask, int ldm, void* D, int ldd, void* H, int ldh, void* stats_s,
                          int ld_s, void* stats_q, int ld_q, long long* count_io, const int* order, int M, int N, int T,
                          const evc_prox_masked_learn_opts* opts, void* workspace, size_t workspace_bytes, int* n_epochs_out,
                          int* n_steps_out, double* trace_out, evc_stream_t stream);

/* Multiplicative updates of the activations with a weight per bin of every frame (missing data), the dictionary fixed:
 * deComP's Likelihood.update_x (decomp/nmf_methods/grads.py), the activation half of nmf.solve(method='mu', likelihood='l2' |
 * 'kl', mask=...), mirrored and not corrected.  `mask` has X's dtype, layout and shape (M x T) with its own leading dimension
 * ldm; NULL means every weight is 1 and no mask is read (deComP's unmasked update).  With J = 1e-15 (deComP's _JITTER, in
 * both element types), per iteration and frame:
 *     EVC_LOSS_FROBENIUS (l2):  V = A h;      Num = A^T (mask . x);          Den = A^T (mask . V)
 *     EVC_LOSS_KL (kl):         V = A h + J;  Num = A^T ((mask . x) / V);    Den = A^T mask
 *     h <- (h * max(Num, 0)) / max(Den, J)        (the product first, then the quotient; a NaN passes both maxima, as numpy's)
 * A frame whose mask is all zero gets h = 0 after one update.  Negative weights are not looked for.
 * deComP has no fixed-dictionary surface, so the error and the stop rule are this library's own: the error of utterance u,
 * at the start and after every `check_every` iterations, is the masked form of sklearn's _beta_divergence(square_root=True),
 *     l2:  sqrt(sum mask (X - V)^2)           kl:  sqrt(2 max(sum mask (X log(X / V) - X + V), 0)),  terms with X = 0: mask V
 * over the utterance's frames, with V = A h (kl: + J), and EVC_STOP_SKLEARN stops an utterance at a check when
 * (err_prev - err) / err_at_start < tol; its frames are frozen while the others go on.  A NaN error never stops.
 * One kernel launch per iteration (k_mum_sweep) on k_beta_sweep's geometry: a workgroup owns 16 frames of one utterance,
 * forms V = A H on the matrix cores, turns it into Q1 | Q2 in LDS (l2: mask . X | mask . V; kl: (mask . X) / V | mask) and forms
 * Num | Den per exemplar tile; mask . X and mask are packed once per call.  The error is summed in float64 for both types, per utterance in a fixed order (no float atomics): the same
 * call gives bitwise the same output every time, a batch of utterances gives bitwise the activations of one call per
 * utterance, a NULL mask the bits of a mask of ones, and a NaN in a frame of X stays in that frame's column.
 *   M      : 1 .. 528 bins (larger: -3);  any N >= 1, T >= 0 (an utterance may be empty);  iters = 0 leaves the start in H
 *   layout, utt_offsets, n_utt, n_iter_out, err_out : as for evc_beta_solve (at most 4097 error slots per utterance: -1)
 * Status -1 / -3 / -2 are returned before any device work.  Host synchronisation: as evc_beta_solve, case (8). */
typedef struct evc_mu_masked_opts {
    int struct_bytes;  /* sizeof(evc_mu_masked_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int loss;          /* EVC_LOSS_FROBENIUS (deComP: 'l2') | EVC_LOSS_KL ('kl') */
    int iters;         /* number of multiplicative updates (>= 0) */
    int init_mode;     /* EVC_INIT_GIVEN | EVC_INIT_CONST */
    int check_every;   /* 0: the error is never evaluated; k > 0: at the start and every k iterations */
    int stop_rule;     /* EVC_STOP_NONE | EVC_STOP_SKLEARN */
    int reserved;      /* 0 */
    int reserved2;     /* 0 */
    double tol;        /* >= 0: threshold of stop_rule */
    double init_value; /* EVC_INIT_CONST */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_mu_masked_opts;
/* bytes of workspace evc_mu_masked_solve needs (0: invalid or unsupported arguments, M > 528 among them) */
size_t evc_mu_masked_workspace_bytes(int M, int N, int T, int n_utt, int dtype);
int evc_mu_masked_solve(const void* A, int lda, const void* X, int ldx, const void* mask, int ldm, void* H, int ldh, int M,
                        int N, int T, const int* utt_offsets, int n_utt, const evc_mu_masked_opts* opts, void* workspace,
                        size_t workspace_bytes, int* n_iter_out, double* err_out, evc_stream_t stream);

/* Multiplicative updates of BOTH factors with a weight per entry (missing data), X ~ W H with unit-norm atoms: deComP's
 * nmf.solve(y, D, x, tol, maxiter=iters + 1, method='mu', likelihood='l2' | 'kl', mask=mask) (decomp/nmf.py,
 * nmf_methods/batch_mu.py, nmf_methods/grads.py, utils/normalize.py), mirrored and not corrected.  X is M x T, W is M x R (atoms
 * as columns; deComP's D is its transpose), H is R x T (deComP's x is its transpose), mask as in evc_mu_masked_solve (NULL:
 * deComP's unmasked nmf.solve); layouts and leading dimensions as in evc_nmf_learn.  W and H hold the start on entry and are
 * updated in place.  On entry every atom of W is divided by its Euclidean norm (nmf.solve does).  Then per iteration:
 *   activations  one update of evc_mu_masked_solve on the current W (the same kernel; its packed dictionary images are
 *                rebuilt from W every iteration): with iters = 1 the activations are bitwise those of
 *                evc_mu_masked_solve(iters = 1, EVC_INIT_GIVEN) on the normalised start
 *   dictionary   with the new H and J = 1e-15:   l2: Num = (mask . X) H^T,              Den = (mask . (W H)) H^T
 *                                                kl: Num = ((mask . X) / (W H + J)) H^T,  Den = mask H^T
 *                W <- (W * max(Num, 0)) / max(Den, J); then every atom is divided by its Euclidean norm (a zero atom becomes
 *                NaN, as in numpy)
 *   statistic    max |W_before - W_after| over all entries (both normalised)
 * With check_every > 0 and (tol > 0 or stat_out) the host reads the statistic after every check_every-th iteration and, with
 * tol > 0, stops when it is < tol (deComP: check_every = 1; a NaN statistic never stops); *n_iter_out is the number of
 * iterations run.  deComP's loop is `for it in range(1, maxiter)`: it runs at most maxiter - 1 iterations and returns `it` when it
 * stops, else maxiter.
 * The dictionary half runs on evc_beta_learn's unfused route: V^T = H^T W^T by the generic contraction, k_mum_dict_q forms the
 * two left operands, the split contraction of evc_nmf_learn sums them against H over S = evc_mu_masked_learn_splits(M, R, T)
 * contiguous frame ranges, and k_mum_dict_apply - one workgroup per atom - adds the S slabs in the order 0 .. S-1, updates,
 * normalises and compares.  Every reduction runs in an order fixed by the sizes and S: no float atomics, the same call gives
 * the same bits every time.
 *   M : 1 .. 528, R : 1 .. 4096 (larger: -3);  T >= 1
 *   stat_out : host, 1 + iters / check_every doubles or NULL: NaN in slot 0 (there is no statistic at the start), then the
 *              statistic at every check that was evaluated (NaN where not); at most 4097 slots (more: -1)
 * Status -1 / -3 / -2 are returned before any device work.  Host synchronisation: as evc_beta_learn, case (9). */
typedef struct evc_mu_masked_learn_opts {
    int struct_bytes;  /* sizeof(evc_mu_masked_learn_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int loss;          /* EVC_LOSS_FROBENIUS (deComP: 'l2') | EVC_LOSS_KL ('kl') */
    int iters;         /* maximum number of iterations (>= 0; deComP: maxiter - 1) */
    int check_every;   /* 0: the statistic is never read; k > 0: after every k-th iteration (deComP: 1) */
    int reserved;      /* 0; tests and tuning: bits 8..15 force the number of frame ranges S (1 .. 64) */
    int reserved2;     /* 0 */
    double tol;        /* >= 0: the call stops when the statistic is < tol; 0: never */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the iteration loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_mu_masked_learn_opts;
/* bytes of workspace evc_mu_masked_learn needs (0: invalid or unsupported arguments, M > 528 and R > 4096 among them) */
size_t evc_mu_masked_learn_workspace_bytes(int M, int R, int T, int dtype);
/* the frame ranges S the dictionary half sums over when none is forced (0: invalid or unsupported sizes) */
int evc_mu_masked_learn_splits(int M, int R, int T);
int evc_mu_masked_learn(const void* X, int ldx, const void* mask, int ldm, void* W, int ldw, void* H, int ldh, int M, int R,
                        int T, const evc_mu_masked_learn_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out,
                        double* stat_out, evc_stream_t stream);

/* deComP's mini-batch NMF, X ~ W H with unit-norm atoms: nmf.solve(y, D, x, tol, minibatch=batch_size, maxiter=epochs + 1,
 * method='asg-mu' | 'gsg-mu' | 'asag-mu' | 'gsag-mu' | 'svrmu' | 'svrmu-acc', likelihood='l2' | 'kl', mask=mask)
 * (decomp/nmf.py, nmf_methods/serizel.py, nmf_methods/kasai.py, nmf_methods/grads.py, utils/data.py, utils/normalize.py),
 * mirrored and not corrected.  X, mask, W, H, layouts and leading dimensions as in evc_mu_masked_learn; W and H hold the start
 * on entry and are updated in place.  On entry every atom of W is divided by its Euclidean norm.  An epoch has n_loop =
 * floor(T / batch_size) steps; step b takes the frames F = order[e][b bs .. (b + 1) bs), the last T mod bs frames of the row
 * are not touched in that epoch.  Per step, with J = 1e-15:
 *   activations  inner_iters updates of evc_mu_masked_solve (the same kernel) on X[:, F], mask[:, F], H[:, F] with the current W
 *   gradients    from the new H_F:  l2: g+ = (mask . X_F) H_F^T,              g- = (mask . (W H_F)) H_F^T
 *                                   kl: g+ = ((mask . X_F) / (W H_F + J)) H_F^T,  g- = mask H_F^T
 *   dictionary   EVC_STOCH_ASG   ('asg-mu'; deComP sends 'gsg-mu' here too):  W_new = (W max(g+, 0)) / max(g-, J), every step
 *                EVC_STOCH_ASAG  a+- <- (1 - rho) a+- + rho g+- (zero at every epoch's start), W_new from a+-, every step
 *                EVC_STOCH_GSAG  the same accumulation every step, W_new from a+- once, after the epoch's last step
 *                EVC_STOCH_SVRMU at every epoch's start, without an activation update, full+- = (sum_b g+-_b) / n_loop in
 *                                step order;  per step P = g+ + prev-[b] + full+,  Q = g- + prev+[b] + full- (the crossed
 *                                signs are deComP's),  W_new = max(W ((1 - alpha) + alpha P / max(Q, J)), 0),  then
 *                                prev+-[b] <- g+-;  prev starts at zero and lives for the whole call
 *                every operation in the order written, none contracted; then every atom of W_new is divided by its
 *                Euclidean norm (a zero atom becomes NaN, as in numpy)
 *   stop         stat = max |W - W_new|;  stat < tol ends the call and W KEEPS THE OLD VALUE (deComP returns D, not D_new), H
 *                keeps this step's update, the frames of later steps are untouched;  a NaN statistic never stops;  otherwise
 *                W <- W_new
 * The dictionary half has two routes (opts.route: 0 the library's choice, fused up to R = 256; 1 fused, R <= 256 or -3; 2 unfused):
 * fused, k_mus_dict_grad recomputes W H_F on the matrix cores, applies mask and loss in registers and contracts against H_F in
 * one launch; unfused, evc_mu_masked_learn's kernels.  Both leave S slabs of partial sums over contiguous frame ranges of the
 * batch (S a function of M, R, batch_size and the route only), added in the order 0 .. S-1.  The stop is decided on the device:
 * the launches enqueued after it return at once, and the host reads the stop word once per epoch (only when tol > 0).  No
 * float atomics, no exchange between workgroups: the same call gives the same bits every time.
 *   M : 1 .. 528, R : 1 .. 4096 (larger: -3);  1 <= batch_size <= T;  svrmu keeps 2 n_loop M R elements (over 2^40 bytes: -3)
 *   order        : host int[order_rows][T], every row a permutation of 0 .. T-1 (else -1); NULL with order_rows = 0: the
 *                  frames as they lie; order_rows = 1: every epoch takes the same row (svrmu); else order_rows = epochs
 *   n_epochs_out : host int or NULL: the epoch (from 1) of the update that stopped the call, else `epochs`
 *   n_steps_out  : host int or NULL: the steps carried out (the stopping one included)
 *   trace_out    : host, one double per dictionary update (epochs * n_loop; gsag: epochs) or NULL: its statistic, NaN after
 *                  the stop
 * Status -1 / -3 / -2 are returned before any device work.  With tol = 0 and all three outputs NULL the call only enqueues. */
enum { EVC_STOCH_ASG = 0, EVC_STOCH_ASAG = 1, EVC_STOCH_GSAG = 2, EVC_STOCH_SVRMU = 3 };
typedef struct evc_mu_stoch_opts {
    int struct_bytes;  /* sizeof(evc_mu_stoch_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int loss;          /* EVC_LOSS_FROBENIUS (deComP: 'l2') | EVC_LOSS_KL ('kl') */
    int method;        /* EVC_STOCH_* */
    int batch_size;    /* frames per step (deComP: minibatch) */
    int epochs;        /* >= 0 (deComP: maxiter - 1) */
    int inner_iters;   /* >= 1 activation updates per step; must be 1 unless EVC_STOCH_SVRMU (deComP's svrmu-acc) */
    int order_rows;    /* 0 (order == NULL) | 1 | epochs */
    int route;         /* 0: the library's choice; 1: fused; 2: unfused */
    int reserved;      /* 0 */
    int reserved2;     /* 0 */
    double forget_rate;   /* rho of asag / gsag, 0 < rho <= 1 (deComP: 0.5) */
    double alpha;         /* svrmu's step (deComP: 1.0) */
    double tol;           /* >= 0: the call stops when the statistic is < tol; 0: never */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the epoch loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_mu_stoch_opts;
/* bytes of workspace evc_mu_stoch_learn needs (0: invalid or unsupported arguments) */
size_t evc_mu_stoch_learn_workspace_bytes(int M, int R, int T, int batch_size, int method, int dtype);
/* the route (1 fused, 2 unfused) and the frame ranges S the dictionary half takes for `route` (0: invalid or unsupported) */
int evc_mu_stoch_learn_route(int R, int route);
int evc_mu_stoch_learn_splits(int M, int R, int batch_size, int route);
int evc_mu_stoch_learn(const void* X, int ldx, const void* mask, int ldm, void* W, int ldw, void* H, int ldh, const int* order,
                       int M, int R, int T, const evc_mu_stoch_opts* opts, void* workspace, size_t workspace_bytes,
                       int* n_epochs_out, int* n_steps_out, double* trace_out, evc_stream_t stream);

/* k-means (pymf kmeans.py:57-83 with base.py:238-270 and dist.py:54-60, 104-127): X (M x T, signed allowed) is clustered
 * around R centres W (M x R).  One assignment with the start centres comes first; each of `iters` rounds then moves every
 * centre to the mean of its members (unless EVC_KM_ASSIGN_ONLY; an empty cluster keeps its centre), assigns again and
 * evaluates err = ||X - W[:, labels]||_F.
 *   Assignment: labels[t] is the smallest r that minimises the Euclidean distance between column t of X and column r of W,
 *   as the direct form sum_m (x_m - w_m)^2 in the working type decides it.  k_km_assign forms the expanded scores
 *   ||w_r||^2 - 2 w_r^T x_t on the matrix cores (v_mfma_*_16x16x4), a workgroup owning 64 samples and walking the centres in
 *   tiles of 32, and keeps the best and the second-best score of every sample in registers: the R x T scores never reach
 *   memory.  Every sample whose two scores lie closer than g_t = 4 (M + 4) u (||x_t||^2 + max_r ||w_r||^2), u the unit
 *   round-off of the working type, is decided again by the direct form over all R centres (k_km_refine).  The comparison is
 *   lexicographic on (score, index): identical centres give identical scores and the lower index wins, whatever the order
 *   of tiles and centre ranges.  Where T alone gives fewer workgroups than the chip has compute units the centres are
 *   split into evc_kmeans_splits(R, T) ranges, merged in ascending order by a second kernel.
 *   Centres: members are summed in ascending sample order, in the working type; no float atomics, the same call gives the
 *   same bits every time.  Error: sum_t ||x_t - w_labels[t]||^2 in the direct form, float64, a fixed order - unchanged
 *   labels and centres give bit-identical consecutive errors, which is what pymf's machine-epsilon stop relies on.
 *   Stop, decided on the device: EVC_KM_STOP_PYMF from the third round on when |err_i - err_{i-1}| / T < tol (pymf:
 *   2.22e-16); EVC_KM_STOP_LABELS when a round changed no label.  The stopping round's centres and labels are kept.
 *   X, W    : addressed as in evc_convex_learn's X and W, under both layouts; W holds the start centres on entry and the
 *             final ones on return; nothing outside the logical elements of any buffer is written
 *   labels  : T device int32 or NULL;  counts : R device int32 or NULL (members per centre under the returned labels)
 *   M : 1 .. 1056, T : 1 .. 2^20, R : 1 .. min(T, 4096) (larger: -3; the workspace query then answers 0).  The assignment
 *   alone (EVC_KM_ASSIGN_ONLY) also takes a codebook of more centres than samples, R : 1 .. 4096 (pymf's doctest assigns one
 *   sample to two centres); the two queries answer for it
 *   n_iter_out : host int or NULL: rounds carried out
 *   err_out    : host, 1 + iters doubles or NULL (at most 4097 slots; more: -1): the error after the first assignment, then
 *                after every round (NaN where not evaluated)
 * float32 inputs are clustered in float32; the error is summed in float64.  Status -1 / -3 / -2 are returned before any
 * device work.  Host synchronisation: as evc_convex_learn. */
enum { EVC_KM_BOTH = 0, EVC_KM_ASSIGN_ONLY = 1 };
enum { EVC_KM_STOP_NONE = 0, EVC_KM_STOP_PYMF = 1, EVC_KM_STOP_LABELS = 2 };
typedef struct evc_kmeans_opts {
    int struct_bytes;  /* sizeof(evc_kmeans_opts) */
    int dtype;         /* EVC_F64 | EVC_F32 */
    int layout;        /* EVC_FRAME_MAJOR | EVC_BIN_MAJOR */
    int iters;         /* >= 0 rounds after the first assignment */
    int update;        /* EVC_KM_BOTH | EVC_KM_ASSIGN_ONLY */
    int stop_rule;     /* EVC_KM_STOP_* */
    int reserved;      /* 0; bits 8..15, tuning and tests: that many centre ranges (1 .. 16) instead of evc_kmeans_splits();
                          bit 0, likewise: every sample goes through the direct-form re-decision; anything else: status -1 */
    double tol;        /* >= 0 (EVC_KM_STOP_PYMF) */
    void* ev_loop_start;  /* optional hipEvent_t pair recorded around the launches of the round loop, as in */
    void* ev_loop_stop;   /* evc_solve_opts; NULL = not recorded */
} evc_kmeans_opts;
/* bytes of workspace evc_kmeans needs (0: invalid or unsupported sizes, wherever the call would return -1 or -3) */
size_t evc_kmeans_workspace_bytes(int M, int R, int T, int dtype);
/* centre ranges the assignment is split into, 1 .. 16: a function of the sizes only (0: invalid or unsupported sizes) */
int evc_kmeans_splits(int R, int T);
int evc_kmeans(const void* X, int ldx, void* W, int ldw, int* labels, int* counts, int M, int R, int T,
               const evc_kmeans_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out, double* err_out,
               evc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* EVC_H */
