// The main activation solve of libevc_hip.so (include/evc.h): evc_nmf_solve / evc_nmf_convert with their size and
// prepared-dictionary entries, evc_synthesize, evc_residual, and the version / status / device entries.  What a solve
// decides and carves is in evc_solve_plan.h (plan_route, plan_fused_tail, the carvers); here are the argument checks
// (solve_checked, which also holds the one redo path), the call record (SolveCall) and the drivers it is handed to: the
// task queues (solve_wide), the float64 fused kernels (solve_fused; float32 callers through solve_f32_on_f64) and the two
// contractions (solve_gemm).  No allocation, no global state, no exceptions.
// (Every other entry sits with its kernels: evc_learn.hip, evc_cd.hip, evc_beta.hip, evc_beta_learn.hip, evc_gl.hip,
// evc_mfcc.hip, evc_dtw.hip.)
#include "evc_solve_plan.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

using namespace evc;

namespace {

constexpr int DICT_MAGIC = 0x45564344;      // "EVCD"

// One evc_nmf_solve / evc_nmf_convert call as the drivers see it: operands, sizes, utterance offsets, workspace, outputs,
// the synthesis that follows (NULL: none) and the stream.  Built once by the entry and passed by reference;
// solve_f32_on_f64 builds the staged one.  Every driver is driver(call, opts, route, info).
struct SolveCall {
    const void* A; int lda;
    const void* X; int ldx;
    void* H; int ldh;
    int M, N, T_;
    const int* utt_offsets; int n_utt;
    void* ws; size_t ws_bytes;
    int* n_iter_out; double* err_out;
    const SynthArgs* y;
    hipStream_t s;
};

// hand back the per-utterance results
int copy_back(const UttState& u, int n_utt, int n_slots, int* n_iter_out, double* err_out, hipStream_t s) {
    if (n_iter_out || err_out) {
        if (n_iter_out)
            HIP_TRY(hipMemcpyAsync(n_iter_out, u.n_iter, sizeof(int) * n_utt, hipMemcpyDeviceToHost, s));
        if (err_out)
            HIP_TRY(hipMemcpyAsync(err_out, u.trace, sizeof(double) * (size_t)n_utt * n_slots,
                                   hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return ST_OK;
}

// Y = B H on frames-as-rows activations Hc (row stride ldc) and the caller's B / Y
template <typename T>
int synth_rows(const T* Hc, long ldc, const SynthArgs& y, int N, int T_, bool fm, hipStream_t s) {
    const T* B = static_cast<const T*>(y.B);
    T* Y = static_cast<T*>(y.Y);
    // B(n, mb) = B[n bsn + mb bsm]
    const long bsn = (fm || y.b_rows) ? y.ldb : 1, bsm = (fm || y.b_rows) ? 1 : y.ldb;
    if (fm)   // Y[t][mb] = sum_n Hc[t][n] B[n][mb]
        HIP_TRY(gemm_strided<T>(Hc, ldc, 1, B, bsm, bsn, Y, y.ldy, 1, T_, y.Mb, N, s));
    else      // Y[mb][t] = sum_n B[mb][n] Hc[t][n]
        HIP_TRY(gemm_strided<T>(B, bsm, bsn, Hc, ldc, 1, Y, y.ldy, 1, y.Mb, T_, N, s));
    return ST_OK;
}

// Bring the caller's dictionary into the generic arrays of `a`
template <typename T>
int prepare_dict(const DictArrays<T>& a, bool kl, const T* A, int lda, const Dims& d, bool fm, double eps, hipStream_t s) {
    HIP_TRY(copy2d<T>(A, lda, d.N, d.M, fm ? 0 : 1, a.At, d.Mk, d.Np, d.Mk, 0, s));
    HIP_TRY(copy2d<T>(A, lda, d.M, d.N, fm ? 1 : 0, a.Am, d.Np, d.Mj, d.Np, 0, s));
    if (kl) HIP_TRY(kl_scale_dict<T>(a.At, d.Mk, d.M, d.Np, eps, a.Akl, s));
    return ST_OK;
}
// ... and into the operand fragments of the float64 fused kernels the plan names.  B may be NULL.
int prepare_dict_fused(const DictArrays<double>& a, const DictPlan& p, const double* B, int ldb, const Dims& d, bool fm,
                       bool want_rowsum, hipStream_t s) {
    if (p.fused) {
        const FusedLayout fl = fused_layout(d.M, d.N, 1);
        if (p.kl) {      // D/P operand order from the scaled dictionary, V' operand order from A
            HIP_TRY(fused_pack_dict(fl, a.A1p, nullptr, a.Akl, d.Mk, d.Np, s));
            HIP_TRY(fused_pack_dict(fl, nullptr, a.A2p, a.At, d.Mk, d.Np, s));
        } else {
            HIP_TRY(fused_pack_dict(fl, a.A1p, a.A2p, a.At, d.Mk, d.Np, s, (d.M % 4) ? d.M : -1));
        }
        if (want_rowsum) HIP_TRY(fused_rowsum(a.At, d.Mk, d.M, d.N, a.rsum, s));
    }
    if (p.packed_b && B && a.Bt) {
        // Bt[n][mb] (zero padded to 32 bins) -> B's V'-operand fragments
        const FusedLayout flB = fused_layout(d.Mb, d.N, 1);
        HIP_TRY(copy2d<double>(B, ldb, d.N, d.Mb, fm ? 0 : 1, a.Bt, 32, d.Np, 32, 0, s));
        HIP_TRY(fused_pack_dict(flB, a.B1p, a.B2p, a.Bt, 32, d.Np, s));
    }
    return ST_OK;
}
template <typename T>
int dict_prepare_typed(const T* A, int lda, const T* B, int ldb, int M, int Mb, int N, bool fm, int loss, double eps,
                       void* mem, size_t skip, hipStream_t s) {
    const DictImage<T> im = dict_image<T>(mem, skip, M, Mb, N, loss);
    const DictArrays<T>& a = im.a;
    HIP_TRY(prepare_dict<T>(a, im.plan.kl, A, lda, im.d, fm, eps, s));
    if (B && a.Bc) HIP_TRY(copy2d<T>(B, ldb, N, Mb, fm ? 0 : 1, a.Bc, Mb, N, Mb, 0, s));
    if constexpr (sizeof(T) == 4) {
        if (im.plan.wide)
            HIP_TRY(wide_pack_dict(wide_layout(M, N, 1, 256, 0, 0), im.plan.kl ? a.Akl : a.At, a.At, im.d.Mk, im.d.Np, a.Aw, s));
    } else {
        if (im.plan.wide64)
            HIP_TRY(wide_pack_dict(wide64_layout(M, N, 1, 256, 0, 0), a.At, nullptr, im.d.Mk, im.d.Np, a.Aw64, s));
        HIP_TRY(prepare_dict_fused(a, im.plan, B, ldb, im.d, fm, true, s));
    }
    return ST_OK;
}

// tests only (evc_solve_opts.test_abort_at, 0 in production): k > 0 raises the abort flag in front of the k-th
// launch of the iteration loop (-1: the call starts with it raised), as a timed-out wait would; the call then
// takes the caller's retry path after a partially completed solve
struct AbortHook {
    int* word;           // the abort flag of this solve's exchange (NULL: nothing is exchanged, nothing to raise)
    int fake_at;         // 0: raised from the start, k > 0: in front of launch k, -1: never
    int launch_no;
    AbortHook(int* w, int test_abort_at)
        : word(w), fake_at(test_abort_at < 0 ? 0 : (test_abort_at > 0 ? test_abort_at : -1)), launch_no(0) {}
    // clear: the flag is not known to be 0 yet
    int begin(bool clear, hipStream_t s) {
        if (word && (clear || fake_at == 0)) HIP_TRY(hipMemsetAsync(word, fake_at == 0 ? 1 : 0, sizeof(int), s));
        return ST_OK;
    }
    int before_launch(hipStream_t s) {
        if (word && fake_at > 0 && launch_no == fake_at) HIP_TRY(hipMemsetAsync(word, 1, sizeof(int), s));
        ++launch_no;
        return ST_OK;
    }
};
// one host round trip: did a launch of this call give up waiting for a peer workgroup?
int read_abort(const int* word, hipStream_t s, int* aborted) {
    *aborted = 0;
    HIP_TRY(hipMemcpyAsync(aborted, word, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return ST_OK;
}

// utterance bookkeeping of one attempt, then - once Xt is there - the start values
int utt_begin(const UttState& u, const int* utt_offsets, int n_utt, const Dims& d, int iters, hipStream_t s) {
    if (utt_offsets)
        HIP_TRY(hipMemcpyAsync(u.offsets, utt_offsets, sizeof(int) * (n_utt + 1), hipMemcpyHostToDevice, s));
    else
        HIP_TRY(utt_single(u, d.T_, s));
    HIP_TRY(utt_setup(u, n_utt, d.T_, d.Tp, iters, s));
    return ST_OK;
}
template <typename T>
int utt_start_values(const UttState& u, const T* Xt, int n_utt, const Dims& d, const evc_solve_opts& o, hipStream_t s) {
    if (o.init_mode == EVC_INIT_SKLEARN) HIP_TRY(utt_sklearn_h0<T>(Xt, d.Mk, d.M, d.N, u, n_utt, s));
    else if (o.init_mode == EVC_INIT_CONST) HIP_TRY(utt_const_h0(u, n_utt, o.init_value, s));
    return ST_OK;
}

// B's fragments for the synthesis from the packed tiles (a prepared dictionary may hold them already)
int pack_synth_dict(const Workspace<double>& w, const Dims& d, const evc_solve_opts& o, const SynthArgs& y, hipStream_t s) {
    if (y.b_packed) return ST_OK;
    const bool fm = (o.layout == EVC_FRAME_MAJOR);
    // Bt[n][mb] (zero padded to 32 bins) -> B's V'-operand fragments
    HIP_TRY(copy2d<double>(static_cast<const double*>(y.B), y.ldb, d.N, y.Mb, (fm || y.b_rows) ? 0 : 1, w.Bt, 32,
                           d.Np, 32, 0, s));
    HIP_TRY(fused_pack_dict(w.flB, w.B1p, w.B2p, w.Bt, 32, d.Np, s));
    return ST_OK;
}

// What the fused driver and solve_gemm do alike before their first launch: the workspace (dictionary arrays from the
// prepared image, if any), the utterance bookkeeping, the caller's matrices imported into the zero-padded frames-as-rows
// arrays At[n][m], Am[m][n], Xt[t][m], and the start values' constants.  (y points into the record: it is not copied.)
template <typename T> struct Imported {
    Dims d;
    int n_slots;
    Workspace<T> w;
    SynthArgs ydict;     // synthesis from the prepared copy of B
    const SynthArgs* y;
};
template <typename T>
int import_call(const SolveCall& c, const evc_solve_opts& o, const Route& r, bool fused, evc_solve_info* inf, Imported<T>* im) {
    const Dims& d = im->d = make_dims((int)sizeof(T), c.M, c.N, c.T_, c.n_utt, c.y ? c.y->Mb : 0);
    im->n_slots = n_slots_for(o.iters, o.check_every);
    if (im->n_slots > MAX_SLOTS) return ST_UNSUPPORTED;
    // dictionary arrays: from the prepared image (float32 callers riding the float64 kernels: behind its staging)
    DictArrays<T> ext{};
    if (o.dict) ext = dict_arrays<T>(o.dict, (sizeof(T) == 8 && o.dict->dtype == EVC_F32) ? dict_f64_staging(c.M, o.dict->Mb, c.N) : 0);
    Workspace<T>& w = im->w = carve<T>(c.ws, d, r.algo, MAX_SLOTS, fused, o.dict ? &ext : nullptr);
    if (w.bytes_min > c.ws_bytes) return ST_WORKSPACE;
    if (w.bytes > c.ws_bytes) w.Yslab = nullptr;      // no room for the members' shares of Y: the two-pass synthesis
    inf->prepared = o.dict ? 1 : 0;
    im->y = c.y;
    if (o.dict && c.y && o.dict->Mb > 0) {
        im->ydict = *c.y;
        im->ydict.B = ext.Bc; im->ydict.ldb = o.dict->Mb; im->ydict.b_rows = 1; im->ydict.b_packed = ext.B2p ? 1 : 0;
        im->y = &im->ydict;
    }
    w.u.n_slots = im->n_slots;
    const bool fm = (o.layout == EVC_FRAME_MAJOR);
    HIP_TRY(utt_begin(w.u, c.utt_offsets, c.n_utt, d, o.iters, c.s));
    if (!o.dict) {
        DictArrays<T> da{};
        da.At = w.At; da.Am = w.Am; da.Akl = w.Akl;
        HIP_TRY(prepare_dict<T>(da, o.loss == EVC_LOSS_KL, static_cast<const T*>(c.A), c.lda, d, fm, o.eps, c.s));
    }
    HIP_TRY(copy2d<T>(static_cast<const T*>(c.X), c.ldx, c.T_, c.M, fm ? 0 : 1, w.Xt, d.Mk, d.Tp, d.Mk, 0, c.s));
    return utt_start_values<T>(w.u, w.Xt, c.n_utt, d, o, c.s);
}

// The launches of the fused persistent path (float64, M <= 32): one per `check_every` iterations (or a single launch when
// no residual is requested); V is carried between launches.  y: the synthesis that follows (NULL: none); t: what the
// last launch does beyond the updates (plan_fused_tail).
int fused_launches(const SolveCall& c, const Workspace<double>& w, const Dims& d, const evc_solve_opts& o,
                   const FusedRoute& r, const FusedTail& t, const SynthArgs* y, evc_solve_info* inf) {
    hipStream_t s = c.s;
    const int n_utt = c.n_utt;
    if (y && w.packed_synth) HIP_TRY(pack_synth_dict(w, d, o, *y, s));
    if (!o.dict) {     // (a prepared dictionary holds the fragments already)
        DictArrays<double> da{};
        da.At = w.At; da.Akl = w.Akl; da.A1p = w.fb.A1p; da.A2p = w.fb.A2p; da.rsum = w.fb.rsum;
        DictPlan pl{};
        pl.fused = true; pl.kl = o.loss == EVC_LOSS_KL;
        HIP_TRY(prepare_dict_fused(da, pl, nullptr, 0, d, true, false, s));
    }
    HIP_TRY(fused_pack_frames(w.fl, w.fb.Xp, w.Xt, d.Mk, s));
    const FusedBuffers& fb = w.fb;
    // the tail of the last launch of a solve in which nothing can stop: the caller's H written by the kernel itself, and on
    // k_fused_all the members' shares of Y formed from the activations in its registers (round 9), when B's bins fit
    // the instance's row tiles and the workspace holds the slabs; the packed activations are then stored only if somebody
    // reads them afterwards (finish_fused: the export of H, the two-pass synthesis)
    FusedLaunchTail lt{};
    if (t.direct_h) { lt.Hx = static_cast<double*>(c.H); lt.ldhx = c.ldh; lt.hx_frame_major = o.layout == EVC_FRAME_MAJOR ? 1 : 0; }
    if (t.y_in_kernel) { lt.Yb2p = w.B2p; lt.Yslab = w.Yslab; lt.y_stride = (long)w.flB.vp; lt.y_mt = w.flB.mtiles; }
    lt.skip_hp = t.skip_hp ? 1 : 0;
    // start values: caller-given ones were imported by the caller of this function; constants are either written
    // into the packed tiles here, or - first launch on k_fused_all, no residual wanted at init - formed by that kernel
    if (r.init_const) {
        if (!o.dict) HIP_TRY(fused_rowsum(w.At, d.Mk, d.M, d.N, fb.rsum, s));
    } else if (o.init_mode != EVC_INIT_GIVEN) {
        HIP_TRY(fused_fill_h(w.fl, fb.Hp, d.N, d.T_, w.u, s));
    }
    inf->kernel = r.kernel;
    inf->members = r.members;
    inf->exchange = r.members > 1 ? 1 : 0;         // then the caller checks the abort flag (one host round trip)
    AbortHook hook(r.members > 1 ? fb.coop_cnt + COOP_MAX_TILES : nullptr, o.test_abort_at);
    HIP_TRY(hook.begin(true, s));
    int first = 1;
    if (o.check_every > 0 && o.stop_rule == EVC_STOP_SKLEARN) {   // error_at_init
        HIP_TRY(fused_iterate(w.fl, fb, r, w.u, d.N, d.T_, 0, 1, 1, w.err2, o.eps_mode, o.eps, o.l1, 1, o.loss, s,
                              nullptr));
        HIP_TRY(utt_check(w.err2, w.u, n_utt, 0, o.check_every, o.stop_rule, o.tol, s));
        first = 0;
    }
    if (o.ev_loop_start) HIP_TRY(hipEventRecord((hipEvent_t)o.ev_loop_start, s));
    int done = 0;
    while (done < o.iters) {
        int n = o.iters - done;
        bool check = false;
        if (o.check_every > 0 && n >= o.check_every) { n = o.check_every; check = true; }
        const bool last = r.direct_export && done + n == o.iters;
        HIP_TRY(hook.before_launch(s));
        ++inf->launches;
        HIP_TRY(fused_iterate(w.fl, fb, r, w.u, d.N, d.T_, n, first, check ? 1 : 0, w.err2, o.eps_mode, o.eps, o.l1,
                              o.stop_rule == EVC_STOP_NONE ? 1 : 0, o.loss, s, last ? &lt : nullptr,
                              !(o.reserved & EVC_FLAG_NO_LONE_BIN), !(o.reserved & EVC_FLAG_NO_RANGE_HOIST),
                              !(o.reserved & EVC_FLAG_NO_QUAD_ROWS)));
        first = 0;
        done += n;
        if (check)
            HIP_TRY(utt_check(w.err2, w.u, n_utt, done / o.check_every, o.check_every, o.stop_rule,
                              o.tol, s));
    }
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord((hipEvent_t)o.ev_loop_stop, s));
    return ST_OK;
}

// tail of the fused path, as planned: H out of the packed tiles, Y from the members' slabs (summed), from the packed
// activations (the pre-pass with B's fragments, which fused_launches packed) or from frames-as-rows activations
int finish_fused(const Workspace<double>& w, const Dims& d, const evc_solve_opts& o, const FusedTail& t, double* H, int ldh,
                 const SynthArgs* y, int y_members, hipStream_t s) {
    const bool fm = (o.layout == EVC_FRAME_MAJOR);
    if (t.export_h) HIP_TRY(fused_export_h(w.fl, w.fb.Hp, H, ldh, fm ? 1 : 0, d.T_, d.N, s));
    switch (t.y_from) {
        case Y_SLABS:
            return fused_unpack_y(w.flB, w.Yslab, y_members, (long)w.flB.vp, d.T_, y->Mb, static_cast<double*>(y->Y), y->ldy,
                                  fm ? 1 : 0, s);
        case Y_PREPASS:
            return fused_synthesize(w.flB, w.B2p, w.fb.Hp, w.Yp, w.u, d.N, d.T_, y->Mb, static_cast<double*>(y->Y), y->ldy,
                                    fm ? 1 : 0, s);
        case Y_ROWS:
            HIP_TRY(fused_export_h(w.fl, w.fb.Hp, w.H0, d.Np, 1, d.T_, d.N, s));
            return synth_rows<double>(w.H0, d.Np, *y, d.N, d.T_, fm, s);
        default: return ST_OK;
    }
}

// The driver of the float64 fused kernels (M <= 32): activations live in the packed tile layout from start to finish.
// An exchange that was voided (plan_fused_tail says when the word is read) returns ST_COOP_TIMEOUT: solve_checked redoes.
int solve_fused(const SolveCall& c, const evc_solve_opts& o, const Route& r, evc_solve_info* inf) {
    Imported<double> im;
    HIP_TRY(import_call<double>(c, o, r, true, inf, &im));
    const Workspace<double>& w = im.w;
    const FusedRoute& fr = r.fused;
    double* H = static_cast<double*>(c.H);
    const bool given = o.init_mode == EVC_INIT_GIVEN;
    if (given)
        HIP_TRY(fused_import_h(w.fl, w.fb.Hp, H, c.ldh, o.layout == EVC_FRAME_MAJOR ? 1 : 0, c.T_, c.N, c.s));
    const FusedTail t = plan_fused_tail(fr, o.iters, given, H != nullptr, im.y != nullptr, w.packed_synth,
                                        w.Yslab && w.y_members == fr.members);
    inf->variant = t.variant;
    HIP_TRY(fused_launches(c, w, im.d, o, fr, t, im.y, inf));
    const int* abort_w = fr.members > 1 ? w.fb.coop_cnt + COOP_MAX_TILES : nullptr;     // (NULL: nothing was exchanged)
    int aborted = 0;
    if (abort_w && t.check_first) HIP_TRY(read_abort(abort_w, c.s, &aborted));
    if (!aborted) {
        HIP_TRY(finish_fused(w, im.d, o, t, H, c.ldh, im.y, fr.members, c.s));
        if (abort_w && !t.check_first) HIP_TRY(read_abort(abort_w, c.s, &aborted));
    }
    if (aborted) return ST_COOP_TIMEOUT;
    return copy_back(w.u, c.n_utt, im.n_slots, c.n_iter_out, c.err_out, c.s);
}

int device_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
    return cus;
}

// ------------------------------------------------------------------------------------------------------
// The wide fused path (float32, 32 < M <= 208, FACTORED): k_fused_wide (evc_wide.hip).  One launch per
// `check_every` iterations (a single launch when no residual is wanted); iteration 0 forms P and V = A H0.
// ------------------------------------------------------------------------------------------------------
template <typename T>
int solve_wide(const SolveCall& c, const evc_solve_opts& o, const Route& r, evc_solve_info* inf) {
    typedef WideKind<T> K;
    const int M = c.M, N = c.N, T_ = c.T_, n_utt = c.n_utt, ldh = c.ldh;
    hipStream_t s = c.s;
    const SynthArgs* y = c.y;
    T* H = static_cast<T*>(c.H);
    const Dims d = make_dims((int)sizeof(T), M, N, T_, n_utt, y ? y->Mb : 0);
    const int n_slots = n_slots_for(o.iters, o.check_every);
    if (n_slots > MAX_SLOTS) return ST_UNSUPPORTED;
    const int n_cus = r.n_cus;
    const bool kl = o.loss == EVC_LOSS_KL, fm = o.layout == EVC_FRAME_MAJOR;
    WideWs<T> w = carve_wide<T>(c.ws, d, MAX_SLOTS, n_cus, true, sizeof(T) == 4);
    if (w.bytes > c.ws_bytes) return ST_WORKSPACE;
    w.u.n_slots = n_slots;
    // tuning / tests: exemplar ranges per frame group, wavefronts per workgroup
    const typename K::Layout fl = K::layout(M, N, T_, n_cus, r.flags.c_req, r.flags.w_req);
    // (a prepared dictionary holds the block images of the DEFAULT layout: a tuning override of the wavefront / tile
    // count does not fit it - unsupported, not a workspace problem)
    if (!wide_fits(fl, w.caps)) return (o.dict && r.flags.w_req) ? ST_UNSUPPORTED : ST_WORKSPACE;

    HIP_TRY(utt_begin(w.u, c.utt_offsets, n_utt, d, o.iters, s));
    SynthArgs ydict;
    if (o.dict) {                 // the block images (and B) come from the prepared dictionary
        const DictArrays<T> ext = dict_arrays<T>(o.dict, 0);
        w.fb.Aw = K::image(ext);
        if (y && o.dict->Mb > 0) {
            ydict = *y;
            ydict.B = ext.Bc; ydict.ldb = o.dict->Mb; ydict.b_rows = 1;
            y = &ydict;
        }
        inf->prepared = 1;
    } else {
        HIP_TRY(copy2d<T>(static_cast<const T*>(c.A), c.lda, N, M, fm ? 0 : 1, w.At, d.Mk, d.Np, d.Mk, 0, s));
        if (kl) HIP_TRY(kl_scale_dict<T>(w.At, d.Mk, M, d.Np, o.eps, w.Akl, s));
        HIP_TRY(wide_pack_dict(fl, kl ? w.Akl : w.At, w.At, d.Mk, d.Np, w.fb.Aw, s));
    }
    HIP_TRY(copy2d<T>(static_cast<const T*>(c.X), c.ldx, T_, M, fm ? 0 : 1, w.Xt, d.Mk, d.Tp, d.Mk, 0, s));
    HIP_TRY(utt_start_values<T>(w.u, w.Xt, n_utt, d, o, s));
    HIP_TRY(wide_pack_x(fl, w.Xt, d.Mk, d.Tp, w.fb.Xw, s));
    const int init_const = o.init_mode == EVC_INIT_GIVEN ? 0 : 1;
    if (!init_const) HIP_TRY(wide_import_h(fl, w.fb.Hw, H, ldh, fm ? 1 : 0, T_, N, s));
    HIP_TRY(wide_begin(fl, w.fb, s));
    // (float64 only: correctly rounded quotients under pymf's stop rule or on request, as on the fused path)
    const bool exact = sizeof(T) == 8 && r.flags.exact_div;
    const int mode = (kl ? 100 : o.eps_mode) | (exact ? 0x1000 : 0);

    inf->kernel = K::kernel;
    inf->members = fl.c;
    inf->variant = wide_variant(fl, n_cus);
    inf->exchange = 1;               // tasks wait for tasks of other workgroups, whatever the number of ranges
    int* abort_w = reinterpret_cast<int*>(w.fb.ctl + 1);
    AbortHook hook(abort_w, o.test_abort_at);
    HIP_TRY(hook.begin(false, s));   // (wide_begin has cleared the flag)
    int next_it = 0;                 // first iteration not yet run (0 = the pass that forms P and V = A H0)
    auto run_to = [&](int it_end, int snap_every = 0, int snap_first = 0) -> int {      // iterations [next_it, it_end)
        if (it_end <= next_it) return 0;
        if constexpr (sizeof(T) == 4)
            HIP_TRY(wide_iterate(fl, w.fb, w.u, N, T_, next_it, it_end, mode, o.eps, o.l1, init_const, n_cus, s, snap_every,
                                 snap_first));
        else
            HIP_TRY(wide_iterate(fl, w.fb, w.u, N, T_, next_it, it_end, mode, o.eps, o.l1, init_const, n_cus, s));
        ++inf->launches;
        next_it = it_end;
        return 0;
    };
    // k_fused_wide: up to 1 + snap_slots stop checks per launch.  A launch boundary costs the task queue about one task
    // time (the tail of one launch and the head of the next do not overlap) plus the residual kernel: with a check every
    // 10 iterations that was 28 % of the STFT flow's default call at 16 utterances (profiles/r03_default_call_wide.jsonl).
    // The checks inside a launch are evaluated after it, in order; an utterance that stopped at one of them gets the
    // snapshot of that check back (k_wide_restore) - results are those of one launch per check, bit for bit.
    int checks_per_launch = 1;
    if constexpr (sizeof(T) == 4)
        if (o.check_every > 0 && !kl) checks_per_launch = 1 + w.fb.snap_slots;
    auto check = [&](int c) -> int {
        HIP_TRY(wide_err2(fl, w.fb, w.u, N, T_, next_it - 1, kl ? 1 : 0, o.eps, w.err2, s));
        HIP_TRY(utt_check(w.err2, w.u, n_utt, c, o.check_every, o.stop_rule, o.tol, s));
        return 0;
    };
    if (o.check_every > 0 && o.stop_rule == EVC_STOP_SKLEARN) {   // error_at_init, sklearn _nmf.py:827
        HIP_TRY(run_to(1));
        HIP_TRY(check(0));
    }
    if (o.ev_loop_start) HIP_TRY(hipEventRecord((hipEvent_t)o.ev_loop_start, s));
    int done = 0;
    while (done < o.iters) {
        int n = o.iters - done;
        bool chk = false;
        int L = 1;
        if (o.check_every > 0 && n >= o.check_every) {
            // the checks of a launch are speculation: iterations behind a check at which every utterance stopped are
            // thrown away.  The number grows with the iterations already done (1, 1, 2, 3, 4 ...: launches end at 10, 20,
            // 40, 70, 110, 150 of the default call), so at most a third of a solve's iterations are wasted
            L = 1 + done / (2 * o.check_every);
            if (L > checks_per_launch) L = checks_per_launch;
            if (L > n / o.check_every) L = n / o.check_every;
            n = L * o.check_every;
            chk = true;
        }
        HIP_TRY(hook.before_launch(s));
        HIP_TRY(L > 1 ? run_to(done + n + 1, o.check_every, done + o.check_every) : run_to(done + n + 1));
        if constexpr (sizeof(T) == 4) {
            for (int k = 0; k + 1 < L; ++k) {      // the checks inside the launch, oldest first
                const int cno = done / o.check_every + 1 + k;
                HIP_TRY(utt_check(w.fb.err2s + (size_t)k * w.fb.err_stride, w.u, n_utt, cno, o.check_every, o.stop_rule,
                                  o.tol, s));
                if (o.stop_rule != EVC_STOP_NONE) HIP_TRY(wide_restore(fl, w.fb, w.u, k, cno * o.check_every, T_, s));
            }
        }
        done += n;
        if (chk) HIP_TRY(check(done / o.check_every));
    }
    HIP_TRY(run_to(1));               // iters == 0: the start values still have to exist
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord((hipEvent_t)o.ev_loop_stop, s));
    // A bounded wait that ran out (a wedged or oversubscribed device) voids the solve: the flag is read back before
    // anything reaches the caller's H or Y - one host round trip per solve, as for the other exchanging kernels
    // (include/evc.h, Host synchronisation) - and the caller of this function redoes the solve on the two contractions
    // from the untouched inputs.  (Round 3 exported NaN under status 0.)
    int aborted = 0;
    HIP_TRY(read_abort(abort_w, s, &aborted));
    if (aborted) return ST_COOP_TIMEOUT;
    const int* abort = abort_w;
    if (H) HIP_TRY(wide_export_h(fl, w.fb.Hw, H, ldh, fm ? 1 : 0, T_, N, abort, s));
    if (y) {
        HIP_TRY(wide_export_h(fl, w.fb.Hw, w.H0, d.Np, 1, T_, N, abort, s));
        HIP_TRY(synth_rows<T>(w.H0, d.Np, *y, N, T_, fm, s));
    }
    return copy_back(w.u, n_utt, n_slots, c.n_iter_out, c.err_out, s);
}

template <typename T> int gemm_kernel_id() {
#if defined(EVC_DIAG_GEMM_V1)
    return EVC_KERNEL_GEMM_NT;
#elif defined(EVC_DIAG_GEMM2_F64)
    return EVC_KERNEL_GEMM2;
#else
    return sizeof(T) == 4 ? EVC_KERNEL_GEMM2 : EVC_KERNEL_GEMM_NT;
#endif
}

// The two contractions per iteration (any M, both dtypes): activations frames-as-rows, Ht[t][n]
template <typename T>
int solve_gemm(const SolveCall& c, const evc_solve_opts& o, const Route& r, evc_solve_info* inf) {
    Imported<T> im;
    HIP_TRY(import_call<T>(c, o, r, false, inf, &im));
    const Workspace<T>& w = im.w;
    const Dims& d = im.d;
    const SynthArgs* y = im.y;
    const int M = c.M, N = c.N, T_ = c.T_, n_utt = c.n_utt, ldh = c.ldh, algo = r.algo;
    hipStream_t s = c.s;
    T* H = static_cast<T*>(c.H);
    const bool fm = (o.layout == EVC_FRAME_MAJOR), kl = (o.loss == EVC_LOSS_KL);

    if (o.init_mode == EVC_INIT_GIVEN)
        HIP_TRY(copy2d<T>(H, ldh, T_, N, fm ? 0 : 1, w.H0, d.Np, d.Tp, d.Np, 0, s));
    else
        HIP_TRY(fill_h0<T>(w.H0, d.Np, d.Tp, N, T_, w.u, s));

    // ---- numerator (and Gram matrix) ----
    const bool gram = (algo == EVC_ALGO_GRAM || algo == EVC_ALGO_LITERAL);
    if (gram) HIP_TRY(gemm_nt<T>(w.At, d.Mk, w.At, d.Mk, w.G, d.Np, d.Np, d.Np, d.Mk, s));
    // what the launchers chose (evc_gemm_plan.h), for evc_solve_info.variant: the numerator, V = H Am^T in the loop, the update
    GemmPlan plan_p{}, plan_v{}, plan_u{};
    if (!kl) HIP_TRY(gemm_nt<T>(w.Xt, d.Mk, w.At, d.Mk, w.Pt, d.Np, d.Tp, d.Np, d.Mk, s, nullptr, 0, nullptr, 0, nullptr, &plan_p));

    T* Hc = w.H0;       // current activations
    T* Hn = w.H1;       // ping-pong partner (GRAM only)
    bool v_valid = false;

    auto residual_check = [&](int c) -> int {
        // (the V of a check serves the next iteration of FACTORED / KL: reported as the loop's; GRAM / LITERAL report none)
        if (!v_valid) HIP_TRY(gemm_nt<T>(Hc, d.Np, w.Am, d.Np, w.Vt, d.Mj, d.Tp, d.Mj, d.Np, s, w.Vsplit, w.vsplit_elems, nullptr, d.Mk,
                                         nullptr, gram ? nullptr : &plan_v));
        v_valid = true;
        if (kl) HIP_TRY(frame_err_kl<T>(w.Xt, d.Mk, w.Vt, d.Mj, M, T_, o.eps, w.err2, s));
        else HIP_TRY(frame_err2<T>(w.Xt, d.Mk, w.Vt, d.Mj, M, T_, w.err2, s));
        HIP_TRY(utt_check(w.err2, w.u, n_utt, c, o.check_every, o.stop_rule, o.tol, s));
        return 0;
    };

    if (o.check_every > 0 && o.stop_rule == EVC_STOP_SKLEARN) {
        HIP_TRY(residual_check(0));     // error_at_init, sklearn _nmf.py:827
    }

    MuEpilogue<T> ep;
    ep.P = w.Pt; ep.frame_utt = w.u.frame_utt; ep.active = w.u.active; ep.ldh = d.Np;
    ep.N = N; ep.T_ = T_; ep.eps_mode = o.eps_mode; ep.eps = (T)o.eps; ep.l1 = (T)o.l1; ep.kl = kl ? 1 : 0;
    // Once the stop rules have stopped every utterance the launches still queued return at once (the host does not
    // read the flags back: the call stays asynchronous).  In-place path only: GRAM swaps its two H buffers per launch.
    const int* gate = (!gram && o.check_every > 0 && o.stop_rule != EVC_STOP_NONE) ? w.u.active + n_utt : nullptr;
    ep.gate = gate;

    inf->kernel = gemm_kernel_id<T>();
    inf->members = 1;
    inf->launches = o.iters * (gram ? 1 : 2);
    if (o.ev_loop_start) HIP_TRY(hipEventRecord((hipEvent_t)o.ev_loop_start, s));
    for (int it = 1; it <= o.iters; ++it) {
        if (algo == EVC_ALGO_LITERAL) {   // pymf nmf.py:68-69 recomputes both every iteration
            HIP_TRY(gemm_nt<T>(w.At, d.Mk, w.At, d.Mk, w.G, d.Np, d.Np, d.Np, d.Mk, s));
            HIP_TRY(gemm_nt<T>(w.Xt, d.Mk, w.At, d.Mk, w.Pt, d.Np, d.Tp, d.Np, d.Mk, s));
        }
        if (gram) {
            ep.Hin = Hc;                  // H' = mu(H, P, H G^T)   (G symmetric)
            HIP_TRY(gemm_nt_mu<T>(Hc, d.Np, w.G, d.Np, Hn, d.Tp, d.Np, d.Np, ep, s, &plan_u));
            T* tmp = Hc; Hc = Hn; Hn = tmp;
        } else {
            if (!v_valid) HIP_TRY(gemm_nt<T>(Hc, d.Np, w.Am, d.Np, w.Vt, d.Mj, d.Tp, d.Mj, d.Np, s, w.Vsplit, w.vsplit_elems, nullptr, d.Mk, gate, &plan_v));
            ep.Hin = Hc;
            if (kl) {                     // H' = H (.) (X (/) max(V, eps)) (A / colsum)   sklearn _nmf.py:556-606
                HIP_TRY(kl_ratio<T>(w.Xt, d.Mk, w.Vt, d.Mj, M, d.Tp, o.eps, w.Rt, d.Mk, s));
                HIP_TRY(gemm_nt_mu<T>(w.Rt, d.Mk, w.Akl, d.Mk, Hc, d.Tp, d.Np, d.Mk, ep, s, &plan_u));
            } else {                      // H' = mu(H, P, V At^T), V = H Am^T ; in place
                HIP_TRY(gemm_nt_mu<T>(w.Vt, d.Mj, w.At, d.Mk, Hc, d.Tp, d.Np, d.Mk, ep, s, &plan_u));
            }
        }
        v_valid = false;
        if (o.check_every > 0 && it % o.check_every == 0) HIP_TRY(residual_check(it / o.check_every));
    }

    inf->variant = gemm_variant(plan_u, plan_v, plan_p);
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord((hipEvent_t)o.ev_loop_stop, s));
    if (H) HIP_TRY(copy2d<T>(Hc, d.Np, d.T_, d.N, 0, H, ldh, d.T_, d.N, fm ? 0 : 1, s));
    if (y) HIP_TRY(synth_rows<T>(Hc, d.Np, *y, d.N, d.T_, fm, s));
    return copy_back(w.u, n_utt, im.n_slots, c.n_iter_out, c.err_out, s);
}

template <typename T>
hipError_t synthesize_typed(const void* B_, int ldb, const void* H_, int ldh, void* Y_, int ldy, int Mb, int N, int T_,
                            bool fm, hipStream_t s) {
    const T* B = static_cast<const T*>(B_);
    const T* H = static_cast<const T*>(H_);
    T* Y = static_cast<T*>(Y_);
    if (Mb <= 64) {     // a handful of bins: one pass over H, wavefronts split the exemplars (k_synth_skinny)
        // FRAME_MAJOR: H[t][n], B[n][mb], Y[t][mb];  BIN_MAJOR: H[n][t], B[mb][n], Y[mb][t]
        const long hst = fm ? ldh : 1, hsn = fm ? 1 : ldh, bsn = fm ? ldb : 1, bsm = fm ? 1 : ldb;
        const long yst = fm ? ldy : 1, ysm = fm ? 1 : ldy;
        return synth_skinny<T>(H, hst, hsn, B, bsn, bsm, Y, yst, ysm, T_, Mb, N, s);
    }
    // Y[t][mb] = sum_n H[t][n] B[n][mb]           (np.matmul(H.T, B), 04_align_n_nmf.py:391)
    if (fm) return gemm_strided<T>(H, ldh, 1, B, 1, ldb, Y, ldy, 1, T_, Mb, N, s);
    // Y[mb][t] = sum_n B[mb][n] H[n][t]
    return gemm_strided<T>(B, ldb, 1, H, 1, ldh, Y, ldy, 1, Mb, T_, N, s);
}

template <typename T>
int residual_typed(const void* A, int lda, const void* X, int ldx, const void* H, int ldh, int M, int N, int T_, bool fm,
                   double* err2_out, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const Dims d = make_dims((int)sizeof(T), M, N, T_, 1, 0);
    Workspace<T> w = carve<T>(workspace, d, EVC_ALGO_FACTORED, MAX_SLOTS, false);
    if (w.bytes > workspace_bytes) return ST_WORKSPACE;
    HIP_TRY(copy2d<T>((const T*)A, lda, M, N, fm ? 1 : 0, w.Am, d.Np, d.Mj, d.Np, 0, s));
    HIP_TRY(copy2d<T>((const T*)X, ldx, T_, M, fm ? 0 : 1, w.Xt, d.Mk, d.Tp, d.Mk, 0, s));
    HIP_TRY(copy2d<T>((const T*)H, ldh, T_, N, fm ? 0 : 1, w.H0, d.Np, d.Tp, d.Np, 0, s));
    HIP_TRY(gemm_nt<T>(w.H0, d.Np, w.Am, d.Np, w.Vt, d.Mj, d.Tp, d.Mj, d.Np, s, nullptr, 0, nullptr, d.Mk));
    HIP_TRY(frame_err2<T>(w.Xt, d.Mk, w.Vt, d.Mj, M, T_, err2_out, s));
    return ST_OK;
}

}  // namespace

extern "C" {

int evc_version(void) { return EVC_VERSION; }

const char* evc_strerror(int status) {
    switch (status) {
        case ST_OK: return "ok";
        case ST_BADARG: return "invalid argument";
        case ST_WORKSPACE: return "workspace too small (see evc_workspace_bytes)";
        case ST_UNSUPPORTED: return "unsupported option combination";
        case ST_COOP_TIMEOUT: return "cooperative launch timed out waiting for a peer workgroup (results void)";
        default: break;
    }
    if (status > 0) return hipGetErrorString((hipError_t)status);
    return "unknown status";
}

int evc_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    return e == hipSuccess ? n : -(int)e;
}

size_t evc_workspace_bytes(int M, int Mb, int N, int T, int n_utt, int dtype, int algo) {
    if (M < 0 || Mb < 0 || N < 0 || T < 0 || n_utt < 1) return 0;
    if (algo < EVC_ALGO_GRAM || algo > EVC_ALGO_AUTO) return 0;
    // (the device is asked only where the count sizes something: the task queues' workspace)
    const int n_cus = wide_family(M, N, T, dtype, algo_eff(algo), EVC_LOSS_FROBENIUS) ? device_cus() : 0;
    if (dtype == EVC_F64) return workspace_typed<double>(M, Mb, N, T, n_utt, algo, n_cus);
    if (dtype != EVC_F32) return 0;
    size_t b = workspace_typed<float>(M, Mb, N, T, n_utt, algo, n_cus);
    if (small_family(M, N, T, algo_eff(algo)))
        b = std::max(b, f32_staging_bytes(M, Mb, N, T) + workspace_typed<double>(M, Mb, N, T, n_utt, algo, n_cus));
    return b;
}

// float32 callers on the float64 fused kernels (f32_staging_bytes, evc_solve_plan.h): the staged call, the fused driver,
// and H / Y narrowed on the way out - unless the exchange was voided: then nothing reaches the caller's H or Y
static int solve_f32_on_f64(const SolveCall& call, const evc_solve_opts& o, const Route& r, evc_solve_info* inf) {
    const int M = call.M, N = call.N, T = call.T_, ldh = call.ldh;
    const SynthArgs* y = call.y;
    void* H = call.H;
    hipStream_t s = call.s;
    const bool fm = (o.layout == EVC_FRAME_MAJOR);
    const int Mb = y ? y->Mb : 0;
    const size_t stage = f32_staging_bytes(M, Mb, N, T);
    if (call.ws_bytes < stage) return ST_WORKSPACE;
    // staged matrices keep the caller's orientation with compact rows: (outer, inner) per layout
    const long aR = fm ? N : M, aC = fm ? M : N, xR = fm ? T : M, xC = fm ? M : T, hR = fm ? T : N, hC = fm ? N : T;
    const long bR = fm ? N : Mb, bC = fm ? Mb : N, yR = fm ? T : Mb, yC = fm ? Mb : T;
    Carver c{static_cast<char*>(call.ws), 0};
    double* A64 = c.take<double>((size_t)N * M);
    double* X64 = c.take<double>((size_t)T * M);
    double* H64 = c.take<double>((size_t)T * N);
    double* B64 = c.take<double>((size_t)N * Mb);
    double* Y64 = c.take<double>((size_t)T * Mb);
    if (!o.dict) HIP_TRY((cvt2d<float, double>(static_cast<const float*>(call.A), call.lda, aR, aC, A64, aC, s)));
    HIP_TRY((cvt2d<float, double>(static_cast<const float*>(call.X), call.ldx, xR, xC, X64, xC, s)));
    if (H && o.init_mode == EVC_INIT_GIVEN)
        HIP_TRY((cvt2d<float, double>(static_cast<const float*>(H), ldh, hR, hC, H64, hC, s)));
    SynthArgs y64{};
    if (y) {
        if (!(o.dict && o.dict->Mb > 0))
            HIP_TRY((cvt2d<float, double>(static_cast<const float*>(y->B), y->ldb, bR, bC, B64, bC, s)));
        y64 = SynthArgs{B64, (int)bC, Y64, (int)yC, Mb};
    }
    evc_solve_opts o64 = o;
    o64.dtype = EVC_F64;
    const SolveCall staged{A64, (int)aC, X64, (int)xC, H ? H64 : nullptr, (int)hC, M, N, T, call.utt_offsets, call.n_utt,
                           static_cast<char*>(call.ws) + stage, call.ws_bytes - stage, call.n_iter_out, call.err_out,
                           y ? &y64 : nullptr, s};
    HIP_TRY(solve_fused(staged, o64, r, inf));
    if (H) HIP_TRY((cvt2d<double, float>(H64, hC, hR, hC, static_cast<float*>(H), ldh, s)));
    if (y) HIP_TRY((cvt2d<double, float>(Y64, yC, yR, yC, static_cast<float*>(y->Y), y->ldy, s)));
    if (call.n_iter_out || call.err_out) HIP_TRY(hipStreamSynchronize(s));    // those calls are synchronous: so are H and Y
    return ST_OK;
}

// ---- prepared dictionaries ----
size_t evc_dict_bytes(int M, int Mb, int N, int dtype, int loss) {
    if (M < 1 || Mb < 0 || N < 1) return 0;
    if (loss != EVC_LOSS_FROBENIUS && loss != EVC_LOSS_KL) return 0;
    if (dtype == EVC_F64) return dict_image<double>(nullptr, 0, M, Mb, N, loss).bytes;
    if (dtype != EVC_F32) return 0;
    if (small_family(M, N, 1, EVC_ALGO_FACTORED))     // widened once, then the float64 image
        return dict_image<double>(nullptr, dict_f64_staging(M, Mb, N), M, Mb, N, loss).bytes;
    return dict_image<float>(nullptr, 0, M, Mb, N, loss).bytes;
}

int evc_dict_prepare(const void* A, int lda, const void* B, int ldb, int M, int Mb, int N, int layout, int dtype, int loss,
                     double eps, void* mem, size_t mem_bytes, evc_dict* dict, evc_stream_t stream) {
    if (!A || !mem || !dict || M < 1 || N < 1 || Mb < 0 || (Mb > 0) != (B != nullptr)) return ST_BADARG;
    if (layout != EVC_FRAME_MAJOR && layout != EVC_BIN_MAJOR) return ST_BADARG;
    if (bad_ld(layout, lda, N, M) || (B && bad_ld(layout, ldb, N, Mb))) return ST_BADARG;
    if (loss == EVC_LOSS_KL && !(eps > 0.0)) return ST_UNSUPPORTED;
    const size_t need = evc_dict_bytes(M, Mb, N, dtype, loss);
    if (need == 0) return ST_BADARG;
    if (mem_bytes < need || (reinterpret_cast<uintptr_t>(mem) & 255)) return ST_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool fm = layout == EVC_FRAME_MAJOR;
    if (dtype == EVC_F64) {
        HIP_TRY(dict_prepare_typed<double>(static_cast<const double*>(A), lda, static_cast<const double*>(B), ldb, M, Mb, N,
                                           fm, loss, eps, mem, 0, s));
    } else if (small_family(M, N, 1, EVC_ALGO_FACTORED)) {
        // widen A and B once (compact rows in the caller's orientation), then the float64 image behind them
        Carver c{static_cast<char*>(mem), 0};
        double* A64 = c.take<double>((size_t)N * M);
        double* B64 = c.take<double>((size_t)N * Mb);
        const long aR = fm ? N : M, aC = fm ? M : N, bR = fm ? N : Mb, bC = fm ? Mb : N;
        HIP_TRY((cvt2d<float, double>(static_cast<const float*>(A), lda, aR, aC, A64, aC, s)));
        if (B) HIP_TRY((cvt2d<float, double>(static_cast<const float*>(B), ldb, bR, bC, B64, bC, s)));
        HIP_TRY(dict_prepare_typed<double>(A64, (int)aC, B ? B64 : nullptr, (int)bC, M, Mb, N, fm, loss, eps, mem,
                                           dict_f64_staging(M, Mb, N), s));
    } else {
        HIP_TRY(dict_prepare_typed<float>(static_cast<const float*>(A), lda, static_cast<const float*>(B), ldb, M, Mb, N, fm,
                                          loss, eps, mem, 0, s));
    }
    dict->struct_bytes = (int)sizeof(evc_dict);
    dict->magic = DICT_MAGIC;
    dict->M = M; dict->Mb = Mb; dict->N = N; dict->dtype = dtype; dict->loss = loss; dict->reserved = 0;
    dict->eps = loss == EVC_LOSS_KL ? eps : 0.0;
    dict->mem = mem;
    dict->bytes = need;
    return ST_OK;
}

// The argument checks of evc_nmf_solve / evc_nmf_convert, the route, the driver - and the one redo path: a driver whose
// exchange was voided returns ST_COOP_TIMEOUT and the call is planned and run again without what was voided.
static int solve_checked(const SolveCall& c, const evc_solve_opts* opts) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_solve_opts)) return ST_BADARG;
    const evc_solve_opts& o = *opts;
    const int M = c.M, N = c.N, T = c.T_, n_utt = c.n_utt;
    const SynthArgs* y = c.y;
    if (M < 1 || N < 1 || T < 0 || n_utt < 1 || o.iters < 0) return ST_BADARG;
    if (o.dtype != EVC_F64 && o.dtype != EVC_F32) return ST_BADARG;
    if (o.layout != EVC_FRAME_MAJOR && o.layout != EVC_BIN_MAJOR) return ST_BADARG;
    if (o.algo < EVC_ALGO_GRAM || o.algo > EVC_ALGO_AUTO) return ST_BADARG;
    if (o.eps_mode < EVC_EPS_ADD || o.eps_mode > EVC_EPS_CLAMP) return ST_BADARG;
    if (o.init_mode < EVC_INIT_GIVEN || o.init_mode > EVC_INIT_CONST) return ST_BADARG;
    if (o.stop_rule < EVC_STOP_NONE || o.stop_rule > EVC_STOP_PYMF) return ST_BADARG;
    if (o.check_every < 0) return ST_BADARG;
    if (o.stop_rule != EVC_STOP_NONE && o.check_every == 0) return ST_BADARG;
    if (!(o.l1 >= 0.0)) return ST_BADARG;
    if (o.loss != EVC_LOSS_FROBENIUS && o.loss != EVC_LOSS_KL) return ST_BADARG;
    if (o.loss == EVC_LOSS_KL) {   // sklearn's KL update: its guards, no Gram shortcut, no (quirky) L1
        if (o.eps_mode != EVC_EPS_ZERO_REPLACE || o.l1 != 0.0 || !(o.eps > 0.0)) return ST_UNSUPPORTED;
        if (o.algo == EVC_ALGO_GRAM || o.algo == EVC_ALGO_LITERAL) return ST_UNSUPPORTED;
    }
    if (y && y->Mb < 1) return ST_BADARG;
    if (o.info && o.info->struct_bytes != (int)sizeof(evc_solve_info)) return ST_BADARG;
    if (T == 0) {
        if (c.n_iter_out) for (int i = 0; i < n_utt; ++i) c.n_iter_out[i] = 0;
        return ST_OK;
    }
    const Route route = plan_route(M, N, T, o.dtype, o, device_cus());
    const evc_dict* dk = o.dict;
    if (dk) {         // a prepared dictionary replaces the A (and B) arguments
        if (dk->struct_bytes != (int)sizeof(evc_dict) || dk->magic != DICT_MAGIC || !dk->mem) return ST_BADARG;
        if (dk->M != M || dk->N != N || dk->dtype != o.dtype || dk->loss != o.loss) return ST_BADARG;
        if (o.loss == EVC_LOSS_KL && dk->eps != o.eps) return ST_BADARG;
        if (y && dk->Mb > 0 && dk->Mb != y->Mb) return ST_BADARG;
        if (dk->bytes < evc_dict_bytes(M, dk->Mb, N, dk->dtype, dk->loss)) return ST_BADARG;
        // a float32 dictionary with M <= 32 was widened for the float64 fused kernels: only that route is prepared
        if (o.dtype == EVC_F32 && small_family(M, N, T, EVC_ALGO_FACTORED) && !route.staged) return ST_UNSUPPORTED;
    }
    if ((!dk && !c.A) || !c.X || !c.ws) return ST_BADARG;
    if (!c.H && (!y || o.init_mode == EVC_INIT_GIVEN)) return ST_BADARG;   // H may be omitted by evc_nmf_convert only
    if ((!dk && bad_ld(o.layout, c.lda, N, M)) || bad_ld(o.layout, c.ldx, T, M) || (c.H && bad_ld(o.layout, c.ldh, T, N)))
        return ST_BADARG;
    if (y && (!y->Y || bad_ld(o.layout, y->ldy, T, y->Mb))) return ST_BADARG;
    if (y && !(dk && dk->Mb > 0) && (!y->B || bad_ld(o.layout, y->ldb, N, y->Mb))) return ST_BADARG;
    if (!utt_offsets_ok(c.utt_offsets, n_utt, T)) return ST_BADARG;
    // tuning bits 16..19: wavefronts per workgroup of k_fused_wide (4 | 8), whole bin tiles per wavefront of
    // k_fused_wide64 (4 | 5 | 7 | 8: the narrowest instance >= the request that holds M); anything else is an error
    const int tw = route.flags.w_req;
    if (M > 32 && tw != 0 && !(o.dtype == EVC_F32 ? (tw == 4 || tw == 8) : (tw == 3 || tw == 4 || tw == 5 || tw == 7 || tw == 8)))
        return ST_BADARG;
    evc_solve_info inf{};
    // one signature: the task queues, the float64 fused kernels (float32 callers staged onto them), the two contractions
    auto run = [&](const Route& r, const evc_solve_opts& oo) -> int {
        const bool f64 = o.dtype == EVC_F64;
        auto driver = f64 ? solve_gemm<double> : solve_gemm<float>;
        switch (r.family) {
            case ROUTE_WIDE: driver = f64 ? solve_wide<double> : solve_wide<float>; break;
            case ROUTE_FUSED: driver = r.staged ? solve_f32_on_f64 : solve_fused; break;
            default: break;
        }
        return driver(c, oo, r, &inf);
    };
    int st = run(route, o);
    if (st == ST_COOP_TIMEOUT && route.family != ROUTE_GEMM) {
        // A bounded wait that ran out voids the attempt.  The task queues have written nothing to H or Y and are redone on
        // the two contractions; a fused attempt is redone with one workgroup per frame tile (no exchange), from the
        // caller's inputs, which it has left as they were (its tail may have written void values to H / Y when the start
        // values were not the caller's: the redo writes them again).  A and X are imported again: the failure path.
        evc_solve_opts redo_o = o;
        redo_o.reserved |= route.family == ROUTE_WIDE ? EVC_FLAG_NO_FUSED : EVC_FLAG_NO_EXCHANGE;
        redo_o.test_abort_at = 0;
        const int launches = inf.launches;
        inf = evc_solve_info{};
        st = run(plan_route(M, N, T, o.dtype, redo_o, route.n_cus), redo_o);
        inf.redo = 1;
        inf.launches += launches;
    }
    if (o.info && o.info->struct_bytes == (int)sizeof(evc_solve_info)) {
        inf.struct_bytes = (int)sizeof(evc_solve_info);
        *o.info = inf;
    }
    return st;
}

int evc_nmf_solve(const void* A, int lda, const void* X, int ldx, void* H, int ldh, int M, int N,
                  int T, const int* utt_offsets, int n_utt, const evc_solve_opts* opts,
                  void* workspace, size_t workspace_bytes, int* n_iter_out, double* err_out,
                  evc_stream_t stream) {
    const SolveCall c{A, lda, X, ldx, H, ldh, M, N, T, utt_offsets, n_utt, workspace, workspace_bytes, n_iter_out, err_out,
                      nullptr, reinterpret_cast<hipStream_t>(stream)};
    return solve_checked(c, opts);
}

int evc_nmf_convert(const void* A, int lda, const void* X, int ldx, const void* B, int ldb, void* H,
                    int ldh, void* Y, int ldy, int M, int Mb, int N, int T, const int* utt_offsets,
                    int n_utt, const evc_solve_opts* opts, void* workspace, size_t workspace_bytes,
                    int* n_iter_out, double* err_out, evc_stream_t stream) {
    const SynthArgs y{B, ldb, Y, ldy, Mb};
    const SolveCall c{A, lda, X, ldx, H, ldh, M, N, T, utt_offsets, n_utt, workspace, workspace_bytes, n_iter_out, err_out,
                      &y, reinterpret_cast<hipStream_t>(stream)};
    return solve_checked(c, opts);
}

int evc_synthesize(const void* B, int ldb, const void* H, int ldh, void* Y, int ldy, int Mb, int N,
                   int T, int layout, int dtype, evc_stream_t stream) {
    if (Mb < 1 || N < 0 || T < 0) return ST_BADARG;
    if (layout != EVC_FRAME_MAJOR && layout != EVC_BIN_MAJOR) return ST_BADARG;
    if (dtype != EVC_F64 && dtype != EVC_F32) return ST_BADARG;
    if (T == 0) return ST_OK;
    if (!Y || (N > 0 && (!B || !H))) return ST_BADARG;
    if (bad_ld(layout, ldb, N, Mb) || bad_ld(layout, ldh, T, N) || bad_ld(layout, ldy, T, Mb))
        return ST_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool fm = layout == EVC_FRAME_MAJOR;
    return (int)(dtype == EVC_F64 ? synthesize_typed<double> : synthesize_typed<float>)(B, ldb, H, ldh, Y, ldy, Mb, N, T, fm, s);
}

int evc_residual(const void* A, int lda, const void* X, int ldx, const void* H, int ldh, int M,
                 int N, int T, int layout, int dtype, double* err2_out, void* workspace,
                 size_t workspace_bytes, evc_stream_t stream) {
    if (M < 1 || N < 1 || T < 0) return ST_BADARG;
    if (layout != EVC_FRAME_MAJOR && layout != EVC_BIN_MAJOR) return ST_BADARG;
    if (dtype != EVC_F64 && dtype != EVC_F32) return ST_BADARG;
    if (T == 0) return ST_OK;
    if (!A || !X || !H || !err2_out || !workspace) return ST_BADARG;
    if (bad_ld(layout, lda, N, M) || bad_ld(layout, ldx, T, M) || bad_ld(layout, ldh, T, N))
        return ST_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool fm = (layout == EVC_FRAME_MAJOR);
    return (dtype == EVC_F64 ? residual_typed<double> : residual_typed<float>)(A, lda, X, ldx, H, ldh, M, N, T, fm, err2_out,
                                                                               workspace, workspace_bytes, s);
}

}  // extern "C"
