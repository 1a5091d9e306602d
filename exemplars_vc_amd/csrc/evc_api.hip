// C ABI of libevc_hip.so (see include/evc.h): argument checking, workspace carving and the
// launch sequence of one activation solve.  No allocation, no global state, no exceptions.
// (The entries that learn the dictionary too sit with their kernels: evc_learn.hip, evc_cd.hip, evc_beta_learn.hip.)
#include "evc_internal.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>

using namespace evc;

namespace {

constexpr int DICT_MAGIC = 0x45564344;      // "EVCD"

// What a solve needs of the dictionary, whatever the frames are.  Carved from the call's workspace and filled on every
// call, or - with a prepared dictionary (evc_dict_prepare) - carved from its image, filled once.
struct DictPlan {
    bool fused;          // float64 fused kernels (M <= 32): operand fragments, row sums
    bool packed_b;       // ... and B's fragments for the synthesis from packed tiles (1 <= Mb <= 32)
    bool wide;           // k_fused_wide's block images (float32, 32 < M <= 208)
    bool wide64;         // k_fused_wide64's block images (float64, 144 < M <= 528, Frobenius)
    bool kl;             // the dictionary divided by its column sums
    bool bc;             // a compact exemplars-as-rows copy of B (prepared images: the caller's B is not consulted)
};
template <typename T> struct DictArrays {
    T *At, *Am, *Akl;
    double *A1p, *A2p, *rsum;
    T* Bt;
    double *B1p, *B2p;
    T* Bc;
    float* Aw;
    double* Aw64;
};
int algo_eff(int algo) { return algo == EVC_ALGO_AUTO ? EVC_ALGO_FACTORED : algo; }
// Which kernels a (M, N, T) problem of one dtype can be routed to.  plan_route, the workspace and dictionary size queries
// and the prepared images all ask these two, so that a new route family is added here and in plan_route only.
// The float64 fused kernels (M <= 32); float32 callers ride them through a staging copy (solve_f32_on_f64).
bool small_family(int M, int N, int T_, int algo) { return algo == EVC_ALGO_FACTORED && fused_supported(M, N, T_, EVC_F64); }
// the task-queue kernels: k_fused_wide (float32), k_fused_wide64 (float64)
bool wide_family(int M, int N, int T_, int dtype, int algo, int loss) {
    return dtype == EVC_F64 ? wide64_supported(M, N, T_, dtype, algo, loss) : wide_supported(M, N, T_, dtype, algo);
}

// the plan of a prepared image (arithmetic type T): every layout a later solve of any size may be routed to
template <typename T> DictPlan dict_plan(int M, int Mb, int N, int loss) {
    const int dt = sizeof(T) == 8 ? EVC_F64 : EVC_F32;
    DictPlan p{};
    p.kl = loss == EVC_LOSS_KL;
    p.fused = sizeof(T) == 8 && small_family(M, N, 1, EVC_ALGO_FACTORED);
    p.packed_b = p.fused && Mb >= 1 && Mb <= 32;
    p.wide = sizeof(T) == 4 && wide_family(M, N, 1, dt, EVC_ALGO_FACTORED, loss);
    p.wide64 = sizeof(T) == 8 && wide_family(M, N, 1, dt, EVC_ALGO_FACTORED, loss);
    p.bc = Mb >= 1;
    return p;
}
template <typename T> DictArrays<T> take_dict(Carver& c, const Dims& d, const DictPlan& p) {
    DictArrays<T> a{};
    a.At = c.take<T>((size_t)d.Np * d.Mk);
    a.Am = c.take<T>((size_t)d.Mj * d.Np);
    a.Akl = c.take<T>((size_t)d.Np * d.Mk);
    if (p.fused) {
        const FusedLayout fl = fused_layout(d.M, d.N, 1);
        a.A1p = c.take<double>(fl.a1);
        a.A2p = c.take<double>(fl.a2);
        a.rsum = c.take<double>(32);
    }
    if (p.packed_b) {
        const FusedLayout flB = fused_layout(d.Mb, d.N, 1);
        a.Bt = c.take<T>((size_t)d.Np * 32);
        a.B1p = c.take<double>(flB.a1);
        a.B2p = c.take<double>(flB.a2);
    }
    if (p.wide) a.Aw = c.take<float>(wide_layout(d.M, d.N, 1, 256, 0, 0).aw);
    if (p.wide64) a.Aw64 = c.take<double>(wide64_layout(d.M, d.N, 1, 256, 0, 0).aw);
    if (p.bc) a.Bc = c.take<T>((size_t)d.N * d.Mb);
    return a;
}

template <typename T> struct Workspace {
    T *At, *Am, *Xt, *H0, *H1, *Pt, *G, *Vt;
    T *Akl, *Rt;         // KL: dictionary / column sums, and X / max(V, eps)
    T* Vsplit;           // split-K slabs of V = H Am^T when there are few frames
    size_t vsplit_elems;
    double* err2;
    UttState u;
    FusedLayout fl;
    FusedBuffers fb;
    // synthesis from the packed activations (fused path, Mb <= 32)
    FusedLayout flB;
    T* Bt;
    double *B1p, *B2p, *Yp;
    // k_fused_all forming Y at the end of its last launch: one Yp image per member (NULL: not for these sizes); carved
    // last, so that a workspace of bytes_min holds everything else at the same place (Yp itself serves one member)
    double* Yslab;
    int y_members;
    bool fused, packed_synth;
    size_t bytes, bytes_min;
};

UttState take_utt(Carver& c, const Dims& d, int n_slots) {
    UttState u;
    u.frame_utt = c.take<int>(d.Tp);
    u.offsets = c.take<int>(d.n_utt + 1);
    u.active = c.take<int>(d.n_utt + 1);
    u.n_iter = c.take<int>(d.n_utt);
    u.err_init = c.take<double>(d.n_utt);
    u.err_prev = c.take<double>(d.n_utt);
    u.h0 = c.take<double>(d.n_utt);
    u.trace = c.take<double>((size_t)d.n_utt * n_slots);
    u.n_slots = n_slots;
    return u;
}

template <typename T>
Workspace<T> carve(void* base, const Dims& d, int algo, int n_slots, bool fused, const DictArrays<T>* ext = nullptr) {
    Workspace<T> w;
    Carver c{static_cast<char*>(base), 0};
    const bool gram = (algo == EVC_ALGO_GRAM || algo == EVC_ALGO_LITERAL);
    w.fused = fused;
    // the dictionary's arrays: from the prepared image, or from this workspace (then filled on every call)
    DictPlan plan{};
    plan.kl = true;
    plan.fused = fused;
    plan.packed_b = fused && d.Mb >= 1 && d.Mb <= 32;
    const DictArrays<T> da = ext ? *ext : take_dict<T>(c, d, plan);
    w.At = da.At;
    w.Am = da.Am;
    w.Akl = da.Akl;
    w.Xt = c.take<T>((size_t)d.Tp * d.Mk);
    w.Rt = fused ? nullptr : c.take<T>((size_t)d.Tp * d.Mk);
    w.packed_synth = fused && d.Mb >= 1 && d.Mb <= 32;
    // the fused path keeps the activations in the packed layout only; a frames-as-rows copy is
    // needed by the generic path, and by a synthesis that cannot run from the packed tiles
    const bool need_h0 = !fused || (d.Mb > 32);
    w.H0 = need_h0 ? c.take<T>((size_t)d.Tp * d.Np) : nullptr;
    w.Pt = fused ? nullptr : c.take<T>((size_t)d.Tp * d.Np);
    w.Vt = fused ? nullptr : c.take<T>((size_t)d.Tp * d.Mj);
    // slabs for the split-K form of V = H Am^T: its T x Mj output has few tiles (Mj is 64..576) against a long
    // contraction (N), so short batches need the split to fill the CUs
    const int vslabs = d.Tp <= 2048 ? 32 : (d.Tp <= 16384 ? 4 : (d.Tp <= 65536 ? 2 : 0));
    w.vsplit_elems = fused ? 0 : (size_t)vslabs * d.Tp * d.Mj;
    w.Vsplit = w.vsplit_elems ? c.take<T>(w.vsplit_elems) : nullptr;
    w.fl = FusedLayout{};
    w.fb = FusedBuffers{};
    if (fused) {
        w.fl = fused_layout(d.M, d.N, d.T_);
        w.fb.A1p = da.A1p;
        w.fb.A2p = da.A2p;
        w.fb.Xp = c.take<double>(w.fl.xp);
        w.fb.Hp = c.take<double>(w.fl.hp);
        w.fb.Vp = c.take<double>(w.fl.vp);
        static_assert(ALL_MAX_WGS >= COOP_MAX_TILES, "coop_buf is sized by k_fused_all's layout");
        w.fb.coop_buf = c.take<double>((size_t)(ALL_SLICE_OFFSET + ALL_SLICE_ELEMS));
        w.fb.coop_cnt = c.take<int>(COOP_MAX_TILES + 1);
        w.fb.rsum = da.rsum;
    }
    w.flB = FusedLayout{};
    w.Bt = nullptr; w.B1p = w.B2p = w.Yp = nullptr;
    if (w.packed_synth) {
        w.flB = fused_layout(d.Mb, d.N, d.T_);
        // (a prepared dictionary without B: these come from the workspace and are filled per call)
        w.Bt = da.Bt ? da.Bt : c.take<T>((size_t)d.Np * 32);
        w.B1p = da.B1p ? da.B1p : c.take<double>(w.flB.a1);
        w.B2p = da.B2p ? da.B2p : c.take<double>(w.flB.a2);
        w.Yp = c.take<double>(w.flB.vp);
    }
    w.H1 = gram ? c.take<T>((size_t)d.Tp * d.Np) : nullptr;
    w.G = gram ? c.take<T>((size_t)d.Np * d.Np) : nullptr;
    w.err2 = c.take<double>(d.Tp);
    w.u = take_utt(c, d, n_slots);
    w.bytes = w.bytes_min = (c.off + 255) & ~size_t(255);
    w.Yslab = nullptr;
    w.y_members = 0;
    if (w.packed_synth && w.flB.NT == w.fl.NT && w.fl.NT % 32 == 0 && w.fl.NT / 32 <= ALL_MAX_MEMBERS &&
        d.Mb <= 16 * w.fl.mtiles) {
        w.y_members = w.fl.NT / 32;
        w.Yslab = w.y_members == 1 ? w.Yp : c.take<double>((size_t)w.y_members * w.flB.vp);
        w.bytes = (c.off + 255) & ~size_t(255);
    }
    return w;
}

struct SynthArgs {          // optional Y = B H appended to a solve (evc_nmf_convert)
    const void* B; int ldb; void* Y; int ldy; int Mb;
    int b_rows;             // 1: B is exemplars-as-rows whatever the call's layout (a prepared dictionary's copy)
    int b_packed;           // 1: B's fragments are already in the dictionary image (nothing to import)
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
// staging of a float32 dictionary that rides the float64 fused kernels: A and B widened once
size_t dict_f64_staging(int M, int Mb, int N) {
    return ((((size_t)N * M + (size_t)N * Mb) * sizeof(double) + 512) + 255) & ~size_t(255);
}

// The image of a prepared dictionary (arithmetic type T) at `mem` (NULL: sizes only); `skip`: bytes of staging in front
// of it.  The size query, evc_dict_prepare and the solve drivers all read the image through this one description.
template <typename T> struct DictImage {
    Dims d;
    DictPlan plan;
    DictArrays<T> a;
    size_t bytes;
};
template <typename T> DictImage<T> dict_image(void* mem, size_t skip, int M, int Mb, int N, int loss) {
    DictImage<T> im;
    im.d = make_dims((int)sizeof(T), M, N, 1, 1, Mb);
    im.plan = dict_plan<T>(M, Mb, N, loss);
    Carver c{static_cast<char*>(mem), skip};
    im.a = take_dict<T>(c, im.d, im.plan);
    im.bytes = (c.off + 255) & ~size_t(255);
    return im;
}
template <typename T> DictArrays<T> dict_arrays(const evc_dict* dk, size_t skip) {
    return dict_image<T>(dk->mem, skip, dk->M, dk->Mb, dk->N, dk->loss).a;
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

// evc_solve_opts.reserved, decoded once per attempt (by plan_route)
struct SolveFlags {
    bool no_fused, exact_div, no_exchange, no_all_resident, pair_tiles;
    int c_req;           // bits 8..15: M <= 32: 1 | 2 = the general kernel; M > 32: exemplar ranges per frame group
    int w_req;           // bits 16..19: wavefronts per workgroup (k_fused_wide), whole bin tiles per wavefront (k_fused_wide64)
};
SolveFlags decode_flags(int reserved, int stop_rule) {
    SolveFlags f;
    f.no_fused = reserved & EVC_FLAG_NO_FUSED;
    // pymf's stop rule compares successive errors against 2.2e-16: it only fires at the reference's
    // iteration if the update reaches the same floating-point fixed point, i.e. with correctly rounded
    // quotients (EVC_FLAG_EXACT_DIV asks for them explicitly)
    f.exact_div = stop_rule == EVC_STOP_PYMF || (reserved & EVC_FLAG_EXACT_DIV);
    f.no_exchange = reserved & EVC_FLAG_NO_EXCHANGE;
    f.no_all_resident = reserved & EVC_FLAG_NO_ALL_RESIDENT;
    f.pair_tiles = reserved & EVC_FLAG_PAIR_TILES;
    f.c_req = (reserved >> 8) & 0xff;
    f.w_req = (reserved >> 16) & 0xf;
    return f;
}

// The route of one attempt of a solve: which driver runs it and, for M <= 32, which kernel.  plan_route (below use_wide)
// is the one place that decides it.
enum { ROUTE_GEMM, ROUTE_FUSED, ROUTE_WIDE };
struct Route {
    int family;          // ROUTE_GEMM: the two contractions; ROUTE_FUSED: float64 fused kernels (M <= 32); ROUTE_WIDE:
                         // k_fused_wide (float32) / k_fused_wide64 (float64)
    bool staged;         // ROUTE_FUSED for a float32 caller: through the staging copy (solve_f32_on_f64)
    int algo;            // EVC_ALGO_AUTO resolved
    int n_cus;
    SolveFlags flags;
    FusedRoute fused;    // ROUTE_FUSED only
};

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

// utterance bookkeeping of one attempt (a redo finds the offsets in place), then - once Xt is there - the start values
int utt_begin(const UttState& u, const int* utt_offsets, int n_utt, const Dims& d, int iters, bool redo, hipStream_t s) {
    if (!redo) {
        if (utt_offsets)
            HIP_TRY(hipMemcpyAsync(u.offsets, utt_offsets, sizeof(int) * (n_utt + 1), hipMemcpyHostToDevice, s));
        else
            HIP_TRY(utt_single(u, d.T_, s));
    }
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

// The fused persistent path (float64, M <= 32): one launch per `check_every` iterations (or a
// single launch when no residual is requested); V is carried between launches.
// H_out: the caller's H when the last launch may write it (NULL: not wanted, or to be exported behind the abort check);
// h_later: finish_fused will export H from the packed tiles whatever this function does; y: the synthesis that follows
// (NULL: none).  *exported / *y_done: the last launch delivered H / left the members' shares of Y in w.Yslab.
int solve_fused(const Workspace<double>& w, const Dims& d, const evc_solve_opts& o, const FusedRoute& r, int n_utt,
                hipStream_t s, double* H_out, int ldh, bool h_later, const SynthArgs* y, int* exported, int* y_done,
                evc_solve_info* inf) {
    *exported = 0;
    *y_done = 0;
    if (y && w.packed_synth) HIP_TRY(pack_synth_dict(w, d, o, *y, s));
    if (!o.dict) {     // (a prepared dictionary holds the fragments already)
        DictArrays<double> da{};
        da.At = w.At; da.Akl = w.Akl; da.A1p = w.fb.A1p; da.A2p = w.fb.A2p; da.rsum = w.fb.rsum;
        DictPlan pl{};
        pl.fused = true; pl.kl = o.loss == EVC_LOSS_KL;
        HIP_TRY(prepare_dict_fused(da, pl, nullptr, 0, d, true, false, s));
    }
    HIP_TRY(fused_pack_frames(w.fl, w.fb.Xp, w.Xt, d.Mk, s));
    FusedBuffers fb = w.fb;
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
        HIP_TRY(fused_iterate(w.fl, fb, r, w.u, d.N, d.T_, 0, 1, 1, w.err2, o.eps_mode, o.eps, o.l1, 1, o.loss, s));
        HIP_TRY(utt_check(w.err2, w.u, n_utt, 0, o.check_every, o.stop_rule, o.tol, s));
        first = 0;
    }
    if (o.ev_loop_start) HIP_TRY(hipEventRecord((hipEvent_t)o.ev_loop_start, s));
    int done = 0;
    while (done < o.iters) {
        int n = o.iters - done;
        bool check = false;
        if (o.check_every > 0 && n >= o.check_every) { n = o.check_every; check = true; }
        // the last launch of a solve in which nothing can stop writes the caller's H itself (k_fused_all)
        if (H_out && r.direct_export && done + n == o.iters) {
            fb.Hx = H_out; fb.ldhx = ldh; fb.hx_frame_major = o.layout == EVC_FRAME_MAJOR ? 1 : 0;
            *exported = 1;
        }
        // ... and on k_fused_all forms the members' shares of Y from the activations in its registers (round 9), when
        // B's bins fit the instance's row tiles and the workspace holds the slabs; the packed activations are then
        // stored only if somebody reads them afterwards (finish_fused: the export of H, the two-pass synthesis)
        if (r.kernel == EVC_KERNEL_FUSED_ALL && r.direct_export && done + n == o.iters) {
            if (y && w.packed_synth && w.Yslab && w.y_members == r.members) {
                fb.Yb2p = w.B2p; fb.Yslab = w.Yslab; fb.y_stride = (long)w.flB.vp; fb.y_mt = w.flB.mtiles;
                *y_done = 1;
            }
            fb.skip_hp = (!h_later && (!y || *y_done)) ? 1 : 0;
            // (reported for a synthesis formed here only: every other solve on this kernel keeps variant 0)
            inf->variant = *y_done ? (1 | (fb.skip_hp ? 0 : 2)) : 0;
        }
        HIP_TRY(hook.before_launch(s));
        ++inf->launches;
        HIP_TRY(fused_iterate(w.fl, fb, r, w.u, d.N, d.T_, n, first, check ? 1 : 0, w.err2, o.eps_mode, o.eps, o.l1,
                              o.stop_rule == EVC_STOP_NONE ? 1 : 0, o.loss, s));
        first = 0;
        done += n;
        if (check)
            HIP_TRY(utt_check(w.err2, w.u, n_utt, done / o.check_every, o.check_every, o.stop_rule,
                              o.tol, s));
    }
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord((hipEvent_t)o.ev_loop_stop, s));
    return ST_OK;
}

// tail of the fused path: H out of the packed tiles, Y from them
// (y_done: k_fused_all's last launch left the members' shares of Y in w.Yslab - they are summed; else the pre-pass over
// the packed activations with B's fragments, which solve_fused packed, forms Y)
int finish_fused(const Workspace<double>& w, const Dims& d, const evc_solve_opts& o, double* H, int ldh,
                 const SynthArgs* y, int y_done, int y_members, hipStream_t s) {
    const bool fm = (o.layout == EVC_FRAME_MAJOR);
    if (H) HIP_TRY(fused_export_h(w.fl, w.fb.Hp, H, ldh, fm ? 1 : 0, d.T_, d.N, s));
    if (!y) return ST_OK;
    if (y_done) {
        HIP_TRY(fused_unpack_y(w.flB, w.Yslab, y_members, (long)w.flB.vp, d.T_, y->Mb, static_cast<double*>(y->Y), y->ldy,
                               fm ? 1 : 0, s));
        return ST_OK;
    }
    if (w.packed_synth) {
        HIP_TRY(fused_synthesize(w.flB, w.B2p, w.fb.Hp, w.Yp, w.u, d.N, d.T_, y->Mb,
                                 static_cast<double*>(y->Y), y->ldy, fm ? 1 : 0, s));
        return ST_OK;
    }
    HIP_TRY(fused_export_h(w.fl, w.fb.Hp, w.H0, d.Np, 1, d.T_, d.N, s));
    return synth_rows<double>(w.H0, d.Np, *y, d.N, d.T_, fm, s);
}

// ------------------------------------------------------------------------------------------------------
// The wide fused path (float32, 32 < M <= 208, FACTORED): k_fused_wide (evc_wide.hip).  One launch per
// `check_every` iterations (a single launch when no residual is wanted); iteration 0 forms P and V = A H0.
// ------------------------------------------------------------------------------------------------------
template <typename T> struct WideKind;
template <> struct WideKind<float> {
    typedef WideLayout Layout;
    typedef WideBuffers Buffers;
    typedef WideCaps Caps;
    static constexpr int kernel = EVC_KERNEL_FUSED_WIDE;
    static Layout layout(int M, int N, int T_, int n_cus, int c_req, int w_req) {
        return wide_layout(M, N, T_, n_cus, c_req, w_req);
    }
    static Caps caps(int M, int N, int T_, int n_cus) { return wide_caps(M, N, T_, n_cus); }
    static float* image(const DictArrays<float>& a) { return a.Aw; }
};
template <> struct WideKind<double> {
    typedef Wide64Layout Layout;
    typedef Wide64Buffers Buffers;
    typedef Wide64Caps Caps;
    static constexpr int kernel = EVC_KERNEL_FUSED_WIDE64;
    static Layout layout(int M, int N, int T_, int n_cus, int c_req, int w_req) {
        return wide64_layout(M, N, T_, n_cus, c_req, w_req);
    }
    static Caps caps(int M, int N, int T_, int n_cus) { return wide64_caps(M, N, T_, n_cus); }
    static double* image(const DictArrays<double>& a) { return a.Aw64; }
};
template <typename T> struct WideWs {
    T *At, *Akl, *Xt, *H0;
    typename WideKind<T>::Buffers fb;
    typename WideKind<T>::Caps caps;
    double* err2;
    UttState u;
    size_t bytes;
};
int device_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
    return cus;
}
template <typename T>
WideWs<T> carve_wide(void* base, const Dims& d, int n_slots, int n_cus, bool with_synth, bool kl) {
    WideWs<T> w{};
    Carver c{static_cast<char*>(base), 0};
    w.caps = WideKind<T>::caps(d.M, d.N, d.T_, n_cus);
    w.At = c.take<T>((size_t)d.Np * d.Mk);
    w.Akl = kl ? c.take<T>((size_t)d.Np * d.Mk) : nullptr;
    w.Xt = c.take<T>((size_t)d.Tp * d.Mk);
    w.H0 = with_synth ? c.take<T>((size_t)d.Tp * d.Np) : nullptr;
    w.fb.Aw = c.take<T>(w.caps.aw);
    w.fb.Xw = c.take<T>(w.caps.xw);
    w.fb.Hw = c.take<T>(w.caps.hw);
    w.fb.Pw = c.take<T>(w.caps.hw);
    w.fb.Vpart = c.take<T>(w.caps.vpart);
    w.fb.Vsum = c.take<T>(w.caps.vsum);
    w.fb.ctl = c.take<unsigned>(w.caps.ctl);
    w.err2 = c.take<double>(d.Tp);
    w.u = take_utt(c, d, n_slots);
    if constexpr (sizeof(T) == 4) {
        // k_fused_wide, several stop checks per launch: up to 4 snapshots of the activations (5 checks per launch), as
        // many as fit in 2 GiB (a 16-utterance STFT batch: 180 MB each)
        const size_t one = w.caps.hw * sizeof(float);
        int slots = one ? (int)(((size_t)2 << 30) / one) : 0;
        slots = slots > 4 ? 4 : slots;
        w.fb.snap_slots = slots;
        w.fb.hs_stride = w.caps.hw;
        w.fb.err_stride = d.Tp;
        w.fb.Hs = slots ? c.take<float>((size_t)slots * w.caps.hw) : nullptr;
        w.fb.err2s = slots ? c.take<double>((size_t)slots * d.Tp) : nullptr;
    }
    w.bytes = (c.off + 255) & ~size_t(255);
    return w;
}
// Routing between the fused task-queue kernels and the two contractions, from the measured table
// profiles/r04_routing_table.md (tools/tune_routing.py on the final build: whole calls, K = 20 and K = 80, N in {1024, 4096,
// 16384}, 1 .. 64 utterances of 688 frames; fractions of the matrix peak, fused / two contractions at K = 80):
//  * float32 (k_fused_wide, 32 < M <= 208): ahead from one utterance on at every N and M measured (M = 201: 0.52 / 0.42 at
//    N = 16384, 0.34 / 0.29 at 4096, 0.16 / 0.13 at 1024), and by more and more towards 64 utterances (M = 201, N = 4096:
//    0.71 / 0.53).
//  * float64 (k_fused_wide64, 144 < M <= 528): small dictionaries (N = 1024) from one utterance on (M = 513: 0.26 / 0.22,
//    three utterances 0.47 / 0.35) up to ~32 (64: 0.64 / 0.69).  N >= 2048: two utterances lose (M = 513, N = 4096:
//    0.50 / 0.61 - five ranges with reduce slices against the contractions' best case), three win (0.60 / 0.53: 260 tasks
//    through the queue) and so do four to ~24 (16: 0.66 / 0.62; 32: 0.67 / 0.67; 64: 0.67 / 0.71).  At M = 257 (4 bin tiles
//    per wavefront: fewer MFMAs per block against the same fixed work) the window closes earlier: 2048 <= N < 8192 up to
//    ~14 utterances (16: 0.55 / 0.55), from N = 8192 on the two contractions win or tie throughout (six utterances at
//    N = 16384: 0.55 / 0.59).  176 < M <= 208 (3 bin tiles per wavefront, 0.49 - 0.52): N < 8192 like the others up to ~45
//    utterances (32: 0.51 / 0.49, 64: 0.51 / 0.58), from 8192 on only where the contractions' tile counts fall badly
//    (12 - 32 utterances: 0.51 - 0.52 / 0.40 - 0.47); M <= 176 pads more than a thirteenth of the tile slots and stays out
//    (M = 160: 0.42).
// The tuning bits (ranges, wavefronts / bin tiles) force the fused kernel at any size.
bool use_wide(int M, int N, int T_, int dtype, int algo, int loss, const SolveFlags& f) {
    if (f.no_fused) return false;
    // the task queues hand partial sums from workgroup to workgroup inside a launch and the call reads one word back at
    // the end (a wait that ran out): exactly what EVC_FLAG_NO_EXCHANGE rules out
    if (f.no_exchange) return false;
    const bool forced = f.c_req != 0 || f.w_req != 0;
    const int tiles = (T_ + 15) / 16;
    if (dtype == EVC_F64) {
        if (!wide64_supported(M, N, T_, dtype, algo, loss)) return false;
        if (forced) return true;
        const int lo64 = N < 2048 ? 43 : 100;
        if (M <= 208) {
            if (M <= 176) return false;
            return tiles >= (N < 8192 ? lo64 : 500) && tiles <= 2000;
        }
        const int hi = N < 2048 ? 1400 : (M >= 400 ? 1000 : (N < 8192 ? 600 : 0));
        return tiles >= lo64 && tiles <= hi;
    }
    if (!wide_supported(M, N, T_, dtype, algo)) return false;
    if (forced) return true;
    // (with tagged hand-offs on the static schedule - the last change of round 4 - the fused kernel is ahead from one
    // utterance of 688 frames on at every (M, N) measured: M = 201, N = 4096: 0.34 / 0.29 at one, 0.49 / 0.34 at two;
    // N = 1024: 0.16 / 0.13; M = 64, N = 4096: 0.21 / 0.15.  Shorter inputs were not measured and stay where they were.)
    return tiles >= 43;
}

// The one place a route is decided (and a new one added): pure host arithmetic on the call's sizes and options.
// The families are disjoint in M (fused: M <= 32; k_fused_wide: 32 < M <= 208, float32; k_fused_wide64: 144 < M <= 528,
// float64), so the order of the questions does not matter.
Route plan_route(int M, int N, int T_, int dtype, const evc_solve_opts& o, int n_cus) {
    Route r{};
    r.algo = algo_eff(o.algo);
    r.n_cus = n_cus;
    const SolveFlags& f = r.flags = decode_flags(o.reserved, o.stop_rule);
    r.family = ROUTE_GEMM;
    if (!f.no_fused && small_family(M, N, T_, r.algo)) r.family = ROUTE_FUSED;
    else if (use_wide(M, N, T_, dtype, r.algo, o.loss, f)) r.family = ROUTE_WIDE;
    if (r.family != ROUTE_FUSED) return r;
    r.staged = dtype == EVC_F32;
    FusedRoute& k = r.fused;
    k.kernel = EVC_KERNEL_FUSED_MU;
    k.members = 1;
    k.c_req = f.c_req;
    k.exact_div = f.exact_div ? 1 : 0;
    k.n_cus = n_cus;
    const FusedLayout fl = fused_layout(M, N, T_);
    // every activation and numerator tile register-resident, NT / 32 workgroups per frame tile (k_fused_all);
    // EVC_FLAG_NO_ALL_RESIDENT switches that kernel off, EVC_FLAG_NO_EXCHANGE every form of inter-workgroup exchange
    if (f.c_req == 0 && !f.no_all_resident) {
        const int c = fused_all_members(fl.NT, N, o.eps_mode, k.exact_div, o.loss);
        if (c == 1 || (c > 1 && c <= n_cus && !f.no_exchange)) { k.kernel = EVC_KERNEL_FUSED_ALL; k.members = c; }
        // two frame tiles per member, exchange inside the sweeps (k_fused_xy, round 4): measured slower than k_fused_all
        // (profiles/r04_xy_notes.md), so only on request - EVC_FLAG_PAIR_TILES
        const int cx = fused_xy_members(fl.NT, N, o.eps_mode, k.exact_div, o.loss);
        if (cx >= 2 && cx <= 2 * n_cus && !f.no_exchange && f.pair_tiles) { k.kernel = EVC_KERNEL_FUSED_XY; k.members = cx; }
    }
    if (f.c_req == 0 && k.kernel == EVC_KERNEL_FUSED_MU && fused_res_supported(N, o.eps_mode, k.exact_div)) {
        k.kernel = EVC_KERNEL_FUSED_RES;
        // few frame tiles (one or two utterances): several workgroups share a tile and split the exemplars
        // (k_fused_res COOP); EVC_FLAG_NO_EXCHANGE switches it off
        if (!f.no_exchange) k.members = fused_res_coop_factor(fl.NT, fl.TT, n_cus);
    }
    const bool all_res = k.kernel == EVC_KERNEL_FUSED_ALL || k.kernel == EVC_KERNEL_FUSED_XY;
    // constant start values: the first launch on k_fused_all forms them itself when no residual is wanted at init
    k.init_const = o.init_mode != EVC_INIT_GIVEN && all_res && o.iters > 0 &&
                   !(o.check_every > 0 && o.stop_rule == EVC_STOP_SKLEARN);
    k.direct_export = all_res && o.stop_rule == EVC_STOP_NONE;
    return r;
}

template <typename T>
int solve_wide(const void* A_, int lda, const void* X_, int ldx, void* H_, int ldh, int M, int N, int T_,
               const int* utt_offsets, int n_utt, const evc_solve_opts& o, const Route& r, void* ws, size_t ws_bytes,
               int* n_iter_out, double* err_out, const SynthArgs* y, hipStream_t s, evc_solve_info* inf) {
    typedef WideKind<T> K;
    const T* A = static_cast<const T*>(A_);
    const T* X = static_cast<const T*>(X_);
    T* H = static_cast<T*>(H_);
    const Dims d = make_dims((int)sizeof(T), M, N, T_, n_utt, y ? y->Mb : 0);
    const int n_slots = n_slots_for(o.iters, o.check_every);
    if (n_slots > MAX_SLOTS) return ST_UNSUPPORTED;
    const int n_cus = r.n_cus;
    const bool kl = o.loss == EVC_LOSS_KL, fm = o.layout == EVC_FRAME_MAJOR;
    WideWs<T> w = carve_wide<T>(ws, d, MAX_SLOTS, n_cus, true, sizeof(T) == 4);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    w.u.n_slots = n_slots;
    // tuning / tests: exemplar ranges per frame group, wavefronts per workgroup
    const typename K::Layout fl = K::layout(M, N, T_, n_cus, r.flags.c_req, r.flags.w_req);
    // (a prepared dictionary holds the block images of the DEFAULT layout: a tuning override of the wavefront / tile
    // count does not fit it - unsupported, not a workspace problem)
    if (!wide_fits(fl, w.caps)) return (o.dict && r.flags.w_req) ? ST_UNSUPPORTED : ST_WORKSPACE;

    HIP_TRY(utt_begin(w.u, utt_offsets, n_utt, d, o.iters, false, s));
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
        HIP_TRY(copy2d<T>(A, lda, N, M, fm ? 0 : 1, w.At, d.Mk, d.Np, d.Mk, 0, s));
        if (kl) HIP_TRY(kl_scale_dict<T>(w.At, d.Mk, M, d.Np, o.eps, w.Akl, s));
        HIP_TRY(wide_pack_dict(fl, kl ? w.Akl : w.At, w.At, d.Mk, d.Np, w.fb.Aw, s));
    }
    HIP_TRY(copy2d<T>(X, ldx, T_, M, fm ? 0 : 1, w.Xt, d.Mk, d.Tp, d.Mk, 0, s));
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
    return copy_back(w.u, n_utt, n_slots, n_iter_out, err_out, s);
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

template <typename T>
int solve_typed(const void* A_, int lda, const void* X_, int ldx, void* H_, int ldh, int M, int N,
                int T_, const int* utt_offsets, int n_utt, const evc_solve_opts& o, const Route& r, void* ws,
                size_t ws_bytes, int* n_iter_out, double* err_out, const SynthArgs* y, hipStream_t s,
                evc_solve_info* inf) {
    const T* A = static_cast<const T*>(A_);
    const T* X = static_cast<const T*>(X_);
    T* H = static_cast<T*>(H_);
    const Dims d = make_dims((int)sizeof(T), M, N, T_, n_utt, y ? y->Mb : 0);
    const int algo = r.algo;
    const int n_slots = n_slots_for(o.iters, o.check_every);
    if (n_slots > MAX_SLOTS) return ST_UNSUPPORTED;
    const bool fused = r.family == ROUTE_FUSED;
    // dictionary arrays: from the prepared image (float32 callers riding the float64 kernels: behind its staging)
    DictArrays<T> ext{};
    if (o.dict) ext = dict_arrays<T>(o.dict, (sizeof(T) == 8 && o.dict->dtype == EVC_F32) ? dict_f64_staging(M, o.dict->Mb, N) : 0);
    Workspace<T> w = carve<T>(ws, d, algo, MAX_SLOTS, fused, o.dict ? &ext : nullptr);
    if (w.bytes_min > ws_bytes) return ST_WORKSPACE;
    if (w.bytes > ws_bytes) w.Yslab = nullptr;      // no room for the members' shares of Y: the two-pass synthesis
    inf->prepared = o.dict ? 1 : 0;
    SynthArgs ydict;              // synthesis from the prepared copy of B
    if (o.dict && y && o.dict->Mb > 0) {
        ydict = *y;
        ydict.B = ext.Bc; ydict.ldb = o.dict->Mb; ydict.b_rows = 1; ydict.b_packed = ext.B2p ? 1 : 0;
        y = &ydict;
    }
    w.u.n_slots = n_slots;
    const bool fm = (o.layout == EVC_FRAME_MAJOR);

    HIP_TRY(utt_begin(w.u, utt_offsets, n_utt, d, o.iters, false, s));

    // ---- import the caller's matrices into zero-padded frames-as-rows workspace arrays ----
    // At[n][m], Am[m][n], Xt[t][m], Ht[t][n]
    const bool kl = (o.loss == EVC_LOSS_KL);
    if (!o.dict) {
        DictArrays<T> da{};
        da.At = w.At; da.Am = w.Am; da.Akl = w.Akl;
        HIP_TRY(prepare_dict<T>(da, kl, A, lda, d, fm, o.eps, s));
    }
    HIP_TRY(copy2d<T>(X, ldx, T_, M, fm ? 0 : 1, w.Xt, d.Mk, d.Tp, d.Mk, 0, s));
    HIP_TRY(utt_start_values<T>(w.u, w.Xt, n_utt, d, o, s));

    if constexpr (sizeof(T) == 8) if (fused) {     // activations live in the packed tile layout from start to finish
        evc_solve_opts oo = o;
        FusedRoute fr = r.fused;
        // A cooperative launch that gave up waiting for a peer workgroup (another process or stream held the
        // CUs it needed) leaves void results, and the solve is redone with one workgroup per frame tile.  The
        // flag costs a host round trip: when the start values can be regenerated it is read after the results
        // have been exported (they are exported again by the redo); with caller-given start values it is read
        // before anything is written to the caller's H.
        const bool check_first = (o.init_mode == EVC_INIT_GIVEN);
        for (int attempt = 0; attempt < 2; ++attempt) {
            if (o.init_mode == EVC_INIT_GIVEN)
                HIP_TRY(fused_import_h(w.fl, w.fb.Hp, H, ldh, fm ? 1 : 0, T_, N, s));
            const bool coop_used = fr.members > 1;
            const int* abort_w = w.fb.coop_cnt + COOP_MAX_TILES;
            int aborted = 0, exported = 0, y_done = 0;        // (constant start values: solve_fused)
            // (with caller-given start values the abort flag is read before anything goes to the caller's H: no
            // direct export then)
            inf->variant = 0;
            HIP_TRY(solve_fused(w, d, oo, fr, n_utt, s, check_first ? nullptr : H, ldh, check_first && H, y, &exported,
                                &y_done, inf));
            if (coop_used && check_first) HIP_TRY(read_abort(abort_w, s, &aborted));
            if (!aborted) {
                HIP_TRY(finish_fused(w, d, o, exported ? nullptr : H, ldh, y, y_done, fr.members, s));
                if (coop_used && !check_first) HIP_TRY(read_abort(abort_w, s, &aborted));
            }
            if (!aborted) break;
            if (attempt == 1) return ST_COOP_TIMEOUT;      // cannot happen: the redo is not cooperative
            oo.reserved |= EVC_FLAG_NO_EXCHANGE;
            oo.test_abort_at = 0;
            fr = plan_route(M, N, T_, EVC_F64, oo, r.n_cus).fused;
            inf->redo = 1;
            HIP_TRY(utt_begin(w.u, utt_offsets, n_utt, d, o.iters, true, s));
            HIP_TRY(utt_start_values<T>(w.u, w.Xt, n_utt, d, o, s));
        }
        return copy_back(w.u, n_utt, n_slots, n_iter_out, err_out, s);
    }

    if (o.init_mode == EVC_INIT_GIVEN)
        HIP_TRY(copy2d<T>(H, ldh, T_, N, fm ? 0 : 1, w.H0, d.Np, d.Tp, d.Np, 0, s));
    else
        HIP_TRY(fill_h0<T>(w.H0, d.Np, d.Tp, N, T_, w.u, s));

    // ---- numerator (and Gram matrix) ----
    const bool gram = (algo == EVC_ALGO_GRAM || algo == EVC_ALGO_LITERAL);
    if (gram) HIP_TRY(gemm_nt<T>(w.At, d.Mk, w.At, d.Mk, w.G, d.Np, d.Np, d.Np, d.Mk, s));
    if (!kl) HIP_TRY(gemm_nt<T>(w.Xt, d.Mk, w.At, d.Mk, w.Pt, d.Np, d.Tp, d.Np, d.Mk, s));

    T* Hc = w.H0;       // current activations
    T* Hn = w.H1;       // ping-pong partner (GRAM only)
    bool v_valid = false;

    auto residual_check = [&](int c) -> int {
        if (!v_valid) HIP_TRY(gemm_nt<T>(Hc, d.Np, w.Am, d.Np, w.Vt, d.Mj, d.Tp, d.Mj, d.Np, s, w.Vsplit, w.vsplit_elems, nullptr, d.Mk));
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
            HIP_TRY(gemm_nt_mu<T>(Hc, d.Np, w.G, d.Np, Hn, d.Tp, d.Np, d.Np, ep, s));
            T* tmp = Hc; Hc = Hn; Hn = tmp;
        } else {
            if (!v_valid) HIP_TRY(gemm_nt<T>(Hc, d.Np, w.Am, d.Np, w.Vt, d.Mj, d.Tp, d.Mj, d.Np, s, w.Vsplit, w.vsplit_elems, nullptr, d.Mk, gate));
            ep.Hin = Hc;
            if (kl) {                     // H' = H (.) (X (/) max(V, eps)) (A / colsum)   sklearn _nmf.py:556-606
                HIP_TRY(kl_ratio<T>(w.Xt, d.Mk, w.Vt, d.Mj, M, d.Tp, o.eps, w.Rt, d.Mk, s));
                HIP_TRY(gemm_nt_mu<T>(w.Rt, d.Mk, w.Akl, d.Mk, Hc, d.Tp, d.Np, d.Mk, ep, s));
            } else {                      // H' = mu(H, P, V At^T), V = H Am^T ; in place
                HIP_TRY(gemm_nt_mu<T>(w.Vt, d.Mj, w.At, d.Mk, Hc, d.Tp, d.Np, d.Mk, ep, s));
            }
        }
        v_valid = false;
        if (o.check_every > 0 && it % o.check_every == 0) HIP_TRY(residual_check(it / o.check_every));
    }

    if (o.ev_loop_stop) HIP_TRY(hipEventRecord((hipEvent_t)o.ev_loop_stop, s));
    if (H) HIP_TRY(copy2d<T>(Hc, d.Np, d.T_, d.N, 0, H, ldh, d.T_, d.N, fm ? 0 : 1, s));
    if (y) HIP_TRY(synth_rows<T>(Hc, d.Np, *y, d.N, d.T_, fm, s));
    return copy_back(w.u, n_utt, n_slots, n_iter_out, err_out, s);
}

// callers may disable the fused kernels per call, so the query covers the carving of every route the sizes allow
template <typename T> size_t workspace_typed(int M, int Mb, int N, int T_, int n_utt, int algo) {
    const Dims d = make_dims((int)sizeof(T), M, N, T_, n_utt, Mb);
    const int al = algo_eff(algo);
    const int dt = sizeof(T) == 8 ? EVC_F64 : EVC_F32;
    size_t b = carve<T>(nullptr, d, al, MAX_SLOTS, false).bytes;
    if (dt == EVC_F64 && small_family(M, N, T_, al))
        b = std::max(b, carve<T>(nullptr, d, al, MAX_SLOTS, true).bytes);
    if (wide_family(M, N, T_, dt, al, EVC_LOSS_FROBENIUS))
        b = std::max(b, carve_wide<T>(nullptr, d, MAX_SLOTS, device_cus(), true, sizeof(T) == 4).bytes);
    return b;
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

// float32 callers with a small bin count: the float64 fused kernels are 2.5x faster than the float32
// generic path (and exact to float32 rounding), so their matrices are widened into a staging region, solved by
// the float64 route and narrowed on the way out.  The reference's float32 surface (nmf_tool, TF1) is compared
// against a float64 restatement anyway: computing in float64 only moves the result towards it.
static size_t f32_staging_bytes(int M, int Mb, int N, int T) {
    const size_t n = (size_t)N * M + (size_t)T * M + (size_t)T * N + (size_t)N * Mb + (size_t)T * Mb;
    return ((n * sizeof(double) + 6 * 256) + 255) & ~size_t(255);   // the inner workspace starts 256-byte aligned
}

size_t evc_workspace_bytes(int M, int Mb, int N, int T, int n_utt, int dtype, int algo) {
    if (M < 0 || Mb < 0 || N < 0 || T < 0 || n_utt < 1) return 0;
    if (algo < EVC_ALGO_GRAM || algo > EVC_ALGO_AUTO) return 0;
    if (dtype == EVC_F64) return workspace_typed<double>(M, Mb, N, T, n_utt, algo);
    if (dtype != EVC_F32) return 0;
    size_t b = workspace_typed<float>(M, Mb, N, T, n_utt, algo);
    if (small_family(M, N, T, algo_eff(algo)))
        b = std::max(b, f32_staging_bytes(M, Mb, N, T) + workspace_typed<double>(M, Mb, N, T, n_utt, algo));
    return b;
}

static int solve_f32_on_f64(const void* A, int lda, const void* X, int ldx, void* H, int ldh, int M, int N, int T,
                            const int* utt_offsets, int n_utt, const evc_solve_opts& o, const Route& r, void* ws,
                            size_t ws_bytes, int* n_iter_out, double* err_out, const SynthArgs* y, hipStream_t s,
                            evc_solve_info* inf) {
    const bool fm = (o.layout == EVC_FRAME_MAJOR);
    const int Mb = y ? y->Mb : 0;
    const size_t stage = f32_staging_bytes(M, Mb, N, T);
    if (ws_bytes < stage) return ST_WORKSPACE;
    // staged matrices keep the caller's orientation with compact rows: (outer, inner) per layout
    const long aR = fm ? N : M, aC = fm ? M : N, xR = fm ? T : M, xC = fm ? M : T, hR = fm ? T : N, hC = fm ? N : T;
    const long bR = fm ? N : Mb, bC = fm ? Mb : N, yR = fm ? T : Mb, yC = fm ? Mb : T;
    Carver c{static_cast<char*>(ws), 0};
    double* A64 = c.take<double>((size_t)N * M);
    double* X64 = c.take<double>((size_t)T * M);
    double* H64 = c.take<double>((size_t)T * N);
    double* B64 = c.take<double>((size_t)N * Mb);
    double* Y64 = c.take<double>((size_t)T * Mb);
    if (!o.dict) HIP_TRY((cvt2d<float, double>(static_cast<const float*>(A), lda, aR, aC, A64, aC, s)));
    HIP_TRY((cvt2d<float, double>(static_cast<const float*>(X), ldx, xR, xC, X64, xC, s)));
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
    HIP_TRY(solve_typed<double>(A64, (int)aC, X64, (int)xC, H ? H64 : nullptr, (int)hC, M, N, T, utt_offsets, n_utt, o64, r,
                                static_cast<char*>(ws) + stage, ws_bytes - stage, n_iter_out, err_out, y ? &y64 : nullptr,
                                s, inf));
    if (H) HIP_TRY((cvt2d<double, float>(H64, hC, hR, hC, static_cast<float*>(H), ldh, s)));
    if (y) HIP_TRY((cvt2d<double, float>(Y64, yC, yR, yC, static_cast<float*>(y->Y), y->ldy, s)));
    if (n_iter_out || err_out) HIP_TRY(hipStreamSynchronize(s));    // those calls are synchronous: so are H and Y
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

static int solve_checked(const void* A, int lda, const void* X, int ldx, void* H, int ldh, int M, int N,
                        int T, const int* utt_offsets, int n_utt, const evc_solve_opts* opts,
                        void* workspace, size_t workspace_bytes, int* n_iter_out, double* err_out,
                        const SynthArgs* y, evc_stream_t stream) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_solve_opts)) return ST_BADARG;
    const evc_solve_opts& o = *opts;
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
        if (n_iter_out) for (int i = 0; i < n_utt; ++i) n_iter_out[i] = 0;
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
    if ((!dk && !A) || !X || !workspace) return ST_BADARG;
    if (!H && (!y || o.init_mode == EVC_INIT_GIVEN)) return ST_BADARG;   // H may be omitted by evc_nmf_convert only
    if ((!dk && bad_ld(o.layout, lda, N, M)) || bad_ld(o.layout, ldx, T, M) || (H && bad_ld(o.layout, ldh, T, N)))
        return ST_BADARG;
    if (y && (!y->Y || bad_ld(o.layout, y->ldy, T, y->Mb))) return ST_BADARG;
    if (y && !(dk && dk->Mb > 0) && (!y->B || bad_ld(o.layout, y->ldb, N, y->Mb))) return ST_BADARG;
    if (!utt_offsets_ok(utt_offsets, n_utt, T)) return ST_BADARG;
    // tuning bits 16..19: wavefronts per workgroup of k_fused_wide (4 | 8), whole bin tiles per wavefront of
    // k_fused_wide64 (4 | 5 | 7 | 8: the narrowest instance >= the request that holds M); anything else is an error
    const int tw = route.flags.w_req;
    if (M > 32 && tw != 0 && !(o.dtype == EVC_F32 ? (tw == 4 || tw == 8) : (tw == 3 || tw == 4 || tw == 5 || tw == 7 || tw == 8)))
        return ST_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    evc_solve_info inf{};
    // three drivers, one signature: the task queues, float32 staged onto the float64 fused kernels, fused / two contractions
    auto run = [&](const Route& r, const evc_solve_opts& oo) -> int {
        const bool f64 = o.dtype == EVC_F64;
        auto driver = f64 ? solve_typed<double> : solve_typed<float>;
        switch (r.family) {
            case ROUTE_WIDE: driver = f64 ? solve_wide<double> : solve_wide<float>; break;
            case ROUTE_FUSED: if (r.staged) driver = solve_f32_on_f64; break;
            default: break;
        }
        return driver(A, lda, X, ldx, H, ldh, M, N, T, utt_offsets, n_utt, oo, r, workspace, workspace_bytes, n_iter_out,
                      err_out, y, s, &inf);
    };
    int st = run(route, o);
    if (st == ST_COOP_TIMEOUT && route.family == ROUTE_WIDE) {
        // a task-queue solve whose bounded wait ran out is redone on the two contractions (nothing has reached H or Y)
        evc_solve_opts redo_o = o;
        redo_o.reserved |= EVC_FLAG_NO_FUSED;
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
    return solve_checked(A, lda, X, ldx, H, ldh, M, N, T, utt_offsets, n_utt, opts, workspace,
                         workspace_bytes, n_iter_out, err_out, nullptr, stream);
}

int evc_nmf_convert(const void* A, int lda, const void* X, int ldx, const void* B, int ldb, void* H,
                    int ldh, void* Y, int ldy, int M, int Mb, int N, int T, const int* utt_offsets,
                    int n_utt, const evc_solve_opts* opts, void* workspace, size_t workspace_bytes,
                    int* n_iter_out, double* err_out, evc_stream_t stream) {
    const SynthArgs y{B, ldb, Y, ldy, Mb};
    return solve_checked(A, lda, X, ldx, H, ldh, M, N, T, utt_offsets, n_utt, opts, workspace,
                         workspace_bytes, n_iter_out, err_out, &y, stream);
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

size_t evc_griffin_lim_workspace_bytes(int T, int fft_size, int hop, int iters) {
    if (T < 1 || fft_size < 2 || (fft_size & 1) || hop < 1 || iters < 0) return 0;
    return gl_workspace_bytes(T, 1, fft_size, hop, iters);
}

int evc_griffin_lim(const void* mag, int ldm, int T, int fft_size, int hop, int iters, void* x,
                    void* workspace, size_t workspace_bytes, double* rmse_out, evc_stream_t stream) {
    if (T < 0) return ST_BADARG;
    const int off[2] = {0, T};
    return evc_griffin_lim_batch(mag, ldm, off, 1, fft_size, hop, iters, x, workspace, workspace_bytes, rmse_out,
                                 stream);
}

static bool gl_offsets_ok(const int* off, int n_utt) {
    if (!off || n_utt < 1 || off[0] != 0) return false;
    for (int u = 0; u < n_utt; ++u)
        if (off[u + 1] < off[u]) return false;
    return true;
}

size_t evc_griffin_lim_batch_workspace_bytes(const int* frame_offsets, int n_utt, int fft_size, int hop, int iters) {
    if (!gl_offsets_ok(frame_offsets, n_utt) || frame_offsets[n_utt] < 1 || fft_size < 2 || (fft_size & 1) ||
        hop < 1 || iters < 0)
        return 0;
    return gl_workspace_bytes(frame_offsets[n_utt], n_utt, fft_size, hop, iters);
}

int evc_griffin_lim_batch(const void* mag, int ldm, const int* frame_offsets, int n_utt, int fft_size, int hop,
                          int iters, void* x, void* workspace, size_t workspace_bytes, double* rmse_out,
                          evc_stream_t stream) {
    if (!gl_offsets_ok(frame_offsets, n_utt) || fft_size < 2 || (fft_size & 1) || hop < 1 || iters < 0)
        return ST_BADARG;
    if (frame_offsets[n_utt] == 0) return ST_OK;
    if (!mag || !x || !workspace || ldm < fft_size / 2 + 1) return ST_BADARG;
    const size_t need = gl_workspace_bytes(frame_offsets[n_utt], n_utt, fft_size, hop, iters);
    if (need == 0) return ST_BADARG;
    if (workspace_bytes < need) return ST_WORKSPACE;
    return (int)gl_run(static_cast<const double*>(mag), ldm, frame_offsets, n_utt, fft_size, hop, iters,
                       static_cast<double*>(x), workspace, rmse_out, reinterpret_cast<hipStream_t>(stream));
}

int evc_stft_frames(long n_samples, int fft_size, int hop, int center) {
    if (n_samples < 1 || fft_size < 2 || (fft_size & 1) || hop < 1) return 0;
    return stft_frames(n_samples, hop, center != 0, fft_size);
}

size_t evc_stft_workspace_bytes(long n_samples, int fft_size, int hop, int center) {
    if (n_samples < 1 || fft_size < 2 || (fft_size & 1) || hop < 1) return 0;
    return stft_workspace_bytes(n_samples, fft_size, hop, center != 0);
}

int evc_stft(const void* x, long n_samples, int fft_size, int hop, int center, void* re, int ldre, void* im,
             int ldim, void* workspace, size_t workspace_bytes, evc_stream_t stream) {
    if (n_samples < 0 || fft_size < 2 || (fft_size & 1) || hop < 1) return ST_BADARG;
    if (n_samples > (1L << 31) - 4096) return ST_BADARG;        // frame counts are ints
    if (n_samples == 0 || stft_frames(n_samples, hop, center != 0, fft_size) == 0) return ST_OK;
    const int nb = fft_size / 2 + 1;
    if (!x || !re || !im || !workspace || ldre < nb || ldim < nb) return ST_BADARG;
    if (workspace_bytes < stft_workspace_bytes(n_samples, fft_size, hop, center != 0)) return ST_WORKSPACE;
    return (int)stft_run(static_cast<const double*>(x), n_samples, fft_size, hop, center != 0,
                         static_cast<double*>(re), ldre, static_cast<double*>(im), ldim, workspace,
                         reinterpret_cast<hipStream_t>(stream));
}

// 0, or the status the options / offsets of an evc_mfcc call earn before anything else is looked at
static int mfcc_check(const long* soff, int n_utt, const evc_mfcc_opts* o) {
    if (!o || o->struct_bytes != (int)sizeof(evc_mfcc_opts) || n_utt < 0) return ST_BADARG;
    if (o->sr < 1 || o->fft_size < 2 || (o->fft_size & 1) || o->hop < 1 || o->n_mels < 1) return ST_BADARG;
    if (o->n_mfcc < 1 || o->n_mfcc > o->n_mels) return ST_BADARG;
    const double fmax_ = o->fmax == 0.0 ? 0.5 * o->sr : o->fmax;
    if (!(o->fmin >= 0.0 && o->fmin < fmax_ && fmax_ <= 0.5 * o->sr) || !(o->amin > 0.0) || o->top_db != o->top_db)
        return ST_BADARG;
    if (n_utt > 0) {
        if (!soff || soff[0] < 0) return ST_BADARG;
        for (int u = 0; u < n_utt; ++u)
            if (soff[u + 1] < soff[u]) return ST_BADARG;
    }
    if (o->n_mels > EVC_MFCC_MAX_MELS || o->fft_size > EVC_MFCC_MAX_FFT) return ST_UNSUPPORTED;
    return ST_OK;
}

size_t evc_mfcc_workspace_bytes(const long* sample_offsets, int n_utt, const evc_mfcc_opts* opts) {
    if (mfcc_check(sample_offsets, n_utt, opts) != ST_OK || n_utt < 1) return 0;
    return mfcc_workspace_bytes(sample_offsets, n_utt, *opts);
}

int evc_mfcc(const void* x, const long* sample_offsets, int n_utt, const evc_mfcc_opts* opts, void* mfcc, int ldc,
             void* re, int ldre, void* im, int ldim, void* workspace, size_t workspace_bytes, evc_stream_t stream) {
    const int st = mfcc_check(sample_offsets, n_utt, opts);
    if (st != ST_OK) return st;
    const int nb = opts->fft_size / 2 + 1;
    if (ldc < opts->n_mfcc || (re && ldre < nb) || (im && ldim < nb)) return ST_BADARG;
    if (n_utt == 0 || !mfcc_has_frames(sample_offsets, n_utt, *opts)) return ST_OK;
    if (!x || !mfcc || !workspace) return ST_BADARG;
    const size_t need = mfcc_workspace_bytes(sample_offsets, n_utt, *opts);
    if (need == 0) return ST_BADARG;                            // more rows than the int indices hold
    if (workspace_bytes < need) return ST_WORKSPACE;
    return (int)mfcc_run(static_cast<const double*>(x), sample_offsets, n_utt, *opts, static_cast<double*>(mfcc), ldc,
                         static_cast<double*>(re), ldre, static_cast<double*>(im), ldim, workspace,
                         reinterpret_cast<hipStream_t>(stream));
}

static bool dtw_offsets_ok(const int* off, int n_pairs) {
    if (!off || off[0] != 0) return false;
    for (int p = 0; p < n_pairs; ++p)
        if (off[p + 1] < off[p] || off[p + 1] - off[p] > dtw_max_frames()) return false;
    return true;
}

size_t evc_dtw_workspace_bytes(const int* a_offsets, const int* b_offsets, int n_pairs) {
    if (n_pairs < 1 || !dtw_offsets_ok(a_offsets, n_pairs) || !dtw_offsets_ok(b_offsets, n_pairs)) return 0;
    return dtw_workspace_bytes(a_offsets, b_offsets, n_pairs);
}

int evc_dtw_align(const void* A, int lda, const int* a_offsets, const void* B, int ldb,
                  const int* b_offsets, int D, int n_pairs, int* path_a, int* path_b, int* path_len,
                  double* total, void* workspace, size_t workspace_bytes, evc_stream_t stream) {
    if (n_pairs < 1 || D < 1 || lda < D || ldb < D) return ST_BADARG;
    if (D > 512 || n_pairs > 65535) return ST_UNSUPPORTED;     // LDS tile of the cost kernel; grid z
    if (!dtw_offsets_ok(a_offsets, n_pairs) || !dtw_offsets_ok(b_offsets, n_pairs)) return ST_BADARG;
    if (!A || !B || !path_a || !path_b || !path_len || !workspace) return ST_BADARG;
    if (workspace_bytes < dtw_workspace_bytes(a_offsets, b_offsets, n_pairs)) return ST_WORKSPACE;
    return (int)dtw_run(static_cast<const double*>(A), lda, a_offsets, static_cast<const double*>(B), ldb,
                        b_offsets, D, n_pairs, path_a, path_b, path_len, total, workspace,
                        reinterpret_cast<hipStream_t>(stream));
}


int evc_dtw_path_rows(const int* path_len, int n_pairs, int* row_start, int* n_rows_out, evc_stream_t stream) {
    if (!path_len || !row_start || n_pairs < 1 || n_pairs > 65535) return ST_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(dtw_path_scan(path_len, n_pairs, row_start, s));
    if (n_rows_out) {
        HIP_TRY(hipMemcpyAsync(n_rows_out, row_start + n_pairs, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return ST_OK;
}

int evc_dtw_gather_rows(const void* src, long ld_src, int elem_stride, const int* path, const int* path_len,
                        const int* src_offsets, const int* pair_offsets, const int* row_start, int n_pairs, int cols,
                        int op, void* dst, long ld_dst, int dtype, evc_stream_t stream) {
    if (!src || !path || !path_len || !src_offsets || !pair_offsets || !row_start || !dst) return ST_BADARG;
    if (n_pairs < 1 || n_pairs > 65535 || cols < 1 || elem_stride < 1 || ld_dst < cols) return ST_BADARG;
    if (ld_src < (long)(cols - 1) * elem_stride + 1) return ST_BADARG;
    if (op != EVC_GATHER_COPY && op != EVC_GATHER_ABS) return ST_BADARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == EVC_F64)
        HIP_TRY(dtw_gather<double>(static_cast<const double*>(src), ld_src, elem_stride, path, path_len, src_offsets,
                                   pair_offsets, row_start, n_pairs, cols, op, static_cast<double*>(dst), ld_dst, s));
    else if (dtype == EVC_F32)
        HIP_TRY(dtw_gather<float>(static_cast<const float*>(src), ld_src, elem_stride, path, path_len, src_offsets,
                                  pair_offsets, row_start, n_pairs, cols, op, static_cast<float*>(dst), ld_dst, s));
    else
        return ST_BADARG;
    return ST_OK;
}

}  // extern "C"
