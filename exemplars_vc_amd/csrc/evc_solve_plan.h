// What evc_nmf_solve / evc_nmf_convert decide and carve before anything is launched (driver: evc_api.hip): the route of an
// attempt (plan_route), the tail of a fused attempt (plan_fused_tail), the workspace of every driver and the image of a
// prepared dictionary.  Pure host arithmetic: no HIP call, no global state; where the device's CU count matters it is an
// argument.  tests/solve_plan_host_main.hip prints all of it without a device.
#pragma once
#include "evc_internal.h"

#include <algorithm>

namespace evc {

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
inline int algo_eff(int algo) { return algo == EVC_ALGO_AUTO ? EVC_ALGO_FACTORED : algo; }
// Which kernels a (M, N, T) problem of one dtype can be routed to.  plan_route, the workspace and dictionary size queries
// and the prepared images all ask these two, so that a new route family is added here and in plan_route only.
// The float64 fused kernels (M <= 32); float32 callers ride them through a staging copy (solve_f32_on_f64).
inline bool small_family(int M, int N, int T_, int algo) {
    return algo == EVC_ALGO_FACTORED && fused_supported(M, N, T_, EVC_F64);
}
// the task-queue kernels: k_fused_wide (float32), k_fused_wide64 (float64)
inline bool wide_family(int M, int N, int T_, int dtype, int algo, int loss) {
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
// staging of a float32 dictionary that rides the float64 fused kernels: A and B widened once
inline size_t dict_f64_staging(int M, int Mb, int N) {
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

inline UttState take_utt(Carver& c, const Dims& d, int n_slots) {
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

// The workspace of the task-queue drivers: k_fused_wide (float32, 32 < M <= 208) and k_fused_wide64 (float64)
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

// callers may disable the fused kernels per call, so the query covers the carving of every route the sizes allow
template <typename T> size_t workspace_typed(int M, int Mb, int N, int T_, int n_utt, int algo, int n_cus) {
    const Dims d = make_dims((int)sizeof(T), M, N, T_, n_utt, Mb);
    const int al = algo_eff(algo);
    const int dt = sizeof(T) == 8 ? EVC_F64 : EVC_F32;
    size_t b = carve<T>(nullptr, d, al, MAX_SLOTS, false).bytes;
    if (dt == EVC_F64 && small_family(M, N, T_, al))
        b = std::max(b, carve<T>(nullptr, d, al, MAX_SLOTS, true).bytes);
    if (wide_family(M, N, T_, dt, al, EVC_LOSS_FROBENIUS))
        b = std::max(b, carve_wide<T>(nullptr, d, MAX_SLOTS, n_cus, true, sizeof(T) == 4).bytes);
    return b;
}
// float32 callers with a small bin count: the float64 fused kernels are 2.5x faster than the float32
// generic path (and exact to float32 rounding), so their matrices are widened into a staging region, solved by
// the float64 route and narrowed on the way out.  The reference's float32 surface (nmf_tool, TF1) is compared
// against a float64 restatement anyway: computing in float64 only moves the result towards it.
inline size_t f32_staging_bytes(int M, int Mb, int N, int T) {
    const size_t n = (size_t)N * M + (size_t)T * M + (size_t)T * N + (size_t)N * Mb + (size_t)T * Mb;
    return ((n * sizeof(double) + 6 * 256) + 255) & ~size_t(255);   // the inner workspace starts 256-byte aligned
}

// evc_solve_opts.reserved, decoded once per attempt (by plan_route)
struct SolveFlags {
    bool no_fused, exact_div, no_exchange, no_all_resident, pair_tiles;
    int c_req;           // bits 8..15: M <= 32: 1 | 2 = the general kernel; M > 32: exemplar ranges per frame group
    int w_req;           // bits 16..19: wavefronts per workgroup (k_fused_wide), whole bin tiles per wavefront (k_fused_wide64)
};
inline SolveFlags decode_flags(int reserved, int stop_rule) {
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
inline bool use_wide(int M, int N, int T_, int dtype, int algo, int loss, const SolveFlags& f) {
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
inline Route plan_route(int M, int N, int T_, int dtype, const evc_solve_opts& o, int n_cus) {
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

// The tail of one fused attempt (ROUTE_FUSED), decided before its first launch: what the last launch of the iteration
// loop does beyond the updates, what finish_fused does after it, and when the abort word of an exchange is read.
// given: caller-given start values; want_h: the caller wants H; synth: a synthesis follows; packed_synth: Workspace's;
// slabs: the workspace holds a slab of Y per member of THIS route (w.Yslab && w.y_members == r.members).
enum { Y_NONE, Y_SLABS, Y_PREPASS, Y_ROWS };
struct FusedTail {
    bool direct_h;       // the last launch writes the caller's H itself (nothing can stop: k_fused_all / k_fused_xy)
    bool y_in_kernel;    // ... and k_fused_all forms the members' shares of Y from the activations in its registers
    bool skip_hp;        // ... and does not store the packed activations: nothing reads them afterwards
    int variant;         // evc_solve_info.variant: reported for a synthesis formed in the kernel only, else 0
    bool export_h;       // finish_fused: H out of the packed tiles
    int y_from;          // finish_fused: Y_SLABS (the members' shares are summed), Y_PREPASS (the pass over the packed
                         // activations with B's fragments), Y_ROWS (frames-as-rows H and a contraction), Y_NONE
    // A cooperative launch that gave up waiting for a peer workgroup (another process or stream held the CUs it needed)
    // leaves void results, and the solve is redone without exchange (solve_checked).  The flag costs a host round trip:
    // when the start values can be regenerated it is read after the tail (whose results the redo writes again); with
    // caller-given start values it is read before anything is written to the caller's H - no direct export then.
    bool check_first;
};
inline FusedTail plan_fused_tail(const FusedRoute& r, int iters, bool given, bool want_h, bool synth, bool packed_synth,
                                 bool slabs) {
    FusedTail t{};
    t.check_first = given;
    const bool last = r.direct_export && iters > 0;      // (iters == 0: there is no last launch)
    t.direct_h = last && want_h && !given;
    if (last && r.kernel == EVC_KERNEL_FUSED_ALL) {
        t.y_in_kernel = synth && packed_synth && slabs;
        t.skip_hp = !(given && want_h) && (!synth || t.y_in_kernel);
        t.variant = t.y_in_kernel ? (1 | (t.skip_hp ? 0 : 2)) : 0;
    }
    t.export_h = want_h && !t.direct_h;
    t.y_from = !synth ? Y_NONE : (t.y_in_kernel ? Y_SLABS : (packed_synth ? Y_PREPASS : Y_ROWS));
    return t;
}

}  // namespace evc
