// Prints what evc_nmf_solve / evc_nmf_convert decide and carve before anything is launched (csrc/evc_solve_plan.h), one
// record per line over a fixed grid, for tests/test_solve_plan_host.py and tools/make_golden_solve_plan.py: every field of
// plan_route, every field of plan_fused_tail, and the byte offsets of every sub-array of carve<T>, carve_wide<T> and
// dict_image<T> from a base that is never dereferenced.  Host code only: built with the host half of hipcc, linked against
// libevc_hip.so for the layout functions (fused_layout, wide_layout, fused_all_members, ...); no HIP call, no arguments.
//
// -DSOLVE_PLAN_PARENT: the build that recorded tests/golden/solve_plan.json on the commit before the header existed: the
// same names came from csrc/evc_api.hip then (included whole: they were local to it), and the tail of a fused attempt was
// decided inside solve_typed / solve_fused / finish_fused, whose conditions are restated literally below.
#ifdef SOLVE_PLAN_PARENT
#include "../exemplars_vc_amd/csrc/evc_api.hip"
#else
#include "../exemplars_vc_amd/csrc/evc_solve_plan.h"
#endif

#include <stdio.h>

using namespace evc;

#ifdef SOLVE_PLAN_PARENT
namespace {
enum { Y_NONE, Y_SLABS, Y_PREPASS, Y_ROWS };
struct FusedTail { bool direct_h, y_in_kernel, skip_hp; int variant; bool export_h; int y_from; bool check_first; };
FusedTail plan_fused_tail(const FusedRoute& r, int iters, bool given, bool want_h, bool synth, bool packed_synth, bool slabs) {
    // stand-ins for what those statements name: the caller's H and the synthesis (NULL: none), the workspace's slabs (only
    // whether `w.Yslab && w.y_members == r.members` holds is an input here), the options and the info record
    static double h_there, slab_there;
    static SynthArgs y_there;
    double* const H = want_h ? &h_there : nullptr;
    const SynthArgs* const y = synth ? &y_there : nullptr;
    struct { bool packed_synth; double* Yslab; int y_members; } w = {packed_synth, slabs ? &slab_there : nullptr, r.members};
    struct { int init_mode, iters, check_every; } o = {given ? EVC_INIT_GIVEN : EVC_INIT_SKLEARN, iters, 0};
    struct { int variant; } inf_{}, *inf = &inf_;
    struct { int skip_hp; } fb{};
    // ---- solve_typed, evc_api.hip:832-843 ----
    const bool check_first = (o.init_mode == EVC_INIT_GIVEN);
    int exported_ = 0, y_done_ = 0, *exported = &exported_, *y_done = &y_done_;
    inf->variant = 0;
    double* const H_out = check_first ? nullptr : H;      // solve_fused(..., check_first ? nullptr : H, ldh, check_first && H, y, ...)
    const bool h_later = check_first && H;
    // ---- solve_fused, evc_api.hip:421-442 ----
    int done = 0;
    while (done < o.iters) {
        int n = o.iters - done;
        if (o.check_every > 0 && n >= o.check_every) { n = o.check_every; }
        if (H_out && r.direct_export && done + n == o.iters) {
            *exported = 1;
        }
        if (r.kernel == EVC_KERNEL_FUSED_ALL && r.direct_export && done + n == o.iters) {
            if (y && w.packed_synth && w.Yslab && w.y_members == r.members) {
                *y_done = 1;
            }
            fb.skip_hp = (!h_later && (!y || *y_done)) ? 1 : 0;
            inf->variant = *y_done ? (1 | (fb.skip_hp ? 0 : 2)) : 0;
        }
        done += n;
    }
    // ---- solve_typed, evc_api.hip:846: finish_fused(w, d, o, exported ? nullptr : H, ldh, y, y_done, ...), :460-477 ----
    FusedTail t{};
    t.direct_h = *exported; t.y_in_kernel = *y_done; t.skip_hp = fb.skip_hp; t.variant = inf->variant; t.check_first = check_first;
    {
        double* const H = *exported ? nullptr : (want_h ? &h_there : nullptr);
        t.export_h = H != nullptr;                     // if (H) fused_export_h(...)
        if (!y) t.y_from = Y_NONE;                     // if (!y) return ST_OK;
        else if (*y_done) t.y_from = Y_SLABS;          // if (y_done) fused_unpack_y(...)
        else if (w.packed_synth) t.y_from = Y_PREPASS; // if (w.packed_synth) fused_synthesize(...)
        else t.y_from = Y_ROWS;                        // fused_export_h(..., w.H0, ...); synth_rows(...)
    }
    return t;
}
}  // namespace
#endif

static char* const g_base = reinterpret_cast<char*>(uintptr_t(1) << 40);      // never dereferenced
static long off(const void* p) { return p ? (long)(static_cast<const char*>(p) - g_base) : -1; }

static const int MS[] = {1, 16, 17, 25, 32, 33, 64, 144, 145, 176, 177, 201, 208, 209, 257, 513, 528, 529, 1025};
static const int MBS[] = {0, 25, 40, 513};
static const int NS[] = {15, 16, 512, 4096, 16384};
static const int TS[] = {1, 90, 688, 11008, 70000};
static const int UTTS[] = {1, 16};
// evc_solve_opts.reserved of tools/route_dump.py's solve cases: defaults, fused=False, exact_div, cooperative=False,
// all_resident=False, pair_tiles, fused_c = 1 | 2, fused_w = 4 | 8, cooperative=False with all_resident=False
static const int FLAGS[] = {0, EVC_FLAG_NO_FUSED, EVC_FLAG_EXACT_DIV, EVC_FLAG_NO_EXCHANGE, EVC_FLAG_NO_ALL_RESIDENT,
                            EVC_FLAG_PAIR_TILES, 1 << 8, 2 << 8, 4 << 16, 8 << 16, EVC_FLAG_NO_EXCHANGE | EVC_FLAG_NO_ALL_RESIDENT};
static const int CUS[] = {256, 64, 8};
// the shapes of those cases themselves (utterances of 688 frames, and the 90-frame ones)
static const int SOLVE_SHAPES[][3] = {
    {25, 512, 11008}, {25, 4096, 1376}, {25, 1024, 17}, {12, 1536, 90}, {64, 4096, 688}, {201, 4096, 1376},
    {201, 8192, 11008}, {513, 1024, 2064}};

// which return of use_wide / which assignments of plan_route a case went through, restated from their inputs and results
enum { UW_NO_FUSED, UW_NO_EXCHANGE, UW_F64_UNSUPPORTED, UW_F64_FORCED, UW_F64_M176, UW_F64_M208_IN, UW_F64_M208_OUT,
       UW_F64_IN, UW_F64_OUT, UW_F32_UNSUPPORTED, UW_F32_FORCED, UW_F32_IN, UW_F32_OUT,
       PR_GEMM, PR_WIDE, PR_FUSED, PR_STAGED, PR_ALL_ONE, PR_ALL_MEMBERS, PR_XY, PR_RES, PR_RES_COOP, PR_MU, PR_MU_FORCED,
       PR_INIT_CONST, PR_DIRECT_EXPORT, N_BRANCHES };
static const char* const BRANCH_NAMES[N_BRANCHES] = {
    "use_wide.no_fused", "use_wide.no_exchange", "use_wide.f64_unsupported", "use_wide.f64_forced", "use_wide.f64_m<=176",
    "use_wide.f64_m<=208_in", "use_wide.f64_m<=208_out", "use_wide.f64_in", "use_wide.f64_out", "use_wide.f32_unsupported",
    "use_wide.f32_forced", "use_wide.f32_in", "use_wide.f32_out",
    "plan_route.gemm", "plan_route.wide", "plan_route.fused", "plan_route.staged", "plan_route.all_one_member",
    "plan_route.all_members", "plan_route.xy", "plan_route.res", "plan_route.res_coop", "plan_route.mu",
    "plan_route.mu_forced", "plan_route.init_const", "plan_route.direct_export"};
static long g_branch[N_BRANCHES];

static void count_branches(int M, int N, int T_, int dtype, const evc_solve_opts& o, const Route& r) {
    const SolveFlags f = decode_flags(o.reserved, o.stop_rule);
    if (r.family != ROUTE_FUSED) {      // use_wide was asked
        const bool forced = f.c_req != 0 || f.w_req != 0, in = r.family == ROUTE_WIDE;
        int b;
        if (f.no_fused) b = UW_NO_FUSED;
        else if (f.no_exchange) b = UW_NO_EXCHANGE;
        else if (dtype == EVC_F64)
            b = !wide64_supported(M, N, T_, dtype, r.algo, o.loss) ? UW_F64_UNSUPPORTED
                : forced ? UW_F64_FORCED
                : M <= 176 ? UW_F64_M176
                : M <= 208 ? (in ? UW_F64_M208_IN : UW_F64_M208_OUT) : (in ? UW_F64_IN : UW_F64_OUT);
        else
            b = !wide_supported(M, N, T_, dtype, r.algo) ? UW_F32_UNSUPPORTED
                : forced ? UW_F32_FORCED : (in ? UW_F32_IN : UW_F32_OUT);
        ++g_branch[b];
        ++g_branch[in ? PR_WIDE : PR_GEMM];
        return;
    }
    ++g_branch[PR_FUSED];
    if (r.staged) ++g_branch[PR_STAGED];
    const FusedRoute& k = r.fused;
    if (k.kernel == EVC_KERNEL_FUSED_ALL) ++g_branch[k.members == 1 ? PR_ALL_ONE : PR_ALL_MEMBERS];
    if (k.kernel == EVC_KERNEL_FUSED_XY) ++g_branch[PR_XY];
    if (k.kernel == EVC_KERNEL_FUSED_RES) ++g_branch[k.members > 1 ? PR_RES_COOP : PR_RES];
    if (k.kernel == EVC_KERNEL_FUSED_MU) ++g_branch[f.c_req ? PR_MU_FORCED : PR_MU];
    if (k.init_const) ++g_branch[PR_INIT_CONST];
    if (k.direct_export) ++g_branch[PR_DIRECT_EXPORT];
}

static void route_line(int M, int N, int T_, int dtype, int reserved, int eps_mode, int loss, int stop_rule, int check_every,
                       int init_mode, int iters, int algo, int n_cus) {
    evc_solve_opts o{};
    o.struct_bytes = (int)sizeof(o);
    o.dtype = dtype; o.algo = algo; o.iters = iters; o.eps_mode = eps_mode; o.init_mode = init_mode;
    o.check_every = check_every; o.stop_rule = stop_rule; o.reserved = reserved; o.loss = loss;
    const Route r = plan_route(M, N, T_, dtype, o, n_cus);
    count_branches(M, N, T_, dtype, o, r);
    const SolveFlags& f = r.flags;
    const FusedRoute& k = r.fused;
    printf("route %d %d %d %d %d %d %d %d %d %d %d %d %d : %d %d %d %d  %d %d %d %d %d %d %d  %d %d %d %d %d %d %d\n", M, N, T_,
           dtype, reserved, eps_mode, loss, stop_rule, check_every, init_mode, iters, algo, n_cus, r.family, (int)r.staged,
           r.algo, r.n_cus, (int)f.no_fused, (int)f.exact_div, (int)f.no_exchange, (int)f.no_all_resident, (int)f.pair_tiles,
           f.c_req, f.w_req, k.kernel, k.members, k.c_req, k.exact_div, k.init_const, k.direct_export, k.n_cus);
}

static void print_layout(const FusedLayout& l) {
    printf(" %d %d %d %d %d %d %zu %zu %zu %zu %zu", l.NT, l.TT, l.TTp, l.msteps, l.mtiles, l.M, l.a1, l.a2, l.xp, l.hp, l.vp);
}
static void print_utt(const UttState& u) {
    printf(" %ld %ld %ld %ld %ld %ld %ld %ld %d", off(u.frame_utt), off(u.offsets), off(u.active), off(u.n_iter),
           off(u.err_init), off(u.err_prev), off(u.h0), off(u.trace), u.n_slots);
}

template <typename T> static void carve_line(int M, int Mb, int N, int T_, int n_utt, int algo, bool fused) {
    const Dims d = make_dims((int)sizeof(T), M, N, T_, n_utt, Mb);
    const Workspace<T> w = carve<T>(g_base, d, algo, MAX_SLOTS, fused);
    printf("carve %d %d %d %d %d %d %d %d : %zu %zu  %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %zu %ld ", (int)sizeof(T), M, Mb,
           N, T_, n_utt, algo, (int)fused, w.bytes, w.bytes_min, off(w.At), off(w.Am), off(w.Xt), off(w.H0), off(w.H1),
           off(w.Pt), off(w.G), off(w.Vt), off(w.Akl), off(w.Rt), off(w.Vsplit), w.vsplit_elems, off(w.err2));
    print_utt(w.u);
    printf(" ");
    print_layout(w.fl);
    printf("  %ld %ld %ld %ld %ld %ld %ld %ld ", off(w.fb.A1p), off(w.fb.A2p), off(w.fb.Xp), off(w.fb.Hp), off(w.fb.Vp),
           off(w.fb.coop_buf), off(w.fb.coop_cnt), off(w.fb.rsum));
    print_layout(w.flB);
    printf("  %ld %ld %ld %ld %ld %d %d %d\n", off(w.Bt), off(w.B1p), off(w.B2p), off(w.Yp), off(w.Yslab), w.y_members,
           (int)w.fused, (int)w.packed_synth);
}

template <typename T> static void wide_line(int M, int Mb, int N, int T_, int n_utt, int n_cus) {
    const Dims d = make_dims((int)sizeof(T), M, N, T_, n_utt, Mb);
    const WideWs<T> w = carve_wide<T>(g_base, d, MAX_SLOTS, n_cus, true, sizeof(T) == 4);
    printf("wide %d %d %d %d %d %d %d : %zu  %ld %ld %ld %ld  %ld %ld %ld %ld %ld %ld %ld  %zu %zu %zu %zu %zu %zu %d  %ld", (int)sizeof(T),
           M, Mb, N, T_, n_utt, n_cus, w.bytes, off(w.At), off(w.Akl), off(w.Xt), off(w.H0), off(w.fb.Aw), off(w.fb.Xw),
           off(w.fb.Hw), off(w.fb.Pw), off(w.fb.Vpart), off(w.fb.Vsum), off(w.fb.ctl), w.caps.aw, w.caps.xw, w.caps.hw,
           w.caps.vpart, w.caps.vsum, w.caps.ctl, w.caps.c_cap, off(w.err2));
    print_utt(w.u);
    if constexpr (sizeof(T) == 4)
        printf("  %ld %zu %ld %ld %d", off(w.fb.Hs), w.fb.hs_stride, off(w.fb.err2s), w.fb.err_stride, w.fb.snap_slots);
    printf("\n");
}

template <typename T> static void dict_line(int M, int Mb, int N, int loss, size_t skip) {
    const DictImage<T> im = dict_image<T>(g_base, skip, M, Mb, N, loss);
    const DictArrays<T>& a = im.a;
    printf("dict %d %d %d %d %d %zu : %zu  %d %d %d %d %d %d  %d %d %d %d  %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld\n",
           (int)sizeof(T), M, Mb, N, loss, skip, im.bytes, (int)im.plan.fused, (int)im.plan.packed_b, (int)im.plan.wide,
           (int)im.plan.wide64, (int)im.plan.kl, (int)im.plan.bc, im.d.Mk, im.d.Mj, im.d.Np, im.d.Tp, off(a.At), off(a.Am),
           off(a.Akl), off(a.A1p), off(a.A2p), off(a.rsum), off(a.Bt), off(a.B1p), off(a.B2p), off(a.Bc), off(a.Aw),
           off(a.Aw64));
}

int main() {
    puts("# route M N T dtype reserved eps_mode loss stop_rule check_every init_mode iters algo n_cus : family staged algo n_cus"
         "  no_fused exact_div no_exchange no_all_resident pair_tiles c_req w_req  kernel members c_req exact_div init_const"
         " direct_export n_cus");
    // the whole product, thinned by a prime stride: every dimension keeps every value, paired differently each time round
    long k = 0;
    for (int M : MS) for (int N : NS) for (int T_ : TS) for (int dtype = 0; dtype < 2; ++dtype) for (int reserved : FLAGS)
        for (int eps_mode = 0; eps_mode < 4; ++eps_mode) for (int loss = 0; loss < 2; ++loss)
            for (int stop_rule = 0; stop_rule < 3; ++stop_rule) for (int check_every = 0; check_every <= 10; check_every += 10)
                for (int init_mode = 0; init_mode < 3; ++init_mode) for (int iters = 0; iters <= 10; iters += 10)
                    for (int n_cus : CUS)
                        if (k++ % 48017 == 0)
                            route_line(M, N, T_, dtype, reserved, eps_mode, loss, stop_rule, check_every, init_mode, iters,
                                       EVC_ALGO_AUTO, n_cus);
    // the solve cases' own shapes under every flag, and under the options one at a time
    for (const auto& sh : SOLVE_SHAPES)
        for (int dtype = 0; dtype < 2; ++dtype) {
            for (int reserved : FLAGS)
                route_line(sh[0], sh[1], sh[2], dtype, reserved, EVC_EPS_ADD, 0, EVC_STOP_NONE, 0, EVC_INIT_SKLEARN, 10,
                           EVC_ALGO_AUTO, 256);
            if (dtype != (sh[0] > 32 && sh[0] <= 208 ? EVC_F32 : EVC_F64)) continue;      // (the options: the cases' own dtype)
            for (int eps_mode = 1; eps_mode < 4; ++eps_mode)
                route_line(sh[0], sh[1], sh[2], dtype, 0, eps_mode, 0, EVC_STOP_NONE, 0, EVC_INIT_SKLEARN, 10, EVC_ALGO_AUTO, 256);
            route_line(sh[0], sh[1], sh[2], dtype, 0, EVC_EPS_ZERO_REPLACE, 1, EVC_STOP_NONE, 0, EVC_INIT_SKLEARN, 10, EVC_ALGO_AUTO, 256);
            for (int stop_rule = 0; stop_rule < 3; ++stop_rule)
                route_line(sh[0], sh[1], sh[2], dtype, 0, EVC_EPS_ADD, 0, stop_rule, 10, EVC_INIT_SKLEARN, 30, EVC_ALGO_AUTO, 256);
            for (int init_mode = 0; init_mode < 3; init_mode += 2)
                route_line(sh[0], sh[1], sh[2], dtype, 0, EVC_EPS_ADD, 0, EVC_STOP_NONE, 0, init_mode, 10, EVC_ALGO_AUTO, 256);
            for (int algo = 0; algo < 3; ++algo)
                route_line(sh[0], sh[1], sh[2], dtype, 0, EVC_EPS_ADD, 0, EVC_STOP_NONE, 0, EVC_INIT_SKLEARN, 10, algo, 256);
            for (int n_cus = 64; n_cus >= 8; n_cus -= 56)
                route_line(sh[0], sh[1], sh[2], dtype, 0, EVC_EPS_ADD, 0, EVC_STOP_NONE, 0, EVC_INIT_SKLEARN, 10, EVC_ALGO_AUTO, n_cus);
        }
    for (int b = 0; b < N_BRANCHES; ++b) printf("branch %s %ld\n", BRANCH_NAMES[b], g_branch[b]);

    puts("# tail kernel direct_export iters : 32 plans, one per bits = given | want_h << 1 | synth << 2 | packed_synth << 3 |"
         " slabs << 4, each the digits direct_h y_in_kernel skip_hp variant export_h y_from check_first");
    for (int kernel = EVC_KERNEL_FUSED_MU; kernel <= EVC_KERNEL_FUSED_XY; ++kernel) {
        if (kernel == EVC_KERNEL_FUSED_WIDE || kernel == EVC_KERNEL_FUSED_WIDE64) continue;
        for (int direct = 0; direct < 2; ++direct) for (int iters = 0; iters <= 10; iters += 5) {
            printf("tail %d %d %d :", kernel, direct, iters);
            for (int bits = 0; bits < 32; ++bits) {
                FusedRoute r{};
                r.kernel = kernel; r.members = 2; r.direct_export = direct;
                const bool given = bits & 1, want_h = bits & 2, synth = bits & 4, packed = bits & 8, slabs = bits & 16;
                const FusedTail t = plan_fused_tail(r, iters, given, want_h, synth, packed, slabs);
                printf(" %d%d%d%d%d%d%d", (int)t.direct_h, (int)t.y_in_kernel, (int)t.skip_hp, t.variant, (int)t.export_h,
                       t.y_from, (int)t.check_first);
            }
            printf("\n");
        }
    }

    puts("# carve esize M Mb N T n_utt algo fused : bytes bytes_min  At Am Xt H0 H1 Pt G Vt Akl Rt Vsplit vsplit_elems err2"
         "  u(frame_utt offsets active n_iter err_init err_prev h0 trace n_slots)  fl(NT TT TTp msteps mtiles M a1 a2 xp hp vp)"
         "  fb(A1p A2p Xp Hp Vp coop_buf coop_cnt rsum)  flB(...)  Bt B1p B2p Yp Yslab y_members fused packed_synth");
    puts("# wide esize M Mb N T n_utt n_cus : bytes  At Akl Xt H0  fb(Aw Xw Hw Pw Vpart Vsum ctl)  caps(aw xw hw vpart vsum ctl"
         " c_cap)  err2 u(...)  [float32: Hs hs_stride err2s err_stride snap_slots]");
    k = 0;
    for (int M : MS) for (int Mb : MBS) for (int N : NS) for (int T_ : TS) for (int n_utt : UTTS) {
        const bool small = small_family(M, N, T_, EVC_ALGO_FACTORED);
        // every M <= 32 shape with a synthesis from the packed tiles shows the slabs' carving; the rest is thinned
        const bool pick = k++ % 97 == 0 || (small && M >= 17 && Mb == 25 && N == 4096 && T_ >= 688 && n_utt == 1);
        if (!pick) continue;
        const int algo = (k / 97) % 2 ? EVC_ALGO_FACTORED : EVC_ALGO_GRAM;
        carve_line<double>(M, Mb, N, T_, n_utt, algo, false);
        carve_line<float>(M, Mb, N, T_, n_utt, algo, false);
        if (small) carve_line<double>(M, Mb, N, T_, n_utt, EVC_ALGO_FACTORED, true);
        const int n_cus = CUS[(k / 97) % 3];
        if (wide_family(M, N, T_, EVC_F32, EVC_ALGO_FACTORED, EVC_LOSS_FROBENIUS)) wide_line<float>(M, Mb, N, T_, n_utt, n_cus);
        if (wide_family(M, N, T_, EVC_F64, EVC_ALGO_FACTORED, EVC_LOSS_FROBENIUS)) wide_line<double>(M, Mb, N, T_, n_utt, n_cus);
    }

    puts("# dict esize M Mb N loss skip : bytes  plan(fused packed_b wide wide64 kl bc)  Mk Mj Np Tp  At Am Akl A1p A2p rsum Bt B1p"
         " B2p Bc Aw Aw64");
    k = 0;
    for (int M : MS) for (int Mb : MBS) for (int N : NS) for (int loss = 0; loss < 2; ++loss) {
        if (k++ % 13 != 0 && !(M == 25 && N == 4096)) continue;
        dict_line<double>(M, Mb, N, loss, 0);
        if (small_family(M, N, 1, EVC_ALGO_FACTORED)) dict_line<double>(M, Mb, N, loss, dict_f64_staging(M, Mb, N));
        else dict_line<float>(M, Mb, N, loss, 0);
    }
    return 0;
}
