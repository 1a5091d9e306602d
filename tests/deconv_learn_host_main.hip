// deconv_learn_host_main.hip - a program of its own (host code only) that runs what evc_deconv_learn
// (csrc/evc_deconv_learn_plan.h) decides on the host and prints it: tests/test_deconv_learn_host.py builds it, once plainly and
// once under the address and undefined-behaviour sanitizers, and checks the lines.
//   carve <M R T n_utt taps update esize> shift <s> : <byte offsets of the twelve arrays> bytes <b> query <q>
//   args <case> <status>      deconv_learn_args_check over a grid of bad and good arguments
//   query <case> <0 | 1>      whether the workspace query is non-zero for the same sizes
//   plan <M R T taps forced> <S> <chunk> <slab bytes of one launch at 8 bytes an element>
#include "../exemplars_vc_amd/csrc/evc_deconv_learn_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace evc;

static void carve_line(int M, int R, int T_, int n_utt, int taps, int update, int dtype, size_t shift) {
    std::vector<char> mem(4096);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~uintptr_t(255)) + shift;
    const DclWs w = carve_deconv_learn(base, M, R, T_, n_utt, taps, update, dtype);      // addresses only: nothing is dereferenced
    const char* arr[] = {w.tiles, w.tpos, w.utt_tile0, w.stop, w.Xp, w.Qn, w.Qd, w.Ap1, w.Ap3, w.errf, w.ring, w.part};
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t MP = (size_t)round_up(M, 16), RP = (size_t)round_up(R, 16), nt = (size_t)frame_tile_cap(T_, BT_F, n_utt);
    const size_t img = nt * MP * BT_F * es, dict = update == EVC_DCL_BOTH ? (size_t)taps * RP * MP * es : 0;
    const DclPlan p = dcl_plan(M, R, T_, taps, 0);
    const size_t room[] = {nt * 16, nt * 16, ((size_t)n_utt + 1) * 4, (size_t)n_utt * 4, img, img, img, dict, dict,
                           (size_t)dcl_bin_groups(M, update) * nt * BT_F * 8, DCL_RING * 8,
                           (size_t)p.S * p.chunk * dcl_pair_elems(M, R) * es};
    printf("carve %d %d %d %d %d %d %zu shift %zu :", M, R, T_, n_utt, taps, update, es, shift);
    for (int i = 0; i < 12; ++i) {
        const size_t off = (size_t)(arr[i] - base);
        const size_t end = i < 11 ? (size_t)(arr[i + 1] - base) : w.bytes;
        if ((reinterpret_cast<uintptr_t>(arr[i]) & 255) != 0 || off + room[i] > end) {
            printf(" BAD");
            exit(3);
        }
        printf(" %zu", off);
    }
    const size_t need = deconv_learn_workspace_bytes(M, R, T_, n_utt, taps, update, dtype);
    if (w.bytes > need) {
        printf(" BAD SIZE");
        exit(4);
    }
    printf(" bytes %zu query %zu\n", w.bytes, need);
}

static void args_lines() {
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
    auto opts = [] {
        evc_deconv_learn_opts o{};
        o.struct_bytes = (int)sizeof(o);
        o.dtype = EVC_F64; o.layout = EVC_BIN_MAJOR; o.loss = EVC_LOSS_KL; o.taps = 4; o.iters = 100;
        o.check_every = 10; o.update = EVC_DCL_BOTH; o.tol = 1e-4;
        return o;
    };
    const int offs_ok[] = {0, 30, 30, 70}, offs_bad[] = {0, 40, 30, 70};
    // bin-major: ldx = ldh = T, ldw = R, a tap's extent is (M - 1) R + R = M R
    auto run = [&](const char* name, const evc_deconv_learn_opts& o, int M, int R, int T, size_t ws, const int* offs = nullptr,
                   int n_utt = 1, long tap_stride = -2, bool with_h = true) {
        const bool fm = o.layout == EVC_FRAME_MAJOR;
        if (tap_stride == -2) tap_stride = (long)M * R;
        int forced;
        const int st = deconv_learn_args_check(p, fm ? M : T, p, fm ? M : R, tap_stride, with_h ? p : nullptr, fm ? R : T, M, R, T,
                                               offs, n_utt, &o, p, ws, &forced);
        printf("args %s %d\n", name, st);
        printf("query %s %d\n", name, deconv_learn_workspace_bytes(M, R, T, n_utt, o.taps, o.update, o.dtype) != 0 ? 1 : 0);
    };
    const size_t big = size_t(1) << 40;
    run("ok", opts(), 25, 17, 70, big);
    run("ok_exact", opts(), 25, 17, 70, deconv_learn_workspace_bytes(25, 17, 70, 1, 4, EVC_DCL_BOTH, EVC_F64));
    run("short_by_one", opts(), 25, 17, 70, deconv_learn_workspace_bytes(25, 17, 70, 1, 4, EVC_DCL_BOTH, EVC_F64) - 1);
    run("ok_utts", opts(), 25, 17, 70, big, offs_ok, 3);
    run("bad_utts", opts(), 25, 17, 70, big, offs_bad, 3);
    run("no_utts", opts(), 25, 17, 70, big, offs_ok, 0);
    run("no_h", opts(), 25, 17, 70, big, nullptr, 1, -2, false);
    run("no_frames", opts(), 25, 17, 0, big);
    { auto o = opts(); o.layout = EVC_FRAME_MAJOR; run("ok_frame_major", o, 25, 17, 70, big, nullptr, 1, 16L * 25 + 25); }
    { auto o = opts(); o.layout = EVC_FRAME_MAJOR; run("overlap_frame_major", o, 25, 17, 70, big, nullptr, 1, 16L * 25 + 24); }
    run("overlap", opts(), 25, 17, 70, big, nullptr, 1, 25L * 17 - 1);
    run("overlap_0", opts(), 25, 17, 70, big, nullptr, 1, 0);
    run("tap_stride_neg", opts(), 25, 17, 70, big, nullptr, 1, -1);
    { auto o = opts(); o.taps = 1; run("one_tap_any_stride", o, 25, 17, 70, big, nullptr, 1, 0); }
    { auto o = opts(); o.struct_bytes = 4; run("struct_bytes", o, 25, 17, 70, big); }
    { auto o = opts(); o.taps = 0; run("taps_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.taps = DC_MAX_TAPS; run("taps_16", o, 25, 17, 70, big); }
    { auto o = opts(); o.taps = DC_MAX_TAPS + 1; run("taps_17", o, 25, 17, 70, big); }
    { auto o = opts(); o.taps = DC_MAX_TAPS + 1; run("taps_17_small_ws", o, 25, 17, 70, 16); }
    { auto o = opts(); o.loss = 2; run("loss", o, 25, 17, 70, big); }
    { auto o = opts(); o.loss = EVC_LOSS_FROBENIUS; run("frobenius", o, 25, 17, 70, big); }
    { auto o = opts(); o.update = 2; run("update", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = -1; run("iters_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = 0; run("iters_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.check_every = -1; run("check_every_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.check_every = 1; o.iters = MAX_SLOTS - 1; run("slots_4097", o, 25, 17, 70, big); }
    { auto o = opts(); o.check_every = 1; o.iters = MAX_SLOTS; run("slots_4098", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 1; run("reserved_bit0", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 1 << 16; run("reserved_bit16", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 7 << 8; run("forced_7", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 64 << 8; run("forced_64", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 65 << 8; run("forced_65", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = -1e-9; run("tol_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = 0.0; run("tol_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.l1_h = -1.0; run("l1_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.l2_h = __builtin_nan(""); run("l2_nan", o, 25, 17, 70, big); }
    { auto o = opts(); o.dtype = 7; run("dtype", o, 25, 17, 70, big); }
    { auto o = opts(); o.layout = 5; run("layout", o, 25, 17, 70, big); }
    run("M_256", opts(), 256, 17, 70, big);
    run("M_257_both", opts(), 257, 17, 70, big);
    run("M_257_both_small_ws", opts(), 257, 17, 70, 16);
    { auto o = opts(); o.update = EVC_DCL_DICT_ONLY; run("M_257_dict_small_ws", o, 257, 17, 70, 16); }
    { auto o = opts(); o.update = EVC_DCL_DICT_ONLY; run("M_1056_dict", o, 1056, 17, 70, big); }
    { auto o = opts(); o.update = EVC_DCL_DICT_ONLY; run("M_1057_dict", o, 1057, 17, 70, big); }
    run("M_1057_both", opts(), 1057, 17, 70, big);
    run("R_4096", opts(), 25, 4096, 70, big);
    run("R_4097", opts(), 25, 4097, 70, big);
    run("R_4097_small_ws", opts(), 25, 4097, 70, 16);
    { auto o = opts(); o.tol = __builtin_nan(""); run("nan_before_limits", o, 257, 17, 70, 16); }
    { auto o = opts(); o.taps = 0; run("taps_0_before_limits", o, 257, 17, 70, 16); }
    run("overlap_before_limits", opts(), 257, 17, 70, 16, nullptr, 1, 5);
}

static void plan_line(int M, int R, int T_, int taps, int forced) {
    const DclPlan p = dcl_plan(M, R, T_, taps, forced);
    printf("plan %d %d %d %d %d %d %d %zu\n", M, R, T_, taps, forced, p.S, p.chunk,
           (size_t)p.S * p.chunk * dcl_pair_elems(M, R) * 8);
}

int main() {
    for (size_t shift : {size_t(0), size_t(8)}) {
        carve_line(25, 12, 90, 4, 4, EVC_DCL_BOTH, EVC_F64, shift);
        carve_line(50, 512, 65536, 96, 8, EVC_DCL_BOTH, EVC_F64, shift);
        carve_line(201, 512, 32768, 48, 4, EVC_DCL_BOTH, EVC_F32, shift);
        carve_line(1056, 4096, 4096, 1, 16, EVC_DCL_DICT_ONLY, EVC_F64, shift);
        carve_line(513, 16, 40, 1, 3, EVC_DCL_DICT_ONLY, EVC_F32, shift);
        carve_line(1, 1, 1, 1, 1, EVC_DCL_BOTH, EVC_F32, shift);
    }
    args_lines();
    for (int taps : {1, 4, 16}) {
        plan_line(25, 12, 90, taps, 0);
        plan_line(50, 512, 65536, taps, 0);
        plan_line(201, 512, 32768, taps, 0);
        plan_line(256, 4096, 1000000, taps, 0);
        plan_line(1056, 4096, 1000000, taps, 0);
        plan_line(1056, 4096, 1000000, taps, 64);
        plan_line(25, 12, 90, taps, 7);
    }
    return 0;
}
