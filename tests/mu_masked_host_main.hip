// mu_masked_host_main.hip - a program of its own (host code only) that runs what evc_mu_masked_solve
// (csrc/evc_mu_masked_plan.h) decides on the host and prints it: tests/test_mu_masked_host.py builds it, once plainly and once
// under the address and undefined-behaviour sanitizers, and checks the lines.
//   carve <M N T n_utt esize> shift <s> : <byte offsets of the 12 arrays in carving order> bytes <b> query <q>
//   args <case> <status>    mum_args_check over a grid of bad and good arguments
//   query <case> <bytes>    mum_workspace_bytes where the call refuses with -1 or -3 (0) and where it does not
//   slots <iters check_every> <n>   the error slots
//   lcarve <M R T esize> shift <s> : <byte offsets of the 9 arrays of evc_mu_masked_learn> bytes <b> query <q>
//   largs <case> <status> <forced>   mum_learn_args_check
//   lquery <case> <bytes>
#include "../exemplars_vc_amd/csrc/evc_mu_masked_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace evc;

static void carve_line(int M, int N, int T_, int n_utt, int dtype, size_t shift) {
    std::vector<char> mem(4096);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~uintptr_t(255)) + shift;
    const MumWs w = carve_mum(base, M, N, T_, n_utt, dtype);      // addresses only: nothing is dereferenced
    const char* arr[MUM_WS_ARRAYS] = {
        w.Ap1, w.Ap3, w.Xp, w.XMp, w.Mp, reinterpret_cast<char*>(w.errf), reinterpret_cast<char*>(w.tiles),
        reinterpret_cast<char*>(w.utt_tile0),
        reinterpret_cast<char*>(w.stop), reinterpret_cast<char*>(w.einit), reinterpret_cast<char*>(w.eprev),
        reinterpret_cast<char*>(w.trace)};
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t MP = (size_t)round_up(M, 16), NP = (size_t)round_up(N, 16);
    // the tiles a call can have: every utterance starts one of its own
    const size_t nt = (size_t)(T_ + MUM_F - 1) / MUM_F + n_utt;
    const size_t room[MUM_WS_ARRAYS] = {
        NP * MP * es, NP * MP * es, nt * MP * 16 * es, nt * MP * 16 * es, nt * MP * 16 * es, nt * 16 * 8, nt * 16,
        ((size_t)n_utt + 1) * 4, (size_t)n_utt * 4, (size_t)n_utt * 8, (size_t)n_utt * 8,
        (size_t)n_utt * MUM_MAX_SLOTS * 8};
    printf("carve %d %d %d %d %zu shift %zu :", M, N, T_, n_utt, es, shift);
    for (int i = 0; i < MUM_WS_ARRAYS; ++i) {
        const size_t off = (size_t)(arr[i] - base);
        const size_t end = i < MUM_WS_ARRAYS - 1 ? (size_t)(arr[i + 1] - base) : w.bytes;
        if ((reinterpret_cast<uintptr_t>(arr[i]) & 255) != 0 || off + room[i] > end) {
            printf(" BAD");
            exit(3);
        }
        printf(" %zu", off);
    }
    const size_t need = mum_workspace_bytes(M, N, T_, n_utt, dtype);
    if (w.bytes > need) {
        printf(" BAD SIZE");
        exit(4);
    }
    printf(" bytes %zu query %zu\n", w.bytes, need);
}

static void args_lines() {
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
    auto opts = [] {
        evc_mu_masked_opts o{};
        o.struct_bytes = (int)sizeof(o);
        o.dtype = EVC_F64; o.layout = EVC_FRAME_MAJOR; o.loss = EVC_LOSS_KL; o.iters = 100;
        o.init_mode = EVC_INIT_CONST; o.check_every = 10; o.stop_rule = EVC_STOP_SKLEARN; o.tol = 1e-3; o.init_value = 1.0;
        return o;
    };
    const int offs_ok[] = {0, 30, 30, 70}, offs_bad[] = {0, 40, 30, 70};
    auto run = [&](const char* name, const evc_mu_masked_opts& o, int M, int N, int T, size_t ws, const int* offs = nullptr,
                   int n_utt = 1, bool with_x = true, bool with_mask = true, int ldm = -1, int lda = -1, int ldh = -1) {
        const int st = mum_args_check(p, lda < 0 ? M : lda, with_x ? p : nullptr, M, with_mask ? p : nullptr, ldm < 0 ? M : ldm, p,
                                      ldh < 0 ? N : ldh, M, N, T, offs, n_utt, &o, p, ws);
        printf("args %s %d\n", name, st);
    };
    const size_t big = size_t(1) << 40;
    run("ok", opts(), 25, 17, 70, big);
    run("ok_exact", opts(), 25, 17, 70, mum_workspace_bytes(25, 17, 70, 1, EVC_F64));
    run("short_by_one", opts(), 25, 17, 70, mum_workspace_bytes(25, 17, 70, 1, EVC_F64) - 1);
    run("f32_ws", opts(), 25, 17, 70, mum_workspace_bytes(25, 17, 70, 1, EVC_F32));
    run("ok_utts", opts(), 25, 17, 70, big, offs_ok, 3);
    run("bad_utts", opts(), 25, 17, 70, big, offs_bad, 3);
    run("no_frames_no_x", opts(), 25, 17, 0, big, nullptr, 1, false);
    run("frames_no_x", opts(), 25, 17, 70, big, nullptr, 1, false);
    run("no_mask", opts(), 25, 17, 70, big, nullptr, 1, true, false);
    run("no_mask_any_ldm", opts(), 25, 17, 70, big, nullptr, 1, true, false, 0);
    run("ldm_short", opts(), 25, 17, 70, big, nullptr, 1, true, true, 24);
    run("ldm_padded", opts(), 25, 17, 70, big, nullptr, 1, true, true, 31);
    run("lda_short", opts(), 25, 17, 70, big, nullptr, 1, true, true, -1, 24);
    run("ldh_short", opts(), 25, 17, 70, big, nullptr, 1, true, true, -1, -1, 16);
    { auto o = opts(); o.layout = EVC_BIN_MAJOR; run("ldm_short_bin_major", o, 70, 70, 70, big, nullptr, 1, true, true, 69); }
    { auto o = opts(); o.struct_bytes = (int)sizeof(evc_beta_opts); run("struct_bytes", o, 25, 17, 70, big); }
    { auto o = opts(); o.struct_bytes = 0; run("struct_bytes_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = -1; run("iters_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = 0; run("iters_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = MUM_MAX_SLOTS - 1; o.check_every = 1; run("slots_4097", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = MUM_MAX_SLOTS; o.check_every = 1; run("slots_4098", o, 25, 17, 70, big); }
    { auto o = opts(); o.iters = 1000000; o.check_every = 0; run("no_checks_many_iters", o, 25, 17, 70, big); }
    { auto o = opts(); o.check_every = -1; run("check_every_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved = 1; run("reserved", o, 25, 17, 70, big); }
    { auto o = opts(); o.reserved2 = 1; run("reserved2", o, 25, 17, 70, big); }
    { auto o = opts(); o.loss = 2; run("loss", o, 25, 17, 70, big); }
    { auto o = opts(); o.loss = EVC_LOSS_FROBENIUS; run("loss_l2", o, 25, 17, 70, big); }
    { auto o = opts(); o.init_mode = EVC_INIT_SKLEARN; run("init_sklearn", o, 25, 17, 70, big); }
    { auto o = opts(); o.init_mode = EVC_INIT_GIVEN; run("init_given", o, 25, 17, 70, big); }
    { auto o = opts(); o.stop_rule = EVC_STOP_DECOMP; run("stop_decomp", o, 25, 17, 70, big); }
    { auto o = opts(); o.stop_rule = EVC_STOP_PYMF; run("stop_pymf", o, 25, 17, 70, big); }
    { auto o = opts(); o.stop_rule = EVC_STOP_NONE; run("stop_none", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = -1e-9; run("tol_neg", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = 0.0; run("tol_0", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = __builtin_inf(); run("tol_inf", o, 25, 17, 70, big); }
    { auto o = opts(); o.tol = __builtin_nan(""); run("tol_nan", o, 25, 17, 70, big); }
    { auto o = opts(); o.init_value = __builtin_inf(); run("init_value_inf", o, 25, 17, 70, big); }
    { auto o = opts(); o.dtype = 7; run("dtype", o, 25, 17, 70, big); }
    { auto o = opts(); o.layout = 5; run("layout", o, 25, 17, 70, big); }
    run("M_528", opts(), MUM_MAX_M, 17, 70, big);
    run("M_529", opts(), MUM_MAX_M + 1, 17, 70, big);
    run("M_529_small_ws", opts(), MUM_MAX_M + 1, 17, 70, 16);
    run("N_large", opts(), 25, 1 << 20, 70, big);
    { auto o = opts(); o.tol = -1.0; run("tol_before_limits", o, MUM_MAX_M + 1, 17, 70, 16); }
    { auto o = opts(); o.struct_bytes = 8; run("struct_bytes_before_limits", o, MUM_MAX_M + 1, 17, 70, 16); }
    run("ldm_before_limits", opts(), MUM_MAX_M + 1, 17, 70, 16, nullptr, 1, true, true, 25);
    run("M_0", opts(), 0, 17, 70, big);
    run("N_0", opts(), 25, 0, 70, big);
    run("T_neg", opts(), 25, 17, -1, big);
    run("n_utt_0", opts(), 25, 17, 70, big, nullptr, 0);
}

static void query_lines() {
    const int q[][5] = {{25, 17, 70, 1, EVC_F64}, {MUM_MAX_M, 17, 70, 1, EVC_F32}, {25, 17, 0, 1, EVC_F64},
                        {MUM_MAX_M + 1, 17, 70, 1, EVC_F64}, {0, 17, 70, 1, EVC_F64}, {25, 0, 70, 1, EVC_F64}, {25, 17, -1, 1, EVC_F64},
                        {25, 17, 70, 0, EVC_F64}, {25, 17, 70, 1, 7}};
    const char* names[] = {"ok", "M_528", "T_0", "M_529", "M_0", "N_0", "T_neg", "n_utt_0", "dtype"};
    for (int i = 0; i < 9; ++i) printf("query %s %zu\n", names[i], mum_workspace_bytes(q[i][0], q[i][1], q[i][2], q[i][3], q[i][4]));
}

static void lcarve_line(int M, int R, int T_, int dtype, size_t shift) {
    std::vector<char> mem(4096);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~uintptr_t(255)) + shift;
    const MumLearnWs w = carve_mum_learn(base, M, R, T_, dtype);      // addresses only: nothing is dereferenced
    const char* arr[MUM_LEARN_WS_ARRAYS] = {w.Am, w.Ht, w.Vt, w.Q1t, w.Q2t, w.part, reinterpret_cast<char*>(w.astat),
                                            reinterpret_cast<char*>(w.stat), w.solve_ws};
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const Dims d = make_dims((int)es, M, R, T_, 1);
    const size_t room[MUM_LEARN_WS_ARRAYS] = {
        (size_t)d.Mj * d.Np * es, (size_t)d.Tp * d.Np * es, (size_t)d.Tp * d.Mj * es, (size_t)d.Tp * d.Mj * es, (size_t)d.Tp * d.Mj * es,
        (size_t)LEARN_MAX_SPLITS * 2 * learn_bin_tiles(M) * 16 * d.Np * es, (size_t)R * 8, 8, mum_workspace_bytes(M, R, T_, 1, dtype)};
    printf("lcarve %d %d %d %zu shift %zu :", M, R, T_, es, shift);
    for (int i = 0; i < MUM_LEARN_WS_ARRAYS; ++i) {
        const size_t off = (size_t)(arr[i] - base);
        const size_t end = i < MUM_LEARN_WS_ARRAYS - 1 ? (size_t)(arr[i + 1] - base) : w.bytes;
        if ((reinterpret_cast<uintptr_t>(arr[i]) & 255) != 0 || off + room[i] > end) {
            printf(" BAD");
            exit(5);
        }
        printf(" %zu", off);
    }
    // the activation half carves its own arrays inside its share
    const MumWs in = carve_mum(w.solve_ws, M, R, T_, 1, dtype);
    const size_t need = mum_learn_workspace_bytes(M, R, T_, dtype);
    if (w.bytes > need || in.bytes > w.solve_bytes) {
        printf(" BAD SIZE");
        exit(6);
    }
    printf(" bytes %zu query %zu\n", w.bytes, need);
}

static void largs_lines() {
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
    auto opts = [] {
        evc_mu_masked_learn_opts o{};
        o.struct_bytes = (int)sizeof(o);
        o.dtype = EVC_F64; o.layout = EVC_FRAME_MAJOR; o.loss = EVC_LOSS_FROBENIUS; o.iters = 100; o.check_every = 1; o.tol = 1e-3;
        return o;
    };
    auto run = [&](const char* name, const evc_mu_masked_learn_opts& o, int M, int R, int T, size_t ws, bool with_mask = true,
                   int ldm = -1, int ldw = -1, bool with_w = true) {
        int forced = -1;
        const int st = mum_learn_args_check(p, M, with_mask ? p : nullptr, ldm < 0 ? M : ldm, with_w ? p : nullptr, ldw < 0 ? M : ldw, p,
                                            R, M, R, T, &o, p, ws, &forced);
        printf("largs %s %d %d\n", name, st, forced);
    };
    const size_t big = size_t(1) << 40;
    run("ok", opts(), 25, 8, 48, big);
    run("ok_exact", opts(), 25, 8, 48, mum_learn_workspace_bytes(25, 8, 48, EVC_F64));
    run("short_by_one", opts(), 25, 8, 48, mum_learn_workspace_bytes(25, 8, 48, EVC_F64) - 1);
    run("no_mask", opts(), 25, 8, 48, big, false, 0);
    run("ldm_short", opts(), 25, 8, 48, big, true, 24);
    run("ldw_short", opts(), 25, 8, 48, big, true, -1, 24);
    run("no_w", opts(), 25, 8, 48, big, true, -1, -1, false);
    { auto o = opts(); o.struct_bytes = (int)sizeof(evc_mu_masked_opts); run("struct_bytes", o, 25, 8, 48, big); }
    { auto o = opts(); o.reserved = 7 << 8; run("forced_7", o, 25, 8, 48, big); }
    { auto o = opts(); o.reserved = 65 << 8; run("forced_65", o, 25, 8, 48, big); }
    { auto o = opts(); o.reserved = 1; run("reserved", o, 25, 8, 48, big); }
    { auto o = opts(); o.reserved2 = 1; run("reserved2", o, 25, 8, 48, big); }
    { auto o = opts(); o.loss = 2; run("loss", o, 25, 8, 48, big); }
    { auto o = opts(); o.loss = EVC_LOSS_KL; run("loss_kl", o, 25, 8, 48, big); }
    { auto o = opts(); o.iters = -1; run("iters_neg", o, 25, 8, 48, big); }
    { auto o = opts(); o.iters = 0; run("iters_0", o, 25, 8, 48, big); }
    { auto o = opts(); o.iters = MUM_MAX_SLOTS; run("slots_4098", o, 25, 8, 48, big); }
    { auto o = opts(); o.iters = MUM_MAX_SLOTS; o.check_every = 0; run("no_checks_many_iters", o, 25, 8, 48, big); }
    { auto o = opts(); o.tol = -1e-9; run("tol_neg", o, 25, 8, 48, big); }
    { auto o = opts(); o.tol = __builtin_nan(""); run("tol_nan", o, 25, 8, 48, big); }
    { auto o = opts(); o.tol = 0.0; run("tol_0", o, 25, 8, 48, big); }
    { auto o = opts(); o.dtype = 3; run("dtype", o, 25, 8, 48, big); }
    run("T_0", opts(), 25, 8, 0, big);
    run("M_528", opts(), MUM_MAX_M, 8, 48, big);
    run("M_529", opts(), MUM_MAX_M + 1, 8, 48, 16);
    run("R_4096", opts(), 25, MUM_LEARN_MAX_R, 48, big);
    run("R_4097", opts(), 25, MUM_LEARN_MAX_R + 1, 48, 16);
    { auto o = opts(); o.tol = -1.0; run("tol_before_limits", o, MUM_MAX_M + 1, 8, 48, 16); }
    const int q[][4] = {{25, 8, 48, EVC_F64}, {MUM_MAX_M, MUM_LEARN_MAX_R, 48, EVC_F32}, {MUM_MAX_M + 1, 8, 48, EVC_F64},
                        {25, MUM_LEARN_MAX_R + 1, 48, EVC_F64}, {25, 8, 0, EVC_F64}, {0, 8, 48, EVC_F64}, {25, 0, 48, EVC_F64}, {25, 8, 48, 5}};
    const char* names[] = {"ok", "limits", "M_529", "R_4097", "T_0", "M_0", "R_0", "dtype"};
    for (int i = 0; i < 8; ++i) printf("lquery %s %zu\n", names[i], mum_learn_workspace_bytes(q[i][0], q[i][1], q[i][2], q[i][3]));
}

int main() {
    const int shapes[][4] = {{25, 64, 32, 1}, {40, 130, 33, 2}, {1, 5, 3, 1}, {201, 300, 20, 2}, {528, 16, 17, 1}, {25, 4096, 11008, 16},
                             {25, 17, 0, 1}, {201, 4096, 688, 3}};
    for (const auto& z : shapes)
        for (int dtype : {EVC_F64, EVC_F32})
            for (size_t shift : {size_t(0), size_t(8)}) carve_line(z[0], z[1], z[2], z[3], dtype, shift);
    args_lines();
    query_lines();
    const int ic[][2] = {{0, 0}, {100, 0}, {100, 10}, {99, 10}, {1, 1}, {4096, 1}, {5, 7}};
    for (const auto& c : ic) printf("slots %d %d %d\n", c[0], c[1], mum_slots(c[0], c[1]));
    const int ls[][3] = {{25, 8, 48}, {40, 19, 33}, {201, 12, 70}, {528, 4096, 1}, {1, 1, 1}, {25, 64, 11008}};
    for (const auto& z : ls)
        for (int dtype : {EVC_F64, EVC_F32})
            for (size_t shift : {size_t(0), size_t(8)}) lcarve_line(z[0], z[1], z[2], dtype, shift);
    largs_lines();
    return 0;
}
