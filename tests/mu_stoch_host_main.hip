// mu_stoch_host_main.hip - a program of its own (host code only) that runs what evc_mu_stoch_learn
// (csrc/evc_mu_stoch_plan.h) decides on the host and prints it: tests/test_mu_stoch_host.py builds it, once plainly and once
// under the address and undefined-behaviour sanitizers, and checks the lines.
//   carve <M R T bs method esize> shift <s> : <byte offsets of the 16 arrays in carving order> bytes <b> query <q>
//   args <case> <status>      mus_args_check over a grid of bad and good arguments
//   query <case> <bytes>      mus_workspace_bytes where the call refuses with -1 or -3 (0) and where it does not
//   prev <case> <ok> <bytes>  the size of svrmu's prev+-[n_loop], at and past its limit
//   order <case> <status>     mus_order_check
//   route <R> <route> <r>     mus_route
#include "../exemplars_vc_amd/csrc/evc_mu_stoch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace evc;

static void carve_line(int M, int R, int T_, int bs, int method, int dtype, size_t shift) {
    std::vector<char> mem(4096);
    char* base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(mem.data()) + 255) & ~uintptr_t(255)) + shift;
    const MusWs w = carve_mus(base, M, R, T_, bs, method, dtype);      // addresses only: nothing is dereferenced
    const char* arr[MUS_WS_ARRAYS] = {
        reinterpret_cast<char*>(w.ord), w.HF, w.Xt, w.Mt, w.Am, w.Vt, w.Q1t, w.Q2t, w.part, w.acc, w.prev, w.cand,
        reinterpret_cast<char*>(w.astat), reinterpret_cast<char*>(w.trace), reinterpret_cast<char*>(w.stop), w.solve_ws};
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const Dims d = make_dims((int)es, M, R, bs, 1);
    const size_t n_loop = (size_t)(T_ / bs), RM = (size_t)R * M;
    const size_t room[MUS_WS_ARRAYS] = {
        (size_t)T_ * 4, (size_t)d.Tp * d.Np * es, (size_t)d.Tp * d.Mk * es, (size_t)d.Tp * d.Mk * es, (size_t)d.Mj * d.Np * es,
        (size_t)d.Tp * d.Mj * es, (size_t)d.Tp * d.Mj * es, (size_t)d.Tp * d.Mj * es,
        (size_t)LEARN_MAX_SPLITS * 2 * learn_bin_tiles(M) * 16 * d.Np * es, 2 * RM * es,
        method == EVC_STOCH_SVRMU ? n_loop * 2 * RM * es : 0, RM * es, (size_t)R * 8, n_loop * 8, 4,
        mum_workspace_bytes(M, R, bs, 1, dtype)};
    printf("carve %d %d %d %d %d %zu shift %zu :", M, R, T_, bs, method, es, shift);
    for (int i = 0; i < MUS_WS_ARRAYS; ++i) {
        const size_t off = (size_t)(arr[i] - base);
        const size_t end = i < MUS_WS_ARRAYS - 1 ? (size_t)(arr[i + 1] - base) : w.bytes;
        if ((reinterpret_cast<uintptr_t>(arr[i]) & 255) != 0 || off + room[i] > end) {
            printf(" BAD");
            exit(3);
        }
        printf(" %zu", off);
    }
    // the activation half carves its own arrays inside its share
    const MumWs in = carve_mum(w.solve_ws, M, R, bs, 1, dtype);
    const size_t need = mus_workspace_bytes(M, R, T_, bs, method, dtype);
    if (w.bytes > need || in.bytes > w.solve_bytes) {
        printf(" BAD SIZE");
        exit(4);
    }
    printf(" bytes %zu query %zu\n", w.bytes, need);
}

static void args_lines() {
    const void* p = reinterpret_cast<const void*>(uintptr_t(256));      // never dereferenced
    auto opts = [] {
        evc_mu_stoch_opts o{};
        o.struct_bytes = (int)sizeof(o);
        o.dtype = EVC_F64; o.layout = EVC_FRAME_MAJOR; o.loss = EVC_LOSS_FROBENIUS; o.method = EVC_STOCH_ASAG;
        o.batch_size = 16; o.epochs = 3; o.inner_iters = 1; o.order_rows = 0; o.route = 0;
        o.forget_rate = 0.5; o.alpha = 1.0; o.tol = 1e-3;
        return o;
    };
    std::vector<int> ident(3 * 50), twice(3 * 50), far(3 * 50);
    for (int e = 0; e < 3; ++e)
        for (int t = 0; t < 50; ++t) ident[e * 50 + t] = twice[e * 50 + t] = far[e * 50 + t] = (t + 7 * e) % 50;
    twice[2 * 50 + 49] = twice[2 * 50 + 48];        // the last row names a frame twice
    far[50 + 3] = 50;                               // the second row names a frame that is not there
    auto run = [&](const char* name, const evc_mu_stoch_opts& o, int M, int R, int T, size_t ws, const int* order = nullptr,
                   bool with_mask = true, int ldm = -1, int ldw = -1, bool with_w = true) {
        const int st = mus_args_check(p, M, with_mask ? p : nullptr, ldm < 0 ? M : ldm, with_w ? p : nullptr, ldw < 0 ? M : ldw, p,
                                      R, order, M, R, T, &o, p, ws);
        printf("args %s %d\n", name, st);
    };
    const size_t big = size_t(1) << 44;
    run("ok", opts(), 25, 8, 50, big);
    run("ok_exact", opts(), 25, 8, 50, mus_workspace_bytes(25, 8, 50, 16, EVC_STOCH_ASAG, EVC_F64));
    run("short_by_one", opts(), 25, 8, 50, mus_workspace_bytes(25, 8, 50, 16, EVC_STOCH_ASAG, EVC_F64) - 1);
    run("asag_ws_for_svrmu", [&] { auto o = opts(); o.method = EVC_STOCH_SVRMU; return o; }(), 25, 8, 50,
        mus_workspace_bytes(25, 8, 50, 16, EVC_STOCH_ASAG, EVC_F64));
    run("no_mask", opts(), 25, 8, 50, big, nullptr, false, 0);
    run("ldm_short", opts(), 25, 8, 50, big, nullptr, true, 24);
    run("ldw_short", opts(), 25, 8, 50, big, nullptr, true, -1, 24);
    run("no_w", opts(), 25, 8, 50, big, nullptr, true, -1, -1, false);
    { auto o = opts(); o.struct_bytes = (int)sizeof(evc_mu_masked_learn_opts); run("struct_bytes", o, 25, 8, 50, big); }
    { auto o = opts(); o.reserved = 1; run("reserved", o, 25, 8, 50, big); }
    { auto o = opts(); o.reserved2 = 1; run("reserved2", o, 25, 8, 50, big); }
    { auto o = opts(); o.loss = 2; run("loss", o, 25, 8, 50, big); }
    { auto o = opts(); o.loss = EVC_LOSS_KL; run("loss_kl", o, 25, 8, 50, big); }
    { auto o = opts(); o.method = 4; run("method_4", o, 25, 8, 50, big); }
    { auto o = opts(); o.method = -1; run("method_neg", o, 25, 8, 50, big); }
    { auto o = opts(); o.batch_size = 0; run("bs_0", o, 25, 8, 50, big); }
    { auto o = opts(); o.batch_size = 50; run("bs_T", o, 25, 8, 50, big); }
    { auto o = opts(); o.batch_size = 51; run("bs_T_plus_1", o, 25, 8, 50, big); }
    { auto o = opts(); o.epochs = -1; run("epochs_neg", o, 25, 8, 50, big); }
    { auto o = opts(); o.epochs = 0; run("epochs_0", o, 25, 8, 50, big); }
    { auto o = opts(); o.epochs = 0x7fffffff; o.batch_size = 1; run("steps_overflow", o, 25, 8, 50, big); }
    { auto o = opts(); o.inner_iters = 0; run("inner_0", o, 25, 8, 50, big); }
    { auto o = opts(); o.inner_iters = 2; run("inner_2_asag", o, 25, 8, 50, big); }
    { auto o = opts(); o.inner_iters = 2; o.method = EVC_STOCH_SVRMU; run("inner_2_svrmu", o, 25, 8, 50, big); }
    { auto o = opts(); o.route = 3; run("route_3", o, 25, 8, 50, big); }
    { auto o = opts(); o.route = 1; run("fused_256", o, 25, 256, 50, big); }
    { auto o = opts(); o.route = 1; run("fused_257", o, 25, 257, 50, big); }
    { auto o = opts(); o.route = 2; run("unfused_257", o, 25, 257, 50, big); }
    run("auto_257", opts(), 25, 257, 50, big);
    { auto o = opts(); o.forget_rate = 0.0; run("rho_0", o, 25, 8, 50, big); }
    { auto o = opts(); o.forget_rate = 1.0; run("rho_1", o, 25, 8, 50, big); }
    { auto o = opts(); o.forget_rate = 1.5; run("rho_big", o, 25, 8, 50, big); }
    { auto o = opts(); o.forget_rate = __builtin_nan(""); run("rho_nan", o, 25, 8, 50, big); }
    { auto o = opts(); o.alpha = __builtin_inf(); run("alpha_inf", o, 25, 8, 50, big); }
    { auto o = opts(); o.tol = -1e-9; run("tol_neg", o, 25, 8, 50, big); }
    { auto o = opts(); o.tol = __builtin_nan(""); run("tol_nan", o, 25, 8, 50, big); }
    { auto o = opts(); o.tol = 0.0; run("tol_0", o, 25, 8, 50, big); }
    { auto o = opts(); o.dtype = 3; run("dtype", o, 25, 8, 50, big); }
    { auto o = opts(); o.layout = 5; run("layout", o, 25, 8, 50, big); }
    { auto o = opts(); o.order_rows = 3; run("order_rows_no_order", o, 25, 8, 50, big); }
    { auto o = opts(); o.order_rows = 3; run("order_ok", o, 25, 8, 50, big, ident.data()); }
    { auto o = opts(); o.order_rows = 1; run("order_one_row", o, 25, 8, 50, big, ident.data()); }
    { auto o = opts(); o.order_rows = 2; run("order_rows_2_of_3", o, 25, 8, 50, big, ident.data()); }
    { auto o = opts(); o.order_rows = 0; run("order_rows_0_with_order", o, 25, 8, 50, big, ident.data()); }
    { auto o = opts(); o.order_rows = 3; run("order_twice", o, 25, 8, 50, big, twice.data()); }
    { auto o = opts(); o.order_rows = 1; run("order_twice_row_not_used", o, 25, 8, 50, big, twice.data()); }
    { auto o = opts(); o.order_rows = 3; run("order_far", o, 25, 8, 50, big, far.data()); }
    { auto o = opts(); o.order_rows = 3; run("order_bad_before_limits", o, MUM_MAX_M + 1, 8, 50, 16, far.data()); }
    run("T_0", opts(), 25, 8, 0, big);
    run("M_528", opts(), MUM_MAX_M, 8, 50, big);
    run("M_529", opts(), MUM_MAX_M + 1, 8, 50, 16);
    run("R_4096", opts(), 25, MUS_MAX_R, 50, big);
    run("R_4097", opts(), 25, MUS_MAX_R + 1, 50, 16);
    { auto o = opts(); o.tol = -1.0; run("tol_before_limits", o, MUM_MAX_M + 1, 8, 50, 16); }
    // svrmu's prev+-: 2^31 - 1 frames in batches of 1 at the limits is 2^31 x 2 x 528 x 4096 x 8 bytes
    { auto o = opts(); o.method = EVC_STOCH_SVRMU; o.batch_size = 1; o.epochs = 1; run("prev_too_large", o, MUM_MAX_M, MUS_MAX_R, 0x7fffffff, big); }
    { auto o = opts(); o.batch_size = 1; o.epochs = 1; run("asag_same_sizes", o, 25, 8, 0x7fffffff, ~size_t(0)); }
}

static void query_lines() {
    const int q[][6] = {{25, 8, 50, 16, EVC_STOCH_ASG, EVC_F64}, {MUM_MAX_M, MUS_MAX_R, 50, 16, EVC_STOCH_SVRMU, EVC_F32},
                        {MUM_MAX_M + 1, 8, 50, 16, 0, EVC_F64}, {25, MUS_MAX_R + 1, 50, 16, 0, EVC_F64}, {25, 8, 0, 16, 0, EVC_F64},
                        {0, 8, 50, 16, 0, EVC_F64}, {25, 0, 50, 16, 0, EVC_F64}, {25, 8, 50, 16, 0, 5}, {25, 8, 50, 0, 0, EVC_F64},
                        {25, 8, 50, 51, 0, EVC_F64}, {25, 8, 50, 16, 4, EVC_F64},
                        {MUM_MAX_M, MUS_MAX_R, 0x7fffffff, 1, EVC_STOCH_SVRMU, EVC_F64}};
    const char* names[] = {"ok", "limits", "M_529", "R_4097", "T_0", "M_0", "R_0", "dtype", "bs_0", "bs_T_plus_1", "method_4",
                           "prev_too_large"};
    for (int i = 0; i < 12; ++i)
        printf("query %s %zu\n", names[i], mus_workspace_bytes(q[i][0], q[i][1], q[i][2], q[i][3], q[i][4], q[i][5]));
    size_t b;
    // exactly at the limit: 2^40 / (2 x 512 x 4096 x 8) = 2^15 batches
    bool ok = mus_prev_bytes(512, 4096, 1 << 15, EVC_STOCH_SVRMU, 8, &b);
    printf("prev at_limit %d %zu\n", (int)ok, b);
    ok = mus_prev_bytes(512, 4096, (1 << 15) + 1, EVC_STOCH_SVRMU, 8, &b);
    printf("prev past_limit %d %zu\n", (int)ok, b);
    ok = mus_prev_bytes(528, 4096, 0x7fffffff, EVC_STOCH_SVRMU, 8, &b);
    printf("prev int_max %d %zu\n", (int)ok, b);
    ok = mus_prev_bytes(528, 4096, 0x7fffffff, EVC_STOCH_ASAG, 8, &b);
    printf("prev not_svrmu %d %zu\n", (int)ok, b);
    ok = mus_prev_bytes(25, 8, 3, EVC_STOCH_SVRMU, 4, &b);
    printf("prev small %d %zu\n", (int)ok, b);
}

static void order_lines() {
    const int good[] = {2, 0, 1, 1, 2, 0}, dup[] = {2, 0, 1, 1, 1, 0}, neg[] = {2, 0, -1, 1, 2, 0}, big[] = {2, 0, 1, 1, 3, 0};
    printf("order good %d\n", mus_order_check(good, 2, 3));
    printf("order null %d\n", mus_order_check(nullptr, 2, 3));
    printf("order no_rows %d\n", mus_order_check(dup, 0, 3));
    printf("order dup %d\n", mus_order_check(dup, 2, 3));
    printf("order dup_first_row_only %d\n", mus_order_check(dup, 1, 3));
    printf("order neg %d\n", mus_order_check(neg, 2, 3));
    printf("order big %d\n", mus_order_check(big, 2, 3));
    for (int R : {1, 64, 65, 256, 257, 4096})
        for (int route : {0, 1, 2, 3}) printf("route %d %d %d\n", R, route, mus_route(route, R));
}

int main() {
    const int shapes[][5] = {{25, 8, 50, 16, EVC_STOCH_ASG},   {40, 19, 70, 16, EVC_STOCH_SVRMU}, {1, 3, 5, 2, EVC_STOCH_GSAG},
                             {201, 12, 40, 16, EVC_STOCH_ASAG}, {528, 4096, 33, 1, EVC_STOCH_SVRMU}, {528, 4096, 33, 33, EVC_STOCH_SVRMU},
                             {25, 64, 11008, 256, EVC_STOCH_SVRMU}, {201, 256, 11008, 1024, EVC_STOCH_ASG}};
    for (const auto& z : shapes)
        for (int dtype : {EVC_F64, EVC_F32})
            for (size_t shift : {size_t(0), size_t(8)}) carve_line(z[0], z[1], z[2], z[3], z[4], dtype, shift);
    args_lines();
    query_lines();
    order_lines();
    return 0;
}
