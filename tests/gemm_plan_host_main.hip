// Prints which block shape and split count the generic path's contractions run with (csrc/evc_gemm_plan.h), one record per
// line over a fixed grid of I, J, Kd, element size, CU count (64, 256, 304) and split-K scratch (none, 2 / 4 / 32 slabs, and
// 32 slabs behind a row length that is not J), for tests/test_gemm_plan_host.py and tools/make_golden_gemm_plan.py.  Host
// code only: built with the host half of hipcc, no HIP call, no library, no arguments.
//
//   nt   I J Kd ldc n_cus have_scratch scratch_elems : bf br splits        gemm_nt    -> k_gemm_nt<bf, br, ., ., false>
//   ntmu I J : bf br                                                        gemm_nt_mu -> k_gemm_nt<bf, br, ., ., true>
//   g2   I J Kd ldc n_cus have_scratch scratch_elems : shape bf br splits   gemm2      -> launch_shape<., false>(shape)
//   g2mu esize I J n_cus : shape bf br                                      gemm2_mu   -> launch_shape<., true>(shape)
//   use2 esize : 0 | 1                                                      which kernel serves an element size
//
// -DGEMM_PLAN_PARENT: the build that recorded tests/golden/gemm_plan.json: the conditions as they stood inside gemm_nt,
// gemm_nt_mu (csrc/evc_gemm.hip) and gemm2, gemm2_mu (csrc/evc_gemm2.hip) on the commit before the header existed, copied
// literally (the device's CU count, which they asked the runtime for, is the parameter n_cus here; launches are replaced by
// the template arguments they named).
#include <stddef.h>
#include <stdio.h>

#ifndef GEMM_PLAN_PARENT
#include "../exemplars_vc_amd/csrc/evc_gemm_plan.h"
using namespace evc;
#else
namespace {
struct GemmPlan { int kernel, bf, br, shape, splits; };
constexpr int KS = 16;

bool plan_use_gemm2(int esize) { return esize == 4; }      // use_gemm2<T>(): sizeof(T) == 4 in the shipped build

// ---- gemm_nt, evc_gemm.hip:249-301 (the part behind the k_gemm2 hand-over) ----
GemmPlan plan_gemm_nt(int I, int J, int Kd, int ldc, int n_cus, bool scratch, size_t scratch_elems) {
    const long blocks = (long)(I / 64) * (J / 64);
    if ((long)((I + 127) / 128) * (J / 64) < 256) {
        int splits = 1;
        const long slab = (long)I * ldc;
        if (scratch && ldc == J) {
            int cus = n_cus;
            if (cus <= 0) cus = 256;
            static const double eff[5] = {1.0, 0.6, 0.8, 0.9, 0.95};
            const int nslabs = Kd / KS, chunk = Kd >= 1024 ? 512 : 64;
            double best = 1e30;
            for (int sp = 1; sp <= 8 && Kd >= 1024; ++sp) {
                if (blocks * sp > 4L * cus || (sp > 1 && (nslabs / sp) * KS < chunk) || (size_t)sp * slab > scratch_elems) continue;
                const long per_cu = (blocks * sp + cus - 1) / cus;
                const double cost = (double)per_cu / sp / eff[per_cu];
                if (cost < best - 1e-9) { best = cost; splits = sp; }
            }
            for (int sp = 2; sp <= 8 && Kd < 1024; ++sp)
                if (nslabs % sp == 0 && blocks * sp <= 1024 && Kd / sp >= chunk && (size_t)sp * slab <= scratch_elems)
                    splits = sp;
        }
        return GemmPlan{1, 64, 64, -1, splits};                  // launch_nt<T, 64, 64, 32, 32, false>(..., splits, ...)
    }
    if (I % 128) {
        if (J % 128 == 0) return GemmPlan{1, 64, 128, -1, 1};    // launch_nt<T, 64, 128, 32, 32, false>
        return GemmPlan{1, 64, 64, -1, 1};                       // launch_nt<T, 64, 64, 32, 32, false>
    }
    if (J % 128 == 0) return GemmPlan{1, 128, 128, -1, 1};       // launch_nt<T, 128, 128, 64, 32, false>
    return GemmPlan{1, 128, 64, -1, 1};                          // launch_nt<T, 128, 64, 32, 32, false>
}

// ---- gemm_nt_mu, evc_gemm.hip:315-319 ----
GemmPlan plan_gemm_nt_mu(int I, int J) {
    const long b128 = (long)((I + 127) / 128) * (J / 128), b64 = (long)(I / 64) * (J / 128);
    const long t128 = 2 * ((b128 + 255) / 256), t64 = (b64 + 511) / 512;
    if (I % 128 || (I <= 2048 && t64 < t128))
        return GemmPlan{1, 64, 128, -1, 1};                      // launch_nt<T, 64, 128, 32, 32, true>
    return GemmPlan{1, 128, 128, -1, 1};                         // launch_nt<T, 128, 128, 64, 32, true>
}

// ---- launch_shape, evc_gemm2.hip:396-401: the block of each case ----
GemmPlan shape_plan(int shape, int splits) {
    switch (shape) {
        case 0: return GemmPlan{2, 128, 128, 0, splits};         // launch2<T, 128, 128, 32, 64, G2K<T>::BIG, ...>
        case 1: return GemmPlan{2, 128, 128, 1, splits};         // launch2<T, 128, 128, 32, 64, G2K<T>::SMALL, ...>
        case 2: return GemmPlan{2, 64, 128, 2, splits};          // launch2<T, 64, 128, 32, 64, G2K<T>::SMALL, ...>
        default: return GemmPlan{2, 64, 64, 3, splits};          // launch2<T, 64, 64, 32, 32, G2K<T>::SMALL, MU, 3, 2>
    }
}

double round_eff(long wg, long slots) { return (double)wg / (double)(((wg + slots - 1) / slots) * slots); }

// ---- gemm2, evc_gemm2.hip:413-443 ----
GemmPlan plan_gemm2(int I, int J, int Kd, int ldc, int n_cus, bool scratch, size_t scratch_elems) {
    if (n_cus <= 0) n_cus = 256;
    const bool wide = J % 128 == 0 && (long)(I / 64) * (J / 128) >= 3L * n_cus;
    const int shape = wide ? 2 : 3;
    const long blocks = (long)(I / 64) * (J / (wide ? 128 : 64));
    const long slots = (long)n_cus * (wide ? 3 : 4);
    int splits = 1;
    const long slab = (long)I * ldc;
    if (scratch && ldc == J) {
        double best = round_eff(blocks, slots);
        for (int sp = 2; sp <= 32 && best < 0.85; ++sp) {
            if (Kd % (sp * 16) || Kd / sp < 128 || (size_t)sp * slab > scratch_elems) continue;
            const double eff = round_eff(blocks * sp, slots);
            if (eff > best + 0.03) { best = eff; splits = sp; }
        }
    }
    return shape_plan(shape, splits);
}

// ---- gemm2_mu, evc_gemm2.hip:462-473 ----
GemmPlan plan_gemm2_mu(int I, int J, int esize, int n_cus) {
    if (n_cus <= 0) n_cus = 256;
    const long b128 = (long)(I / 128) * (J / 128), b64 = (long)(I / 64) * (J / 128);
    const int shape = (esize == 4 && I % 128 == 0 && b128 >= 8L * n_cus) ? 1 : (b64 >= 3L * n_cus ? 2 : 3);
    return shape_plan(shape, 1);
}
}  // namespace
#endif

static const int IS[] = {64, 128, 192, 704, 768, 1984, 2048, 2176, 3072, 8192, 11008, 24576, 70016};
static const int JS[] = {64, 128, 192, 256, 320, 512, 896, 1024, 1088, 2048, 4096, 8192};
static const int KDS[] = {16, 48, 112, 128, 208, 256, 384, 400, 512, 896, 1008, 1024, 1536, 4096, 8192};
static const int CUS[] = {64, 256, 304};
// split-K scratch: none; 2, 4, 32 slabs of I x J; 32 slabs behind a row length of J + 128 (the rules then do not split)
enum { SC_NONE, SC_2, SC_4, SC_32, SC_LDC, N_SCRATCH };
// the contractions of tests/test_gpu_gemm_steps.py's cases on 256 CUs (frames, rows, depth), printed under every CU count
static const int CASES[][3] = {
    {1984, 1024, 48}, {1984, 64, 1024}, {2176, 1024, 48}, {2176, 64, 1024}, {2176, 1024, 1024}, {11008, 192, 128},
    {1984, 1088, 128}, {128, 128, 48}, {128, 64, 128}, {128, 64, 256}, {128, 64, 384}, {128, 64, 512}, {128, 64, 896},
    {128, 256, 32}, {128, 64, 256}, {128, 128, 256}, {128, 192, 256}, {3072, 2048, 48}, {3072, 64, 2048},
    {3072, 2048, 2048}, {8192, 4096, 48}, {8192, 64, 4096}, {24576, 256, 128}, {24576, 128, 208}, {192, 384, 48},
    {192, 64, 384}, {3072, 2048, 208}, {3072, 256, 2048}};

// which way through each rule a record went, restated from its inputs and result
enum { NT_FEW_NO_SCRATCH, NT_FEW_LDC, NT_FEW_COST_1, NT_FEW_COST_N, NT_FEW_DIV_1, NT_FEW_DIV_N, NT_64x128, NT_64x64_LARGE,
       NT_128x128, NT_128x64, NTMU_64_ODD, NTMU_64_ROUNDS, NTMU_128,
       G2_WIDE, G2_NARROW_J, G2_NARROW_SMALL, G2_NO_SCRATCH, G2_FULL, G2_SPLIT, G2_NO_BETTER,
       G2MU_1, G2MU_2, G2MU_2_NOT_1, G2MU_3, N_BRANCHES };
static const char* const BRANCH_NAMES[N_BRANCHES] = {
    "nt.few.no_scratch", "nt.few.ldc", "nt.few.cost_model.1", "nt.few.cost_model.split", "nt.few.divisor.1",
    "nt.few.divisor.split", "nt.64x128", "nt.64x64.large", "nt.128x128", "nt.128x64",
    "ntmu.64x128.odd_frames", "ntmu.64x128.rounds", "ntmu.128x128",
    "g2.wide", "g2.narrow.rows", "g2.narrow.small_grid", "g2.no_scratch", "g2.full_rounds", "g2.split", "g2.no_better_split",
    "g2mu.1", "g2mu.2", "g2mu.2.not_1", "g2mu.3"};
static long g_branch[N_BRANCHES];

static size_t scratch_of(int mode, int I, int J) {
    const size_t slab = (size_t)I * J;
    return mode == SC_NONE ? 0 : mode == SC_2 ? 2 * slab : mode == SC_4 ? 4 * slab : 32 * slab;
}

static void nt_line(int I, int J, int Kd, int n_cus, int mode) {
    const int ldc = mode == SC_LDC ? J + 128 : J;
    const size_t se = scratch_of(mode, I, J);
    const GemmPlan p = plan_gemm_nt(I, J, Kd, ldc, n_cus, mode != SC_NONE, se);
    printf("nt %d %d %d %d %d %d %zu : %d %d %d\n", I, J, Kd, ldc, n_cus, (int)(mode != SC_NONE), se, p.bf, p.br, p.splits);
    if ((long)((I + 127) / 128) * (J / 64) < 256) {
        if (mode == SC_NONE) ++g_branch[NT_FEW_NO_SCRATCH];
        else if (mode == SC_LDC) ++g_branch[NT_FEW_LDC];
        else if (Kd >= 1024) ++g_branch[p.splits > 1 ? NT_FEW_COST_N : NT_FEW_COST_1];
        else ++g_branch[p.splits > 1 ? NT_FEW_DIV_N : NT_FEW_DIV_1];
    } else if (I % 128) {
        ++g_branch[J % 128 == 0 ? NT_64x128 : NT_64x64_LARGE];
    } else {
        ++g_branch[J % 128 == 0 ? NT_128x128 : NT_128x64];
    }
}

static void ntmu_line(int I, int J) {
    const GemmPlan p = plan_gemm_nt_mu(I, J);
    printf("ntmu %d %d : %d %d\n", I, J, p.bf, p.br);
    if (I % 128) ++g_branch[NTMU_64_ODD];
    else if (p.bf == 64) ++g_branch[NTMU_64_ROUNDS];
    else ++g_branch[NTMU_128];      // (I > 2048 always: with I % 128 == 0, b64 = 2 b128 and t64 = ceil(b128 / 256) < t128)
}

static void g2_line(int I, int J, int Kd, int n_cus, int mode) {
    const int ldc = mode == SC_LDC ? J + 128 : J;
    const size_t se = scratch_of(mode, I, J);
    const GemmPlan p = plan_gemm2(I, J, Kd, ldc, n_cus, mode != SC_NONE, se);
    printf("g2 %d %d %d %d %d %d %zu : %d %d %d %d\n", I, J, Kd, ldc, n_cus, (int)(mode != SC_NONE), se, p.shape, p.bf, p.br,
           p.splits);
    const int cus = n_cus > 0 ? n_cus : 256;
    if (p.shape == 2) ++g_branch[G2_WIDE];
    else ++g_branch[J % 128 ? G2_NARROW_J : G2_NARROW_SMALL];
    const long blocks = (long)(I / 64) * (J / (p.shape == 2 ? 128 : 64)), slots = (long)cus * (p.shape == 2 ? 3 : 4);
    const double full = (double)blocks / (double)(((blocks + slots - 1) / slots) * slots);
    if (mode == SC_NONE || mode == SC_LDC) ++g_branch[G2_NO_SCRATCH];
    else if (full >= 0.85) ++g_branch[G2_FULL];
    else ++g_branch[p.splits > 1 ? G2_SPLIT : G2_NO_BETTER];
}

static void g2mu_line(int esize, int I, int J, int n_cus) {
    const GemmPlan p = plan_gemm2_mu(I, J, esize, n_cus);
    printf("g2mu %d %d %d %d : %d %d %d\n", esize, I, J, n_cus, p.shape, p.bf, p.br);
    const bool enough = (long)(I / 128) * (J / 128) >= 8L * (n_cus > 0 ? n_cus : 256);
    if (p.shape == 1) ++g_branch[G2MU_1];
    else if (p.shape == 2) ++g_branch[enough ? G2MU_2_NOT_1 : G2MU_2];
    else ++g_branch[G2MU_3];
}

int main() {
    puts("# nt I J Kd ldc n_cus have_scratch scratch_elems : bf br splits");
    puts("# g2 I J Kd ldc n_cus have_scratch scratch_elems : shape bf br splits");
    // the whole product, thinned by a prime stride: every dimension keeps every value, paired differently each time round
    long k = 0;
    for (int I : IS) for (int J : JS) for (int Kd : KDS) for (int n_cus : CUS) for (int mode = 0; mode < N_SCRATCH; ++mode)
        if (k++ % 53 == 0) {
            nt_line(I, J, Kd, n_cus, mode);
            g2_line(I, J, Kd, n_cus, mode);
        }
    for (const auto& c : CASES) for (int n_cus : CUS) for (int mode = SC_NONE; mode <= SC_32; mode += SC_32) {
        nt_line(c[0], c[1], c[2], n_cus, mode);
        g2_line(c[0], c[1], c[2], n_cus, mode);
    }
    // an unknown CU count (the query failed) counts as 256
    nt_line(128, 64, 2048, 0, SC_32);
    g2_line(128, 64, 2048, 0, SC_32);
    puts("# ntmu I J : bf br");
    puts("# g2mu esize I J n_cus : shape bf br");
    for (int I : IS) for (int J : JS) {
        if (J % 128) continue;      // the update's rows are the exemplars, padded to 128
        ntmu_line(I, J);
        for (int esize = 4; esize <= 8; esize += 4) for (int n_cus : CUS) g2mu_line(esize, I, J, n_cus);
    }
    g2mu_line(4, 8192, 4096, 0);
    puts("# use2 esize : k_gemm2 serves it");
    for (int esize = 4; esize <= 8; esize += 4) printf("use2 %d : %d\n", esize, (int)plan_use_gemm2(esize));
    for (int b = 0; b < N_BRANCHES; ++b) printf("branch %s %ld\n", BRANCH_NAMES[b], g_branch[b]);
    return 0;
}
