// Which block shape and how many k-splits a contraction of the generic path runs with: the pure host arithmetic of
// gemm_nt / gemm_nt_mu (evc_gemm.hip, k_gemm_nt) and gemm2 / gemm2_mu (evc_gemm2.hip, k_gemm2), kept apart from the
// launches so that it can be printed and pinned without a device (tests/gemm_plan_host_main.hip,
// tests/test_gemm_plan_host.py) and reported per solve (evc_solve_info.variant, include/evc.h).
//
// Inputs are the contraction's sizes (I frames x J rows of R, Kd deep, C's row length ldc), the element size, the CU
// count and the split-K scratch (whether there is one, and how many elements).  No HIP call, no global state.
#pragma once
#include <stddef.h>

namespace evc {

constexpr int GEMM_KS = 16;      // k-slab depth of k_gemm_nt

// what a launcher chose.  shape: k_gemm2's launch_shape case (0 deep-slab 128 x 128 - diagnostic builds only, 1 128 x 128,
// 2 64 x 128, 3 64 x 64 with two slabs in flight); -1 for k_gemm_nt
struct GemmPlan {
    int kernel;      // 1: k_gemm_nt, 2: k_gemm2 (EVC_KERNEL_GEMM_NT / EVC_KERNEL_GEMM2); 0: nothing was launched
    int bf, br;      // block: frames x rows of R
    int shape;
    int splits;      // k-ranges (blockIdx.z); 1: no split
};

// evc_solve_info.variant of the generic path: 4-bit block codes and the split count of V = H Am^T
//   bits 0..3 update contraction, bits 4..7 V = H Am^T (0: not formed in the loop - GRAM, LITERAL), bits 8..13 its split
//   count, bits 16..19 numerator P = X A (0: none - KL)
enum { GEMM_BLK_NONE = 0, GEMM_BLK_64x64 = 1, GEMM_BLK_64x128 = 2, GEMM_BLK_128x64 = 3, GEMM_BLK_128x128 = 4,
       GEMM_BLK_128x128_DEEP = 5 };

inline int gemm_block_code(const GemmPlan& p) {
    if (p.kernel == 0) return GEMM_BLK_NONE;
    if (p.kernel == 2 && p.shape == 0) return GEMM_BLK_128x128_DEEP;
    if (p.bf == 64) return p.br == 64 ? GEMM_BLK_64x64 : GEMM_BLK_64x128;
    return p.br == 64 ? GEMM_BLK_128x64 : GEMM_BLK_128x128;
}

inline int gemm_variant(const GemmPlan& update, const GemmPlan& v, const GemmPlan& p) {
    return gemm_block_code(update) | (gemm_block_code(v) << 4) | ((v.kernel ? v.splits & 63 : 0) << 8) |
           (gemm_block_code(p) << 16);
}

// Which generation of the contraction kernel serves an element size: k_gemm2 for float32 (77 against 65 Tflop/s on the
// STFT flow); float64 stays on k_gemm_nt, which k_gemm2 does not beat (its 64-cycle MFMAs hide what k_gemm2
// removes).  Diagnostic builds (-DEVC_DIAG_GEMM_V1 / -DEVC_DIAG_GEMM2_F64) force one or the other for A/B timing;
// the shipped library reads nothing from the environment.
inline bool plan_use_gemm2(int esize) {
#if defined(EVC_DIAG_GEMM_V1)
    (void)esize;
    return false;
#elif defined(EVC_DIAG_GEMM2_F64)
    (void)esize;
    return true;
#else
    return esize == 4;
#endif
}

// ---------------------------------------------------------------------------------------------------------------------
// k_gemm_nt, plain product
// ---------------------------------------------------------------------------------------------------------------------
// few output tiles (one utterance): 64x64 tiles put 2-4x more workgroups on the 256 CUs, and a long
// contraction is additionally split over blockIdx.z into slabs of partial products (summed in order)
inline bool plan_nt_few_tiles(int I, int J) { return (long)((I + 127) / 128) * (J / 64) < 256; }

// the split rule reads the CU count only here (the launcher asks the device only then)
inline bool plan_nt_wants_cus(int I, int J, int ldc, bool have_scratch) {
    return plan_nt_few_tiles(I, J) && have_scratch && ldc == J;
}

inline GemmPlan plan_gemm_nt(int I, int J, int Kd, int ldc, int n_cus, bool have_scratch, size_t scratch_elems) {
    GemmPlan pl{1, 64, 64, -1, 1};
    const long blocks = (long)(I / 64) * (J / 64);
    if (plan_nt_few_tiles(I, J)) {
        int splits = 1;
        const long slab = (long)I * ldc;
        if (have_scratch && ldc == J) {
            // The split (<= 8, not necessarily a divisor of the k-slabs) that is expected to finish first: a CU works
            // on up to four of these workgroups at once, one wavefront of each per SIMD, so a launch lasts about
            // (most workgroups on one CU) x (one workgroup's work ~ 1 / split), a little longer when few workgroups
            // share a CU (their latencies are less well covered: 0.6 / 0.8 / 0.9 / 0.95 of the matrix rate for 1..4).
            // C3's V = H Am^T (99 tiles): 7 ranges put at most 3 workgroups on a CU where 8 put 4 on some.  Every
            // workgroup keeps a worthwhile chunk (512 deep for long contractions, 64 for short ones such as the
            // 400-point DFTs of Griffin-Lim, whose 84 tiles would otherwise run 25 slabs each on a third of the CUs).
            const int cus = n_cus > 0 ? n_cus : 256;
            static const double eff[5] = {1.0, 0.6, 0.8, 0.9, 0.95};
            const int nslabs = Kd / GEMM_KS, chunk = Kd >= 1024 ? 512 : 64;
            double best = 1e30;
            for (int sp = 1; sp <= 8 && Kd >= 1024; ++sp) {
                if (blocks * sp > 4L * cus || (sp > 1 && (nslabs / sp) * GEMM_KS < chunk) || (size_t)sp * slab > scratch_elems) continue;
                const long per_cu = (blocks * sp + cus - 1) / cus;
                const double cost = (double)per_cu / sp / eff[per_cu];
                if (cost < best - 1e-9) { best = cost; splits = sp; }
            }
            // short contractions (measured on Griffin-Lim's: 12.7 ms per 300 iterations with the rule above against
            // 11.2): the largest split that divides the k-slabs evenly
            for (int sp = 2; sp <= 8 && Kd < 1024; ++sp)
                if (nslabs % sp == 0 && blocks * sp <= 1024 && Kd / sp >= chunk && (size_t)sp * slab <= scratch_elems)
                    splits = sp;
        }
        pl.splits = splits;
        return pl;
    }
    if (I % 128) {      // short batches are padded to 64 frames only: 64-row blocks
        if (J % 128 == 0) pl.br = 128;
        return pl;
    }
    pl.bf = 128;
    if (J % 128 == 0) pl.br = 128;
    return pl;
}

// k_gemm_nt with the multiplicative update as epilogue (J % 128 == 0)
// Tile quantisation for one or two utterances: 128x128 tiles run in rounds of 256 (one per CU), 64x128
// tiles in rounds of 512 (two per CU, half the work each; a trailing all-padding row tile leaves at
// once).  C3 (768 x 8192): 384 full tiles = 2 rounds against 768 half tiles = 2 half rounds.
inline GemmPlan plan_gemm_nt_mu(int I, int J) {
    const long b128 = (long)((I + 127) / 128) * (J / 128), b64 = (long)(I / 64) * (J / 128);
    const long t128 = 2 * ((b128 + 255) / 256), t64 = (b64 + 511) / 512;     // in half-tile rounds
    if (I % 128 || (I <= 2048 && t64 < t128)) return GemmPlan{1, 64, 128, -1, 1};
    return GemmPlan{1, 128, 128, -1, 1};
}

// ---------------------------------------------------------------------------------------------------------------------
// k_gemm2
// ---------------------------------------------------------------------------------------------------------------------
inline GemmPlan gemm2_shape_plan(int shape, int splits) {
    return GemmPlan{2, shape <= 1 ? 128 : 64, shape == 3 ? 64 : 128, shape, splits};
}

inline double plan_round_eff(long wg, long slots) { return (double)wg / (double)(((wg + slots - 1) / slots) * slots); }

// C = L R^T.  With scratch (and ldc == J) a short grid is split over k into slabs.  (The element size does not enter: the
// shapes hold the same number of workgroups per CU for both.)
inline GemmPlan plan_gemm2(int I, int J, int Kd, int ldc, int n_cus, bool have_scratch, size_t scratch_elems) {
    if (n_cus <= 0) n_cus = 256;
    // 64 x 128 blocks (three per CU) when R has a multiple of 128 rows and the grid fills the CUs; 64 x 64 blocks
    // (four per CU) otherwise: a grid of less than one round runs as long as ONE workgroup does, so the smallest
    // tile is the fastest
#ifdef EVC_G2_PLAIN_SHAPE      // diagnostic builds: force a block shape of the plain product (0 / 1: 128 x 128)
    const bool wide = EVC_G2_PLAIN_SHAPE != 3;
    const int shape = EVC_G2_PLAIN_SHAPE;
    const long blocks = shape <= 1 ? (long)(I / 128) * (J / 128) : (long)(I / 64) * (J / (wide ? 128 : 64));
    const long slots = (long)n_cus * (shape == 0 ? 1 : (shape == 1 ? 2 : (wide ? 3 : 4)));
#else
    const bool wide = J % 128 == 0 && (long)(I / 64) * (J / 128) >= 3L * n_cus;
    const int shape = wide ? 2 : 3;
    const long blocks = (long)(I / 64) * (J / (wide ? 128 : 64));
    // (48 KiB of LDS hold three workgroups per CU for either shape; counting four for the narrow one makes the rule
    // split a little earlier, which measured better: STFT flow, 16 utterances, 157.8 against 155.5 kframes/s)
    const long slots = (long)n_cus * (wide ? 3 : 4);
#endif
    // split-K so that the grid fills the CUs' workgroup slots in whole rounds: the smallest split whose rounds
    // are >= 85 % full (each workgroup keeps >= 128 of k)
    int splits = 1;
    const long slab = (long)I * ldc;
    if (have_scratch && ldc == J) {
        double best = plan_round_eff(blocks, slots);
        for (int sp = 2; sp <= 32 && best < 0.85; ++sp) {
            if (Kd % (sp * 16) || Kd / sp < 128 || (size_t)sp * slab > scratch_elems) continue;
            const double eff = plan_round_eff(blocks * sp, slots);
            if (eff > best + 0.03) { best = eff; splits = sp; }
        }
    }
    return gemm2_shape_plan(shape, splits);
}

// the same contraction with the multiplicative update as epilogue
// The epilogue moves 3 elements per output against 2 Kd flops: for short contractions (Kd of a few hundred) it is as
// long as the main loop, so several workgroups share a CU and one's epilogue runs beside the others' MFMAs.
// float32: 128 x 128 blocks, two per CU, when there are enough of them for whole rounds; else (and float64,
// whose accumulators need the registers) 64 x 128 blocks, three per CU.
// A grid of less than one round of 64 x 128 blocks takes the 64 x 64 shape (four per CU): it then runs as long
// as one small workgroup does.
inline GemmPlan plan_gemm2_mu(int I, int J, int esize, int n_cus) {
    if (n_cus <= 0) n_cus = 256;
    const long b128 = (long)(I / 128) * (J / 128), b64 = (long)(I / 64) * (J / 128);
#ifdef EVC_G2_MU_SHAPE
    const int shape = EVC_G2_MU_SHAPE;       // diagnostic builds: force a block shape
    (void)b128; (void)b64; (void)esize;
#else
    const int shape = (esize == 4 && I % 128 == 0 && b128 >= 8L * n_cus) ? 1 : (b64 >= 3L * n_cus ? 2 : 3);
#endif
    return gemm2_shape_plan(shape, 1);
}

}  // namespace evc
