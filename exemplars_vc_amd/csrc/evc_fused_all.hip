// All-resident variant of the fused FACTORED kernel (float64, M <= 32): nothing streams.
//
// k_fused_res keeps half of a 16-frame block's activations in registers and recomputes the numerator
// tiles P = A_j^T X in every iteration (7 of the 22 MFMAs of a unit at M = 25), because one workgroup
// owns all N exemplars of its frames: at N = 4096 that is 512 KiB of H plus 512 KiB of P per 16 frames,
// more than a CU holds.  Here a frame tile is shared by C "members" (a group), each owning 32 exemplar
// tiles (512 exemplars): 4 wavefronts x 8 tiles, whose activations AND numerators stay in VGPRs (128 of
// the 256 registers of a wavefront) for all iterations of a frame tile.  A unit is then 15 MFMAs
// (D = A_j^T V: 7, V' += A_j H'_j: 8) instead of 20.5 on average, and the only memory traffic of the loop
// is the dictionary fragments (LDS where the member's dictionary fits, see AllShape; L2 otherwise) and the
// exchange of the partial V' between the members of a group.
//
// The exchange costs a memory round trip per iteration (measured 3.5 us against a 3.8 us sweep), so it has
// to hide behind matrix work of ANOTHER frame tile.  Two free-running 4-wavefront workgroups per CU do not
// do that: coupled through their peers they fall into lock step - both sweep together (sharing the matrix
// pipes), then both wait together (measured: 10.9 us per iteration, 7.3 + 3.5).  So one workgroup of 8
// wavefronts holds TWO members, of two different groups: wavefronts 0-3 ("half" 0) and 4-7 (half 1; wave
// w and w + 4 share a SIMD).  They alternate by construction: in every step one half sweeps while the other
// exchanges, and a workgroup barrier closes the step, so a SIMD's matrix pipe always belongs to exactly one
// wavefront and the exchange of one frame tile always runs beside the sweep of the other.
//
//   step      0        1        2        3      ...   2K-1      2K
//   half 0  sweep 0   exch    sweep 1   exch    ...   exch       -
//   half 1    -      sweep 0   exch    sweep 1  ...  sweep K-1  exch
//
// The grid is persistent: one workgroup per CU, G = 2 floor(#CUs / C) groups walk the frame tiles g, g + G,
// ... (all members of a group walk the same list in lock step), so every member of every group is resident
// for the whole launch whatever the batch size.
//
// Every exchange: after the sweep the half's wavefronts leave their partial V' in LDS; the exchanging threads sum
// their elements over the 4 wavefronts in fixed order and publish them with agent-scope stores (sc1: past the
// non-coherent per-XCD L2s); the lowest mantissa bit of a word is the epoch of the buffer, so data and arrival travel
// in one word.  Two buffers alternate by exchange parity (a member overwrites a buffer two exchanges later, after it
// has read every peer's words of the exchange in between, which the peer published after reading this member's words
// of the exchange before).  Every member sums in the same order: all obtain the bitwise identical V'.  Every wait is
// bounded (all_polls_out); a member that gives up raises coop_abort, everybody leaves, and the host redoes the solve
// without inter-workgroup communication (solve_checked, evc_api.hip).
//
// Which exchange (pick_c; template C > 0: that many members, C <= 0: member count at run time):
//   direct (C = 2, 4, 8; 8 only where the dictionary is in LDS): every member fetches every peer's partial,
//     16-byte words, one memory round trip.  Each wavefront first watches one word per peer, so that the bulk fetch
//     normally succeeds at once.  k_fused_all and k_fused_lone skip the load of the member's own slot and take that pair
//     from registers; k_fused_quad loads all C slots, its own included (a word it stored earlier in the same exchange:
//     stale, it carries the other epoch and is fetched again like a peer's) - eight loads for seven, and in exchange no
//     slot is zeroed or copied first, nothing branches on the member index, and the tag test is one chain per value of
//     the wave-uniform epoch: 75 vector instructions per exchange at 8 members instead of 138, beside the other half's
//     sweep on the same SIMDs (DESIGN.md 5.1a cont., profiles/lean_exchange_README.md).
//   reduce-scatter, whole slices (C == 0: 8 members at M 26 .. 28, and 16, 32, 64): fetching every peer's partial
//     would cost (C - 1) x 3.5 KB per member and exchange, so member m sums slice m of all partials and publishes it,
//     and everybody fetches the summed slices: two memory round trips, 7 KB fetched per member whatever C is.  Whole
//     slices: C divides the NE elements.
//   reduce-scatter, ragged slices (C == -1: 3, 5, 6, 7 and 9 .. 128 members otherwise): the same with ragged slices of
//     ceil(NE / C) elements, the last ones short or empty.
// Measured at N = 16384 (C5): 5.8 us per step against 5.2 us at N = 4096, where the sweep is the longer half.
//
// Requirements (the host checks them, fused_all_members): guarded eps mode, fast quotients, Frobenius or KL loss, NT a
// multiple of 32 (fused_layout pads N to whole members when that costs <= 12.5 %), at most 128 members.  Frame
// tiles whose frames are not all live are left to the general kernel (skip_all_live), like in k_fused_res.
#include "evc_fused_common.h"

namespace evc {

constexpr int AW = 4;                  // wavefronts per half
constexpr int AKT = 8;                 // exemplar tiles per wavefront, all register-resident
constexpr int ATILES = AW * AKT;       // exemplar tiles per member
constexpr int ATHREADS = 2 * AW * 64;  // two halves per workgroup
constexpr unsigned ALL_POLL_LIMIT = 1u << 17;
constexpr int ALL_STAGGER_PER_ITER = 11000;    // shader cycles of one iteration of one half (two steps) / 2: launch_all
// Priority of a wavefront while it exchanges.  The exchange is a chain of a few dozen dependent instructions (LDS,
// stores, polls) on a SIMD whose other wavefront issues MFMAs and vector work back to back; at equal priority the older
// wavefront wins the issue arbitration, so half 1's exchange (wavefronts 4-7) took 12.8 k cycles where half 0's took
// 10.4 k (profiles/r04_fused_all_stamps_prio_and_11_tiles.txt).  The exchanging wavefront goes first: its instructions
// are few, the sweep beside it does not notice.  Both exchanges then take 10.9 k and a C2 step 11.8 k cycles, not 12.6 k.
constexpr int ALL_EXCH_PRIO = 3;
typedef unsigned all_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned all_u32x4 __attribute__((ext_vector_type(4)));
typedef long long all_i64x2 __attribute__((ext_vector_type(2)));

// The one bounded wait: has this poll loop run out?  After ALL_POLL_LIMIT polls, or when somebody raised coop_abort
// (looked at every 64th poll).
__device__ __forceinline__ bool all_polls_out(unsigned& polls, const int* coop_abort) {
    return ++polls > ALL_POLL_LIMIT ||
           ((polls & 63) == 0 && __hip_atomic_load(coop_abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0);
}

// Round 5: the member's dictionary in LDS.  Both halves of a workgroup are the same member and read the same 32 exemplar
// tiles in every step, for the whole launch; streamed from L2 (8 x 16-byte loads per unit and wavefront) the fragments
// queue in the CU's memory pipe in front of the exchange's stores and polls.  Where it fits, one copy is filled once per
// launch from A2p and both operand orders are read from it with ds_read_b64 - no vector-memory instruction in the sweep.
//
// Layout (doubles): slot w * AKT + k holds tile w + AW k of the member (a wavefront's 8 tiles lie within 64 KiB: the tile
// and the k-step ride in the instruction's immediate), 16 rows of PR per tile, row rho(e) holding exemplar e of the tile,
// bins 0 .. M-1 then zeros.  PR = 2 mod 4 and rho(4q + r) = 4 sigma(q) + r (sigma swaps 1 and 2) make both read patterns
// conflict-free (ds_read_b64: two groups of 32 lanes, bank = dword address mod 64):
//   D and P  (lane: exemplar 4 (l&3) + (l&15)/4 as in A1p, bin = k-step base + l/16): the 16 row starts of a tile are
//            distinct even numbers mod 32, the two bins of a 32-lane group add 0 or 1;
//   V'       (lane: bin l&15, exemplar 4 (l/16) + r): the rows of lane groups q and q + 1 start 16 apart mod 32.
// Bins past M (the last k-step's upper lane groups, the last bin tile's upper lanes) read the zero slot M of their own row
// (PR > M): same address within a row, a broadcast.  The values equal A1p's and A2p's: the MFMAs see the same operands.
constexpr long ALL_LDS_BUDGET = 160 * 1024 - 256;      // static LDS of one workgroup, with room for alignment
__host__ __device__ constexpr int all_dict_row(int e) { return 4 * (((e >> 2) & 1) * 2 + (e >> 3)) + (e & 3); }
template <int MSTEPS, int C, bool KL>
struct AllShape {
    static constexpr int MT = MSTEPS > 4 ? 2 : 1;
    static constexpr int E = MT * 4 * 64;          // stride of one V image (accumulator order)
    static constexpr int NE = MSTEPS * 64;         // elements of V actually used
    static constexpr int RSTR = NE < 256 ? 256 : NE;   // stride of a wavefront's partial V' (exchange threads read th < 256)
    // reduce-scatter staging: whole slices hold NE words, ragged ones at most C x ceil(NE / C) <= NE + C - 1
    static constexpr int STG = C > 0 ? 1 : (C == 0 ? NE : NE + ALL_MAX_MEMBERS - 1);
    static constexpr long REST = 8L * 2 * (AW * RSTR + 2 * E + (KL ? E : 1) + STG) + 3 * 4;
    static constexpr long dict_bytes(int pr) { return 8L * ATILES * 16 * pr; }
    // M of these k-steps is 4 MSTEPS - 3 .. 4 MSTEPS; the widest row pitch that fits serves M <= PR - 1
    static constexpr int PR_ALL = 4 * MSTEPS + 2;
    static constexpr int PR = KL ? 0
                              : REST + dict_bytes(PR_ALL) <= ALL_LDS_BUDGET       ? PR_ALL
                              : REST + dict_bytes(PR_ALL - 4) <= ALL_LDS_BUDGET   ? PR_ALL - 4
                                                                                  : 0;
    // (one member - N = 512, no exchange, both halves sweep at once: measured 1.2 % slower from LDS, C1 A/B - it streams)
    static constexpr bool LDS_DICT = C != 1 && PR > 0 && PR - 1 >= 4 * MSTEPS - 3;
};

#ifdef EVC_ALL_TIMING   // diagnostic build only (tools/ubench/fused_all_bench.hip); no stamp executes in the library
#define EVC_STAMP(i)                                                                                             \
    do {                                                                                                         \
        if (a.dbg && tt0 == g - half && lane == 0 && w == 0)                                                     \
            a.dbg[(((long)blockIdx.x * 2 + half) * (2 * a.iters + 1) + step) * 4 + (i)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define EVC_STAMP(i)
#endif

// The kernel's text is evc_fused_all_body.inc, compiled three times.  EVC_ALL_LONE 0: k_fused_all<MSTEPS, C, KL>, every shape.
// EVC_ALL_LONE 1: k_fused_lone<MSTEPS, C>, the same algorithm for M == 4 MSTEPS - 3 (Frobenius, dictionary in LDS, direct
// exchange), where the last k-step of D = A_j^T V holds ONE real bin and three zero slots: that bin goes into the
// accumulator's start value as a rank-1 update (four v_fma_f64 per lane) and the D chain is one MFMA shorter - 14 MFMAs per
// unit at M = 25 instead of 15.  A kernel of its own, not a branch or a template parameter of k_fused_all: that kernel's
// instances keep their names and their code, instruction for instruction (DESIGN.md 5.1a cont.).
// EVC_ALL_LONE 2: k_fused_quad<MSTEPS, C>, k_fused_lone with bins 16 .. 24 of V' on twelve v_mfma_f64_4x4x4_4b_f64 per unit
// instead of a second 16-row tile of four v_mfma_f64_16x16x4_f64 - again a kernel of its own, for the same reason.
#define EVC_ALL_LONE 0
#include "evc_fused_all_body.inc"
#undef EVC_ALL_LONE
#define EVC_ALL_LONE 1
#include "evc_fused_all_body.inc"
#undef EVC_ALL_LONE
#define EVC_ALL_LONE 2
#include "evc_fused_all_body.inc"
#undef EVC_ALL_LONE

// LONE: 0 k_fused_all, 1 k_fused_lone, 2 k_fused_quad
template <int MSTEPS, int C, bool KL, int LONE = 0>
static hipError_t launch_all(FusedArgs a, int n_cus, hipStream_t s) {
    void (*kernel)(FusedArgs);
    if constexpr (LONE == 2) kernel = k_fused_quad<MSTEPS, C>;
    else if constexpr (LONE == 1) kernel = k_fused_lone<MSTEPS, C>;
    else kernel = k_fused_all<MSTEPS, C, KL>;
    int occ = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, ATHREADS, 0);
    if (e != hipSuccess) return e;
    if (occ < 1) return hipErrorInvalidValue;
    long resident = n_cus;                       // one workgroup (two members) per CU
    if (2 * resident > ALL_MAX_WGS) resident = ALL_MAX_WGS / 2;
    const int cr = C > 0 ? C : a.coop_c;
    if (C == 0 && (cr < 8 || cr > 64 || (cr & (cr - 1)))) return hipErrorInvalidValue;
    if (C < 0 && (cr < 2 || cr > ALL_MAX_MEMBERS)) return hipErrorInvalidValue;
    int pairs = (int)(resident / cr);            // pairs of groups
    const int want = (a.TT + 1) / 2;
    if (pairs > want) pairs = want;
    if (pairs < 1) return hipErrorInvalidValue;
    a.groups = 2 * pairs;
    // stagger (see the kernel): launches of few iterations over many rounds of frame tiles
    a.stagger_cycles = (a.iters > 0 && a.iters <= 25 && a.TT >= 4L * a.groups && pairs >= 2) ? (long long)a.iters * ALL_STAGGER_PER_ITER : 0;
    // (the 16-byte exchange words: every group's buffer starts a multiple of 4096 bytes behind this base)
    if (C > 1 && (reinterpret_cast<uintptr_t>(a.coop_buf) & 15)) return hipErrorInvalidValue;
    if (C != 1) {
        // stale words must not carry the epoch bit of the first two exchanges (0): fill with ones
        e = hipMemsetAsync(a.coop_buf, 0xFF, sizeof(double) * 2 * (size_t)a.groups * cr * (C < 0 ? ALL_RS_STRIDE : 512), s);
        if (e != hipSuccess) return e;
    }
    if (C <= 0) {
        if (2L * a.groups * 512 > ALL_SLICE_ELEMS) return hipErrorInvalidValue;
        e = hipMemsetAsync(a.coop_buf + ALL_SLICE_OFFSET, 0xFF, sizeof(double) * 2 * (size_t)a.groups * 512, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)(pairs * cr)), dim3(ATHREADS), 0, s, a);
    return hipGetLastError();
}

template <int MSTEPS, bool KL>
static hipError_t pick_c(const FusedArgs& a, int n_cus, hipStream_t s, bool lone_bin, bool quad_rows) {
    // M = 25 with 2, 4 or 8 members: the 14-MFMA unit of k_fused_lone (C2 +1.5 %, profiles/lone_bin_README.md; lone_bin
    // false: EVC_FLAG_NO_LONE_BIN).  (Instantiated for 7 k-steps only: 25 is the one narrow width in use; with 16 members
    // and more the exchange is the longer half of a step, and M 26 .. 28 have no lone bin.)
    // The same shapes, quad_rows (false: EVC_FLAG_NO_QUAD_ROWS): k_fused_quad, whose bins 16 .. 24 of V' run on 4x4x4 MFMAs
    // (profiles/quad_rows_README.md).
    if constexpr (MSTEPS == 7 && !KL)
        if (lone_bin && a.M == 4 * MSTEPS - 3) switch (a.NT / ATILES) {
            case 2: return quad_rows ? launch_all<MSTEPS, 2, KL, 2>(a, n_cus, s) : launch_all<MSTEPS, 2, KL, 1>(a, n_cus, s);
            case 4: return quad_rows ? launch_all<MSTEPS, 4, KL, 2>(a, n_cus, s) : launch_all<MSTEPS, 4, KL, 1>(a, n_cus, s);
            case 8: return quad_rows ? launch_all<MSTEPS, 8, KL, 2>(a, n_cus, s) : launch_all<MSTEPS, 8, KL, 1>(a, n_cus, s);
            default: break;
        }
    switch (a.NT / ATILES) {
        case 1: return launch_all<MSTEPS, 1, KL>(a, n_cus, s);
        case 2: return launch_all<MSTEPS, 2, KL>(a, n_cus, s);
        case 4: return launch_all<MSTEPS, 4, KL>(a, n_cus, s);
        // 8 members.  With the fragments streamed from L2 the direct exchange (every member fetches all 8 partials: 296 GB
        // of fabric traffic per C2 launch) and the reduce-scatter (37 GB) ran equally fast - 953 vs 958 k frames/s at C2 -
        // so the leaner one served.  With the dictionary in LDS (round 5) the sweep no longer queues fragment loads in
        // front of the exchange's, and the direct form's single hand-off makes the shorter step: C2 1.099 M frames/s
        // against 1.050 M for the reduce-scatter and 1.058 M before.  Shapes whose dictionary does not
        // fit (M 26 .. 28) keep the reduce-scatter of the streamed kernel.  (Below 7 members the reduce-scatter's 4 lanes
        // per element do not cover a slice.)
        case 8:
            if constexpr (AllShape<MSTEPS, 8, KL>::LDS_DICT)
                if (a.M > 0 && a.M < AllShape<MSTEPS, 8, KL>::PR) return launch_all<MSTEPS, 8, KL>(a, n_cus, s);
            return launch_all<MSTEPS, 0, KL>(a, n_cus, s);
        case 16:
        case 32:
        case 64: return launch_all<MSTEPS, 0, KL>(a, n_cus, s);    // run-time members, reduce-scatter, whole slices
        default: return launch_all<MSTEPS, -1, KL>(a, n_cus, s);  // any other count: ragged slices
    }
}

// members per frame tile the all-resident kernel would use for this problem, 0 if it does not apply
int fused_all_members(int NT, int N, int eps_mode, int exact_div, int loss) {
    // (either loss: the KL update needs the ZERO_REPLACE guard and no L1, which evc_nmf_solve checks)
    if (eps_mode == EVC_EPS_NONE || exact_div || (loss != EVC_LOSS_FROBENIUS && loss != EVC_LOSS_KL)) return 0;
    if (NT % ATILES) return 0;
    const int c = NT / ATILES;
    // The KL sweep has almost no VALU work (3.5 us), so with 2 .. 15 members a step is as long as its exchange and
    // k_fused_res's streaming form is as fast or faster (C2-sized batches, k frames/s, all-resident vs streamed:
    // N = 512: 19 800 vs 14 000; 2048: 2 234 vs 2 263; 4096: 930 vs 1 115; 8192: 458 vs 423; 16 384: 214 vs 138)
    if (loss == EVC_LOSS_KL && c >= 2 && c < 16) return 0;
    return (c >= 1 && c <= ALL_MAX_MEMBERS) ? c : 0;
}

hipError_t fused_all_launch(int msteps, const FusedArgs& a, int n_cus, hipStream_t s, bool lone_bin, bool quad_rows) {
    if (a.NT % ATILES || !a.coop_buf || !a.coop_abort) return hipErrorInvalidValue;
    switch (msteps) {
        case 1: return a.loss == EVC_LOSS_KL ? pick_c<1, true>(a, n_cus, s, lone_bin, quad_rows) : pick_c<1, false>(a, n_cus, s, lone_bin, quad_rows);
        case 2: return a.loss == EVC_LOSS_KL ? pick_c<2, true>(a, n_cus, s, lone_bin, quad_rows) : pick_c<2, false>(a, n_cus, s, lone_bin, quad_rows);
        case 3: return a.loss == EVC_LOSS_KL ? pick_c<3, true>(a, n_cus, s, lone_bin, quad_rows) : pick_c<3, false>(a, n_cus, s, lone_bin, quad_rows);
        case 4: return a.loss == EVC_LOSS_KL ? pick_c<4, true>(a, n_cus, s, lone_bin, quad_rows) : pick_c<4, false>(a, n_cus, s, lone_bin, quad_rows);
        case 5: return a.loss == EVC_LOSS_KL ? pick_c<5, true>(a, n_cus, s, lone_bin, quad_rows) : pick_c<5, false>(a, n_cus, s, lone_bin, quad_rows);
        case 6: return a.loss == EVC_LOSS_KL ? pick_c<6, true>(a, n_cus, s, lone_bin, quad_rows) : pick_c<6, false>(a, n_cus, s, lone_bin, quad_rows);
        case 7: return a.loss == EVC_LOSS_KL ? pick_c<7, true>(a, n_cus, s, lone_bin, quad_rows) : pick_c<7, false>(a, n_cus, s, lone_bin, quad_rows);
        case 8: return a.loss == EVC_LOSS_KL ? pick_c<8, true>(a, n_cus, s, lone_bin, quad_rows) : pick_c<8, false>(a, n_cus, s, lone_bin, quad_rows);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace evc
