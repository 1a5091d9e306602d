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
//     normally succeeds at once.
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

// KL: the generalised Kullback-Leibler update (sklearn _nmf.py:557-606 with update_H=False): A1p then holds the
// dictionary divided by its column sums, the sweep's B operand is R = X / max(V, eps) instead of V, the update is
// h <- h * (A~_j^T R) - no numerator tiles, no division in the sweep - and R is formed where V is combined.
template <int MSTEPS, int C, bool KL>
__global__ __launch_bounds__(ATHREADS, 2) void k_fused_all(FusedArgs a) {
    using S = AllShape<MSTEPS, C, KL>;
    constexpr int MT = S::MT;
    constexpr int E = S::E;
    constexpr int NE = S::NE;
    constexpr int RSTR = S::RSTR;
    constexpr int MSP = (MSTEPS + 1) & ~1;       // k-steps padded to pairs in A1p
    constexpr int PR = S::PR;                    // LDS dictionary: row pitch (doubles)
    constexpr int TPD = 16 * PR;                 // LDS dictionary: doubles per tile
    // (16-byte aligned: the direct exchange reads and writes pairs of elements)
    __shared__ __attribute__((aligned(16))) double s_red[2][AW * RSTR];   // partial V' of every wavefront, per half
    __shared__ __attribute__((aligned(16))) double s_v[2][E];             // V, B-operand order
    __shared__ __attribute__((aligned(16))) double s_x[2][E];             // X, B-operand order
    __shared__ __attribute__((aligned(16))) double s_r[2][KL ? E : 1];    // KL: X / max(V, eps), B-operand order
    __shared__ double s_stage[2][S::STG];        // reduce-scatter staging (more than 8 members only)
    __shared__ double s_dict[S::LDS_DICT ? ATILES * TPD : 1];   // the member's dictionary (see AllShape)
    __shared__ unsigned s_hb[2];                 // arrivals of a half's wavefronts at its LDS barrier
    __shared__ int s_fail;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = w8 >> 2, w = w8 & 3, th = tid & (AW * 64 - 1);
    const int CR = C > 0 ? C : a.coop_c;                     // members per group (C <= 0: at run time)
    const int member = blockIdx.x % CR;
    const int g = 2 * (blockIdx.x / CR) + half;          // the group this half is a member of
    double* const red = s_red[half];
    double* const vL = s_v[half];
    double* const xL = s_x[half];
    double* const rL = s_r[half];
    double* const stage = s_stage[half];
    unsigned hb = 0;                             // arrivals expected at this half's next LDS barrier
    const double* __restrict__ A1p = a.A1p;
    const double* __restrict__ A2p = a.A2p;
    f64x2* __restrict__ Hp = a.Hp;
    const int NT = a.NT;
    const long tile0 = (long)member * ATILES + w;       // this wavefront's tiles: tile0 + AW * k
    const unsigned ul = (unsigned)lane;
    // Tile base addresses are wave-uniform (SGPR base + unsigned per-lane offset).  `sw` is an opaque zero
    // refreshed once per sweep so that the 16 tile addresses are re-derived with scalar adds instead of being
    // hoisted out of the loops as per-lane 64-bit addresses (32 VGPRs).
    long sw = 0;

    // Round 4: the fragments come by buffer loads - the tile's byte offset rides in the instruction's scalar offset, the
    // lane's in a 32-bit register computed once, the k-step's in the immediate: no address arithmetic in the sweep.
    // (As global loads the lane term became a 64-bit shift-and-add per fragment group: 6 vector instructions per unit,
    // ~24 cycles beside the MFMAs; the compiler does not select the scalar-base form of global_load for it.)
    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(A1p), 0, NT * (MSP * 512), 0x00020000);
    const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(A2p), 0, NT * (MT * 2048), 0x00020000);
    // the direct exchange's buffers, both parities of every group: a group's base rides in the scalar offset
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(a.coop_buf, 0, C > 1 ? 2 * a.groups * (C * 4096) : 0, 0x00020000);
#ifdef EVC_ALL_NOFRAG
    bool nofrag_go = false;
#endif
    const unsigned ul16 = ul * 16u;
    // LDS dictionary (S::LDS_DICT and M < PR): this lane's element of every fragment is one immediate away from one of
    // four addresses - D/P order, its last k-step, V' order, its last bin tile (bins past M: the row's zero slot M)
    constexpr int BL = 16 * ((MSTEPS - 1) >> 2) + 4 * ((MSTEPS - 1) & 3);     // first bin of the last k-step
    const int rowA = w * AKT * TPD + all_dict_row(4 * (lane & 3) + ((lane & 15) >> 2)) * PR;
    const int rowB = w * AKT * TPD + all_dict_row(4 * (lane >> 4)) * PR;
    const double* const dA = s_dict + rowA + (lane >> 4);
    const double* const dAL = s_dict + rowA + min(lane >> 4, a.M - BL);
    const double* const dB = s_dict + rowB + (lane & 15);
    const double* const dBL = s_dict + rowB + min(lane & 15, a.M - 16 * (MT - 1));
    // `lds`: std::true_type - fragments from s_dict, std::false_type - buffer loads from A1p / A2p.  (The compiler would
    // pair reads off one address into ds_read2_b64: 8 LDS cycles for 16-lane groups, where this layout is 2-way
    // conflicted, against 2 x 2 for two ds_read_b64 - an empty asm with a memory clobber between the reads keeps them apart.)
#define LDS_NO_PAIR() asm volatile("" ::: "memory")
    auto load_a1 = [&](double (&a1)[MSTEPS], int k, auto lds) {
        if constexpr (decltype(lds)::value) {
#pragma unroll
            for (int s = 0; s < MSTEPS; ++s) {
                a1[s] = (s == MSTEPS - 1 ? dAL : dA)[k * TPD + 16 * (s >> 2) + 4 * (s & 3)];
                LDS_NO_PAIR();
            }
            return;
        }
#ifdef EVC_ALL_NOFRAG    // diagnostic (tools/ubench): no fragment traffic after the numerator pass (wrong results, timing only)
        if (nofrag_go) return;
#endif
        const int so = (int)(tile0 + sw + AW * k) * (MSP * 512);
#pragma unroll
        for (int s = 0; s < MSTEPS; s += 2) {
            if (s + 1 < MSTEPS) {
                const f64x2 v = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(r1, ul16 + (s >> 1) * 1024, so, 0));
                a1[s] = v[0];
                a1[s + 1] = v[1];
            } else {        // (the odd k-step's half of the pair: the first double of the lane's 16 bytes)
                a1[s] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r1, ul16 + (s >> 1) * 1024, so, 0));
            }
        }
    };
    auto load_a2 = [&](double (&a2)[MT][4], int k, auto lds) {
        if constexpr (decltype(lds)::value) {
#pragma unroll
            for (int u = 0; u < MT; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    a2[u][r] = (u == MT - 1 ? dBL : dB)[k * TPD + r * PR + 16 * u];
                    LDS_NO_PAIR();
                }
            return;
        }
#ifdef EVC_ALL_NOFRAG
        if (nofrag_go) return;
#endif
        const int so = (int)(tile0 + sw + AW * k) * (MT * 2048);
#pragma unroll
        for (int u = 0; u < MT; ++u)
#pragma unroll
            for (int r = 0; r < 4; r += 2) {
                const f64x2 v = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(r2, ul16 + (u * 2 + (r >> 1)) * 1024, so, 0));
                a2[u][r] = v[0];
                a2[u][r + 1] = v[1];
            }
    };

    const int mode = a.eps_mode;
    const double eps = a.eps;
    const double d0 = a.l1 + (mode == EVC_EPS_ADD ? a.eps : 0.0);
    const f64x4 dinit = {d0, d0, d0, d0};
    const unsigned lo = fast_lo(mode, eps);
    unsigned seq = 0;                            // exchanges done by this half's group so far
    // reduce-scatter exchange with ragged slices (C < 0): what this thread publishes and fetches, the same in every exchange
    int rs_es = 1, rs_len = 0, rs_pub0 = 0, rs_pub1 = 0, rs_src0 = -1, rs_src1 = -1, rs_src2 = -1;
    if (C < 0) {
        rs_es = (NE + CR - 1) / CR;                                  // elements per slice
        rs_len = NE - member * rs_es;                                // of which valid in mine
        rs_len = rs_len < 0 ? 0 : (rs_len > rs_es ? rs_es : rs_len);
        const int e0 = th, e1 = th + AW * 64;
        const int j0 = e0 / rs_es, j1 = (e1 < NE ? e1 : e0) / rs_es;
        rs_pub0 = (j0 * CR + member) * rs_es + (e0 - j0 * rs_es);
        rs_pub1 = (j1 * CR + member) * rs_es + ((e1 < NE ? e1 : e0) - j1 * rs_es);
        // my slice region is [m][ES] row-major at (member * CR) * ES: word idx = m * ES + el, valid while el < len
        auto src = [&](int idx) {
            if (idx >= CR * rs_es) return -1;
            const int el = idx % rs_es;
            return el < rs_len ? member * CR * rs_es + idx : -1;
        };
        rs_src0 = src(th);
        rs_src1 = src(th + AW * 64);
        rs_src2 = src(th + 2 * AW * 64);
    }
    if (tid == 0) s_fail = 0;
    if (tid < 2) s_hb[tid] = 0;

    // Short launches (the stop rule's 10-iteration pieces of a long batch): every group reaches the end of a frame tile
    // at the same moment, and the chip then does nothing but store and reload activations (2 x 66 MB per round at C2:
    // 21 us against 100 us of iterations, profiles/r04_default_call.md).  Every second pair of groups starts half a
    // tile's duration late, once per launch, so that only half of the CUs move activations at any time: the default
    // call's rate went from 0.845 to 0.866 of the rate without stop tests (same box, A/B; four or eight phases: the same -
    // a CU streams at ~25 GB/s however many others do, so what is left would have to overlap with the CU's own sweeps).
    if (a.stagger_cycles > 0 && ((blockIdx.x / CR) & 1)) {
        const long long t0 = __builtin_amdgcn_s_memtime();
        while (__builtin_amdgcn_s_memtime() - t0 < a.stagger_cycles) __builtin_amdgcn_s_sleep(32);
    }

    auto run = [&](auto lds) __attribute__((always_inline)) {
    for (long tt0 = g - half; tt0 < a.TT; tt0 += a.groups) {     // half 0's tile decides (it has the lower index)
        const long tt = tt0 + half;
        bool valid;
        {
            const long t = 16 * tt + (lane & 15);
            int u = -1;
            if (tt < a.TT && t < a.T_) u = a.frame_utt[t];
            // padding frames count as live; a tile beyond the batch, or one holding frames of a stopped
            // utterance (left to the general kernel, skip_all_live), is not processed
            const bool live = tt < a.TT && ((t >= a.T_) || ((u >= 0) && (a.active[u] != 0)));
            const int v0 = __syncthreads_and(half == 0 ? live : true);
            const int v1 = __syncthreads_and(half == 1 ? live : true);
            valid = (half ? v1 : v0) != 0;
        }
        HTile h[AKT];
        f64x4 p[AKT];
        double a1[MSTEPS], a2[MT][4];
        if (valid && a.first && a.init_const) {
            // first launch from the utterances' constants: H = h0 (0 in the padding), V = A H = h0 rowsum(A)
            auto h0_of = [&](int fr) {
                const long t = 16 * tt + fr;
                const int u = t < a.T_ ? a.frame_utt[t] : -1;
                return u >= 0 ? a.h0[u] : 0.0;
            };
            for (int e = th; e < E; e += AW * 64) {
                const int s = e >> 6, l = e & 63;
                const bool in = s < MSTEPS;
                xL[e] = in ? a.Xp[(tt * MSTEPS + s) * 64 + l] : 0.0;
                vL[e] = in ? a.rsum[bin_of(s, l >> 4)] * h0_of(l & 15) : 0.0;
                if (KL) rL[e] = xL[e] / (vL[e] < a.eps ? a.eps : vL[e]);
            }
            const double hv = h0_of(lane & 15);
#pragma unroll
            for (int k = 0; k < AKT; ++k) {
                const long n0 = 16 * (tile0 + AW * k) + 4 * (lane >> 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) h[k][r] = n0 + r < a.N ? hv : 0.0;
            }
        } else if (valid) {
            for (int e = th; e < E; e += AW * 64) {
                const int s = e >> 6, l = e & 63;
                const bool in = s < MSTEPS;
                xL[e] = in ? a.Xp[(tt * MSTEPS + s) * 64 + l] : 0.0;
                vL[e] = in ? a.Vp[(tt * 8 + s) * 64 + l] : 0.0;
                if (KL) rL[e] = xL[e] / (vL[e] < a.eps ? a.eps : vL[e]);       // sklearn _nmf.py:572-576
            }
#pragma unroll
            for (int k = 0; k < AKT; ++k) {
                const f64x2* t = Hp + (tt * NT + tile0 + AW * k) * 128;
                const f64x2 h01 = t[ul], h23 = t[ul + 64];
                h[k][0] = h01[0]; h[k][1] = h01[1]; h[k][2] = h23[0]; h[k][3] = h23[1];
            }
        }
        __syncthreads();
        if (valid && !KL) {                      // numerator tiles, once per frame tile
            double x[MSTEPS];
#pragma unroll
            for (int s = 0; s < MSTEPS; ++s) x[s] = xL[s * 64 + lane];
            load_a1(a1, 0, lds);
#pragma unroll
            for (int k = 0; k < AKT; ++k) {
                f64x4 acc = {0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < MSTEPS; ++s) acc = Mma<double>::mma(a1[s], x[s], acc);
                if (!decltype(lds)::value || k + 1 < AKT) load_a1(a1, (k + 1) % AKT, lds);
                p[k] = acc;
            }
        }

        if (valid && KL) load_a1(a1, 0, lds);         // (the numerator pass, which otherwise leaves them, is skipped)
        for (int step = 0; step <= 2 * a.iters; ++step) {
#ifdef EVC_ALL_NOFRAG
            nofrag_go = step > 2;
#endif
            // this half's turn on the matrix pipes.  (One member per frame tile - N <= 512 - has no exchange to hide:
            // both halves then sweep in the same steps, two wavefronts per SIMD.)
            const bool mine = C == 1 ? (step & 1) == 0 : (step & 1) == half;
            EVC_STAMP(0);
            if (valid && mine && step < 2 * a.iters) {
                // ---------------- sweep: h <- h p / (A_j^T V), V' += A_j h over the 8 resident tiles
                asm volatile("" : "+s"(sw));
                double v[MSTEPS];
#pragma unroll
                for (int s = 0; s < MSTEPS; ++s) v[s] = KL ? rL[s * 64 + lane] : vL[s * 64 + lane];
                // (from LDS the first unit's fragments come at the start of the sweep: held across the exchange step
                // instead, they cost 14 registers there, and the compiler spilled around the sweep)
                if constexpr (decltype(lds)::value) load_a1(a1, 0, lds);
                f64x4 vn[MT];
#pragma unroll
                for (int u = 0; u < MT; ++u) vn[u] = f64x4{0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < AKT; ++k) {
                    __builtin_amdgcn_sched_barrier(0);
                    load_a2(a2, k, lds);
                    f64x4 d = KL ? f64x4{0, 0, 0, 0} : dinit;
#pragma unroll
                    for (int s = 0; s < MSTEPS; ++s) d = Mma<double>::mma(a1[s], v[s], d);
                    if (!decltype(lds)::value || k + 1 < AKT)
                        load_a1(a1, (k + 1) % AKT, lds);  // the next unit's (streamed: or the next sweep's first) fragments
                    __builtin_amdgcn_sched_barrier(0);
                    if (KL) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) h[k][r] *= d[r];
                    } else {
                        mu_tile_guarded(h[k], p[k], d, mode, eps, lo);
                    }
#pragma unroll
                    for (int u = 0; u < MT; ++u)
#pragma unroll
                        for (int r = 0; r < 4; ++r) vn[u] = Mma<double>::mma(a2[u][r], h[k][r], vn[u]);
                }
#pragma unroll
                for (int u = 0; u < MT; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (u * 4 + r < MSTEPS) red[w * RSTR + (u * 4 + r) * 64 + lane] = vn[u][r];
            } else if (C > 1 && valid && !mine && step > 0) {
                // ---------------- exchange, 2 / 4 / 8 members, on 16-byte words (round 7).  Thread th < NE / 2 owns the
                // elements 2 th and 2 th + 1: one ds_read_b128 per wavefront's partial, ONE 16-byte sc1 store, and per fetch
                // round one 16-byte sc1 load per peer (8-byte sc1 accesses run at 0.54 - 0.70 of the 16-byte rate, and a
                // per-lane 8-byte sc1 store costs 2.7 x the fabric time per byte).  Each 8-byte half still carries its own
                // epoch bit and is checked by itself: nothing rests on the 16 bytes arriving together.  The sums run in the
                // order wavefronts 0 .. 3, then members 0 .. C - 1 (the 8-byte form it replaced: DESIGN.md 5.1a, round 7).
                // Threads from NE / 2 on move nothing; a wavefront of such threads only counts the exchange.
                __builtin_amdgcn_s_setprio(ALL_EXCH_PRIO);
                const bool act = th < NE / 2;
                const int ep = act ? 2 * th : 0;
                f64x2 sm = {0.0, 0.0};
                if (w * 64 < NE / 2) {
                    f64x2 pv[AW];
#pragma unroll
                    for (int ww = 0; ww < AW; ++ww) pv[ww] = *reinterpret_cast<const f64x2*>(red + ww * RSTR + ep);
                    // (the four reads in flight together: one LDS round trip, not four)
                    static_assert(AW == 4, "the four partials are named one by one");
                    asm volatile("" : "+v"(pv[0]), "+v"(pv[1]), "+v"(pv[2]), "+v"(pv[3]));
#pragma unroll
                    for (int ww = 0; ww < AW; ++ww) sm += pv[ww];
                    const long long tag = (seq >> 1) & 1;        // a buffer is reused every second exchange
                    const long long m0 = (__double_as_longlong(sm[0]) & ~1LL) | tag;
                    const long long m1 = (__double_as_longlong(sm[1]) & ~1LL) | tag;
                    // byte offset of this exchange's buffer (wave-uniform); member m's words follow at m * 4096
                    const int xo = __builtin_amdgcn_readfirstlane((int)(((seq & 1) * (unsigned)a.groups + (unsigned)g) * (unsigned)(C * 4096)));
                    if (act)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(all_u32x4, all_i64x2{m0, m1}), rx, ep * 8,
                                                               xo + member * 4096, 16);
                    bool ok = true;
                    unsigned polls = 0;
                    {   // watch one word per peer (lane m <-> member m): C - 1 loads per poll and wavefront.  (Without it the
                        // exchange is shorter but its polls lengthen the sweep beside it: profiles/r07_README.md)
                        const long long* sp = reinterpret_cast<const long long*>(a.coop_buf) +
                                              ((size_t)(seq & 1) * a.groups + g) * (size_t)(C * 512) +
                                              (lane < C ? lane : 0) * 512 + (NE - 1);
                        for (;;) {
                            const long long b = __hip_atomic_load(sp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            const bool ready = lane >= C || lane == member || (b & 1) == tag;
                            if (__all(ready)) break;
                            if (all_polls_out(polls, a.coop_abort)) {
                                ok = false;
                                break;
                            }
                            __builtin_amdgcn_s_sleep(2);
                        }
                    }
                    // every active thread fetches its pair from every peer (its own comes from registers); a half with a
                    // stale epoch makes the thread fetch again
                    all_i64x2 b[C > 0 ? C : 1] = {};
                    polls = 0;
                    while (__builtin_expect(ok && act, 1)) {        // (runs at least once: laid out in line)
                        asm volatile("" ::: "memory");      // (the builtin load is not volatile: it stays in the loop)
#pragma unroll
                        for (int m = 0; m < C; ++m)
                            if (m != member)
                                b[m] = __builtin_bit_cast(all_i64x2, __builtin_amdgcn_raw_buffer_load_b128(rx, ep * 8, xo + m * 4096, 16));
                        long long bad = 0;
#pragma unroll
                        for (int m = 0; m < C; ++m) {
                            b[m] = (m == member) ? all_i64x2{m0, m1} : b[m];
                            bad |= (b[m][0] ^ tag) | (b[m][1] ^ tag);
                        }
                        if ((bad & 1) == 0) break;
                        if (all_polls_out(polls, a.coop_abort)) {
                            ok = false;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(2);
                    }
                    f64x2 v2 = {0.0, 0.0};
#pragma unroll
                    for (int m = 0; m < C; ++m) {                 // member order: identical on every member
                        v2[0] += __longlong_as_double(b[m][0] & ~1LL);
                        v2[1] += __longlong_as_double(b[m][1] & ~1LL);
                    }
                    if (!ok) s_fail = 1;
                    if (act) {
                        *reinterpret_cast<f64x2*>(vL + ep) = v2;
                        if (KL) {
                            const f64x2 x2 = *reinterpret_cast<const f64x2*>(xL + ep);
                            *reinterpret_cast<f64x2*>(rL + ep) =
                                f64x2{x2[0] / (v2[0] < a.eps ? a.eps : v2[0]), x2[1] / (v2[1] < a.eps ? a.eps : v2[1])};
                        }
                    }
                }
                ++seq;
                __builtin_amdgcn_s_setprio(0);
            } else if (valid && !mine && step > 0) {
                // ---------------- exchange: V' = sum over wavefronts and members, no barrier inside
                // (run-time member counts with M <= 12: fewer elements than threads - several threads carry one element, word
                // for word; a thread beyond NE used to poll a word of the summed slices that nobody writes)
                const int e0 = C <= 0 ? th % NE : th, e1 = th + AW * 64;
                const bool has1 = e1 < NE;
                // (the exchanging wavefront goes first: ALL_EXCH_PRIO)
                __builtin_amdgcn_s_setprio(ALL_EXCH_PRIO);
                double s0 = 0.0, s1 = 0.0;
#pragma unroll
                for (int ww = 0; ww < AW; ++ww) {
                    s0 += red[ww * RSTR + e0];
                    s1 += red[ww * RSTR + (has1 ? e1 : e0)];
                }
                if (C < 0) {
                    // ---- any member count without a template of its own (3, 5, 6, 7, 9 ... : N up to 32 x 512 x ...):
                    // reduce-scatter + all-gather.  Fetching every member's partial costs (C - 1) x 3.5 KB per member
                    // and exchange (108 KB at C = 32): far longer than the sweep it hides behind.  Instead member m sums
                    // slice m (ES = ceil(NE / C) elements; the last slices may be short or empty) of all C partials
                    // and publishes it; everybody then fetches the summed slices: 7 KB per member and exchange
                    // whatever C is, for a second memory round trip - which the alternation hides.
                    long long* xb1 = reinterpret_cast<long long*>(a.coop_buf) +
                                     ((size_t)(seq & 1) * a.groups + g) * (size_t)CR * ALL_RS_STRIDE;
                    long long* xb2 = reinterpret_cast<long long*>(a.coop_buf) + ALL_SLICE_OFFSET +
                                     ((size_t)(seq & 1) * a.groups + g) * 512;
                    const long long tag = (seq >> 1) & 1;
                    // partials: [slice j][member m][ES], so that what member j reduces is one contiguous run
                    __hip_atomic_store(xb1 + rs_pub0, (__double_as_longlong(s0) & ~1LL) | tag, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                    if (has1)
                        __hip_atomic_store(xb1 + rs_pub1, (__double_as_longlong(s1) & ~1LL) | tag, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                    bool ok = true;
                    // poll three words (one memory round trip for all) until each carries the epoch of this exchange
                    auto fetch3 = [&](const long long* p0, const long long* p1, const long long* p2, long long& b0,
                                      long long& b1, long long& b2) {
                        unsigned polls = 0;
                        for (;;) {
                            b0 = __hip_atomic_load(p0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            b1 = __hip_atomic_load(p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            b2 = __hip_atomic_load(p2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (__all(!ok || (((b0 ^ tag) | (b1 ^ tag) | (b2 ^ tag)) & 1) == 0)) break;
                            if (all_polls_out(polls, a.coop_abort))
                                ok = false;
                            __builtin_amdgcn_s_sleep(1);
                        }
                    };
                    // reduce: my slice of all CR partials (one contiguous run: fully coalesced) goes through LDS; the
                    // half's 4 wavefronts meet at an LDS counter (a workgroup barrier would stop the other half's
                    // sweep); then 4 lanes per element sum the members q, q + 4, ... in order and combine (a fixed
                    // tree: every member obtains the bitwise identical V').  A thread's words are the same in every
                    // exchange (rs_src*, -1: none - it then re-reads a word it published itself).
                    {
                        long long b0, b1, b2;
                        const long long* own = xb1 + rs_pub0;
                        fetch3(rs_src0 >= 0 ? xb1 + rs_src0 : own, rs_src1 >= 0 ? xb1 + rs_src1 : own,
                               rs_src2 >= 0 ? xb1 + rs_src2 : own, b0, b1, b2);
                        if (rs_src0 >= 0) stage[th] = __longlong_as_double(b0 & ~1LL);
                        if (rs_src1 >= 0) stage[th + AW * 64] = __longlong_as_double(b1 & ~1LL);
                        if (rs_src2 >= 0) stage[th + 2 * AW * 64] = __longlong_as_double(b2 & ~1LL);
                        hb += AW;
                        if (lane == 0)
                            __hip_atomic_fetch_add(&s_hb[half], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                        while ((int)(__hip_atomic_load(&s_hb[half], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) - hb) < 0)
                            __builtin_amdgcn_s_sleep(1);
                        const int q = th & 3;
                        for (int el = th >> 2; el < rs_len; el += AW * 16) {
                            double v = 0.0;
                            for (int m = q; m < CR; m += 4) v += stage[m * rs_es + el];
                            v += __shfl_xor(v, 1, 64);
                            v += __shfl_xor(v, 2, 64);
                            if (q == 0)
                                __hip_atomic_store(xb2 + member * rs_es + el, (__double_as_longlong(v) & ~1LL) | tag,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                    // gather: the summed slices (element e of V' is word e)
                    long long g0, g1, g2;
                    fetch3(xb2 + e0, xb2 + (has1 ? e1 : e0), xb2 + e0, g0, g1, g2);
                    s0 = __longlong_as_double(g0 & ~1LL);
                    s1 = __longlong_as_double(g1 & ~1LL);
                    ++seq;
                    if (!ok) s_fail = 1;
                } else if (C == 0) {
                    // ---- 16, 32 or 64 members (N = 8192, 16384, 32768): the same reduce-scatter with whole slices
                    // (CR divides NE) and two words per thread: the leaner code of the common sizes.
                    const int ES = NE / CR;                          // elements per slice (CR divides 64)
                    long long* xb1 = reinterpret_cast<long long*>(a.coop_buf) +
                                     ((size_t)(seq & 1) * a.groups + g) * (size_t)CR * 512;
                    long long* xb2 = reinterpret_cast<long long*>(a.coop_buf) + ALL_SLICE_OFFSET +
                                     ((size_t)(seq & 1) * a.groups + g) * 512;
                    const long long tag = (seq >> 1) & 1;
                    // partials: [slice j][member m][ES], so that what member j reduces is one contiguous run
                    {
                        const int j0 = e0 / ES, j1 = (has1 ? e1 : e0) / ES;
                        __hip_atomic_store(xb1 + ((size_t)j0 * CR + member) * ES + (e0 - j0 * ES),
                                           (__double_as_longlong(s0) & ~1LL) | tag, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                        if (has1)
                            __hip_atomic_store(xb1 + ((size_t)j1 * CR + member) * ES + (e1 - j1 * ES),
                                               (__double_as_longlong(s1) & ~1LL) | tag, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                    }
                    bool ok = true;
                    // poll two words (one memory round trip for both) until each carries the epoch of this exchange
                    auto fetch2 = [&](const long long* p0, const long long* p1, long long& b0, long long& b1) {
                        unsigned polls = 0;
                        for (;;) {
                            b0 = __hip_atomic_load(p0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            b1 = __hip_atomic_load(p1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (__all(!ok || (((b0 ^ tag) | (b1 ^ tag)) & 1) == 0)) break;
                            if (all_polls_out(polls, a.coop_abort))
                                ok = false;
                            __builtin_amdgcn_s_sleep(1);
                        }
                    };
                    // reduce: my slice of all CR partials (NE words, contiguous: fully coalesced) goes through LDS;
                    // the half's 4 wavefronts meet at an LDS counter (a workgroup barrier would stop the other
                    // half's sweep); then 4 lanes per element sum CR / 4 members each in fixed order and combine
                    // (a fixed tree: every member obtains the bitwise identical V')
                    {
                        long long b0, b1;
                        const long long* mine_ = xb1 + (size_t)member * NE;
                        fetch2(mine_ + e0, mine_ + (has1 ? e1 : e0), b0, b1);
                        stage[e0] = __longlong_as_double(b0 & ~1LL);
                        if (has1) stage[e1] = __longlong_as_double(b1 & ~1LL);
                        hb += AW;
                        if (lane == 0)
                            __hip_atomic_fetch_add(&s_hb[half], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                        while ((int)(__hip_atomic_load(&s_hb[half], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) - hb) < 0)
                            __builtin_amdgcn_s_sleep(1);
                        // (4 lanes per element, each walking CR / 4 staged values.  Round 4 tried as many lanes as the half
                        // has - 16 per element at 32 members, a lane summing two values before a 4-step butterfly:
                        // slower, 1.63 against 1.53 ms per 60 iterations at C5 - the butterfly's permutes cost more than
                        // the LDS reads they replace)
                        if (th < 4 * ES) {
                            const int el = th >> 2, q = th & 3, per = CR >> 2;
                            double v = 0.0;
                            for (int i = 0; i < per; ++i) v += stage[(q * per + i) * ES + el];
                            v += __shfl_xor(v, 1, 64);
                            v += __shfl_xor(v, 2, 64);
                            if (q == 0)
                                __hip_atomic_store(xb2 + member * ES + el, (__double_as_longlong(v) & ~1LL) | tag,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                    // gather: the C summed slices
                    long long g0, g1;
                    fetch2(xb2 + e0, xb2 + (has1 ? e1 : e0), g0, g1);
                    s0 = __longlong_as_double(g0 & ~1LL);
                    s1 = __longlong_as_double(g1 & ~1LL);
                    ++seq;
                    if (!ok) s_fail = 1;
                }
                vL[e0] = s0;
                if (has1) vL[e1] = s1;
                if (KL) {
                    rL[e0] = xL[e0] / (s0 < a.eps ? a.eps : s0);
                    if (has1) rL[e1] = xL[e1] / (s1 < a.eps ? a.eps : s1);
                }
                __builtin_amdgcn_s_setprio(0);
            }
            EVC_STAMP(1);
            __syncthreads();
            EVC_STAMP(2);
            if (C != 1 && s_fail) {              // a peer never showed up: void the launch, let everybody leave
                if (tid == 0) __hip_atomic_store(a.coop_abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
        }

        // ---------------- the end of the frame tile
        // Round 9, last launch with a synthesis behind it (a.Yslab): this member's share of Y = B H while the activations
        // are still in registers - one more V'-shaped pass over the 8 resident tiles with B's fragments (streamed from
        // B2p: the LDS dictionary holds A), the 4 wavefronts' partials summed in order through s_red (nobody exchanges
        // any more), the sums to the member's slab.  k_unpack_y adds the slabs in member order.  Every frame tile is
        // valid in such a launch (nothing can stop); the barriers are taken by everybody all the same.
        // B's bin tiles of 16 (a.y_mt) are the instance's MT or, for a short B beside a tall A, 1: the tile count is a
        // compile-time constant of each copy of the pass, so that its loads are those of the streamed load_a2.
        auto y_tail = [&](auto ut) __attribute__((always_inline)) {
            constexpr int UT = decltype(ut)::value;
            f64x4 yn[UT];
#pragma unroll
            for (int u = 0; u < UT; ++u) yn[u] = f64x4{0, 0, 0, 0};
            if (valid) {
                const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(a.Yb2p), 0, NT * (UT * 2048), 0x00020000);
#pragma unroll
                for (int k = 0; k < AKT; ++k) {
                    const int so = (int)(tile0 + AW * k) * (UT * 2048);
                    double b2[UT][4];
#pragma unroll
                    for (int u = 0; u < UT; ++u)
#pragma unroll
                        for (int r = 0; r < 4; r += 2) {
                            const f64x2 v = __builtin_bit_cast(f64x2, __builtin_amdgcn_raw_buffer_load_b128(rb, ul16 + (u * 2 + (r >> 1)) * 1024, so, 0));
                            b2[u][r] = v[0];
                            b2[u][r + 1] = v[1];
                        }
#pragma unroll
                    for (int u = 0; u < UT; ++u)
#pragma unroll
                        for (int r = 0; r < 4; ++r) yn[u] = Mma<double>::mma(b2[u][r], h[k][r], yn[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < UT; ++u) {
                if (valid) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) red[w * RSTR + r * 64 + lane] = yn[u][r];
                }
                __syncthreads();
                if (valid) {                     // thread th: k-step 4 u + th / 64, lane th % 64 of the image
                    double y = 0.0;
#pragma unroll
                    for (int ww = 0; ww < AW; ++ww) y += red[ww * RSTR + th];
                    a.Yslab[member * a.y_stride + (tt * 8 + 4 * u) * 64 + th] = y;
                }
                __syncthreads();
            }
        };
        if (a.Yslab) {
            if (MT > 1 && a.y_mt == 1) y_tail(std::integral_constant<int, 1>{});
            else y_tail(std::integral_constant<int, MT>{});
        }
        if (valid) {
            if (!a.skip_hp) {                    // (skipped: the last launch, when nothing reads the packed tiles after it)
#pragma unroll
                for (int k = 0; k < AKT; ++k) {
                    f64x2* t = Hp + (tt * NT + tile0 + AW * k) * 128;
                    t[ul] = f64x2{h[k][0], h[k][1]};
                    t[ul + 64] = f64x2{h[k][2], h[k][3]};
                }
            }
            if (a.Hx) {                          // last launch: the caller's H as well (no separate export pass)
                const long t = 16 * tt + (lane & 15);
                if (t < a.T_ && a.hx_wide) {
                    // frame-major, 16-byte aligned rows: a lane's four exemplars are 32 contiguous bytes - two 16-byte
                    // stores; the pair that straddles or passes N goes element by element
#pragma unroll
                    for (int k = 0; k < AKT; ++k) {
                        const long n0 = 16 * (tile0 + AW * k) + 4 * (lane >> 4);
                        double* const row = a.Hx + t * a.ldhx + n0;
#pragma unroll
                        for (int r = 0; r < 4; r += 2) {
                            if (n0 + r + 1 < a.N) *reinterpret_cast<f64x2*>(row + r) = f64x2{h[k][r], h[k][r + 1]};
                            else if (n0 + r < a.N) row[r] = h[k][r];
                        }
                    }
                } else if (t < a.T_) {
#pragma unroll
                    for (int k = 0; k < AKT; ++k) {
                        const long n0 = 16 * (tile0 + AW * k) + 4 * (lane >> 4);
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (n0 + r < a.N) {
                                if (a.hx_frame_major) a.Hx[t * a.ldhx + n0 + r] = h[k][r];
                                else a.Hx[(n0 + r) * a.ldhx + t] = h[k][r];
                            }
                    }
                }
            }
            // carry V to the next launch; per-frame squared residual of the final activations
            if (member == 0) {                   // every member holds the same V: one writes it
                for (int e = th; e < NE; e += AW * 64) a.Vp[(tt * 8 + (e >> 6)) * 64 + (e & 63)] = vL[e];
                if (a.write_err && w == 0) {
                    double e = 0.0;
#pragma unroll
                    for (int s = 0; s < MSTEPS; ++s) {
                        const double x = xL[s * 64 + lane], vv = vL[s * 64 + lane];
                        e += KL ? kl_terms(x, vv, a.eps) : (x - vv) * (x - vv);
                    }
                    e += __shfl_xor(e, 16, 64);  // the 4 lane groups hold one frame's bins
                    e += __shfl_xor(e, 32, 64);
                    const long t = 16 * tt + lane;
                    if (lane < 16 && t < a.T_) a.err2[t] = e;
                }
            }
        }
        __syncthreads();                         // xL / vL are rewritten for the next frame tile
    }
    };

    if constexpr (S::LDS_DICT) {
        if (a.M > 0 && a.M < PR) {
            // the member's 32 tiles from A2p (A2p[j][u][r/2][l][r&1] = A[16 u + (l&15)][16 j + 4 (l>>4) + r]), once per launch
            for (int x = tid; x < ATILES * TPD; x += ATHREADS) {
                const int slot = x / TPD, e = all_dict_row((x / PR) % 16), b = x % PR;   // (all_dict_row is an involution)
                const long j = (long)member * ATILES + slot / AKT + AW * (slot % AKT);
                const int q = e >> 2, r = e & 3;
                s_dict[x] = b < a.M ? A2p[((j * MT + (b >> 4)) * 2 + (r >> 1)) * 128 + (16 * q + (b & 15)) * 2 + (r & 1)] : 0.0;
            }
            __syncthreads();
            run(std::true_type{});
            return;
        }
    }
    run(std::false_type{});
}

template <int MSTEPS, int C, bool KL>
static hipError_t launch_all(FusedArgs a, int n_cus, hipStream_t s) {
    int occ = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_fused_all<MSTEPS, C, KL>, ATHREADS, 0);
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
    hipLaunchKernelGGL((k_fused_all<MSTEPS, C, KL>), dim3((unsigned)(pairs * cr)), dim3(ATHREADS), 0, s, a);
    return hipGetLastError();
}

template <int MSTEPS, bool KL>
static hipError_t pick_c(const FusedArgs& a, int n_cus, hipStream_t s) {
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

hipError_t fused_all_launch(int msteps, const FusedArgs& a, int n_cus, hipStream_t s) {
    if (a.NT % ATILES || !a.coop_buf || !a.coop_abort) return hipErrorInvalidValue;
    switch (msteps) {
        case 1: return a.loss == EVC_LOSS_KL ? pick_c<1, true>(a, n_cus, s) : pick_c<1, false>(a, n_cus, s);
        case 2: return a.loss == EVC_LOSS_KL ? pick_c<2, true>(a, n_cus, s) : pick_c<2, false>(a, n_cus, s);
        case 3: return a.loss == EVC_LOSS_KL ? pick_c<3, true>(a, n_cus, s) : pick_c<3, false>(a, n_cus, s);
        case 4: return a.loss == EVC_LOSS_KL ? pick_c<4, true>(a, n_cus, s) : pick_c<4, false>(a, n_cus, s);
        case 5: return a.loss == EVC_LOSS_KL ? pick_c<5, true>(a, n_cus, s) : pick_c<5, false>(a, n_cus, s);
        case 6: return a.loss == EVC_LOSS_KL ? pick_c<6, true>(a, n_cus, s) : pick_c<6, false>(a, n_cus, s);
        case 7: return a.loss == EVC_LOSS_KL ? pick_c<7, true>(a, n_cus, s) : pick_c<7, false>(a, n_cus, s);
        case 8: return a.loss == EVC_LOSS_KL ? pick_c<8, true>(a, n_cus, s) : pick_c<8, false>(a, n_cus, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace evc
