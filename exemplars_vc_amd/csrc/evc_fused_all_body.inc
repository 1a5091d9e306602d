// The text of k_fused_all, k_fused_lone and k_fused_quad (evc_fused_all.hip includes this file once for each, EVC_ALL_LONE
// 0 / 1 / 2).
// LONE (k_fused_lone only, M == 4 MSTEPS - 3): the last k-step of D = A_j^T V and of P = A_j^T X would multiply one real
// bin, BL = M - 1, and three zero slots.  It is not issued: the bin enters the accumulator's start value instead,
//   d[r] = fma(A[BL, e_r], V[BL, f], d0)   and   p[r] = A[BL, e_r] X[BL, f]        (e_r: the lane's four exemplars, f: its frame)
// and DS = MSTEPS - 1 MFMAs follow; a1[], v[] and x[] hold DS k-steps.  A[BL, e_r] (a24 at M = 25) are four ds_read_b64
// from the V'-order rows of s_dict, fetched with the unit's D fragments; V[BL, f] is lane f of the last k-step's image.
// The four FMAs of a unit stand in the update of the unit before it (see the sweep), not in front of its own D chain.
// V' keeps all its MFMAs (the bins from 16 on need the second row tile), and so do the exchange, the tile end and the Y pass.
//
// QUAD (k_fused_quad only: k_fused_lone but for the sweep's V' part): the second row tile of V' holds M - 16 = 9 real bins and
// 7 rows of zeros.  Its four v_mfma_f64_16x16x4_f64 per unit are replaced by twelve v_mfma_f64_4x4x4_4b_f64, whose rows come
// in fours: NQ = 3 bin blocks (16 .. 19, 20 .. 23, 24 and three zero slots) x 4 exemplar registers.  The instruction
// computes four independent 4 x 4 x 4 products; with A[i][k] of block b in lane i + 4 b + 16 k, B[k][j] in lane
// j + 4 b + 16 k and D[i][j] in lane j + 4 b + 16 i (tools/ubench/mfma64_quad.hip, profiles/quad_rows_ubench.txt) the
// contraction runs over the lane groups as in the 16x16x4 form, so h[k][r] is the B operand as it stands, the blocks are the
// frame groups f >> 2, and lane l of accumulator beta holds V'[16 + 4 beta + (l >> 4)][frame l & 15]: element l of k-step image
// 4 + beta of the B-operand order, the slot the second tile's accumulator register beta filled.  A has to be the same in all
// four blocks.  The f64 form ignores cbsz / abid (the same record), so the fragment is READ replicated: aq[beta][r], lane l:
// A[min(16 + 4 beta + (l & 3), M)][exemplar 4 (l >> 4) + r], lanes l, l + 4, l + 8, l + 12 sharing an address - twelve
// ds_read_b64 per unit in place of four, issued behind the update, where its temporaries are dead.
//
// KL: the generalised Kullback-Leibler update (sklearn _nmf.py:557-606 with update_H=False): A1p then holds the
// dictionary divided by its column sums, the sweep's B operand is R = X / max(V, eps) instead of V, the update is
// h <- h * (A~_j^T R) - no numerator tiles, no division in the sweep - and R is formed where V is combined.
#if EVC_ALL_LONE
template <int MSTEPS, int C>
#if EVC_ALL_LONE == 2
__global__ __launch_bounds__(ATHREADS, 2) void k_fused_quad(FusedArgs a) {
    constexpr bool QUAD = true;
#else
__global__ __launch_bounds__(ATHREADS, 2) void k_fused_lone(FusedArgs a) {
    constexpr bool QUAD = false;
#endif
    constexpr bool KL = false, LONE = true;
    static_assert(MSTEPS > 4 && C > 1 && AllShape<MSTEPS, C, false>::LDS_DICT, "two bin tiles, the dictionary in LDS, direct exchange");
#else
template <int MSTEPS, int C, bool KL>
__global__ __launch_bounds__(ATHREADS, 2) void k_fused_all(FusedArgs a) {
    constexpr bool LONE = false, QUAD = false;
#endif
    using S = AllShape<MSTEPS, C, KL>;
    constexpr int DS = LONE ? MSTEPS - 1 : MSTEPS;   // k-steps of the D and P chains
    // the update's range test decided once per sweep (mu_tile_hoisted, evc_fused_common.h): the instances whose step is
    // the sweep - one member and the direct exchange, Frobenius.  The reduce-scatter instances (their step is the
    // exchange) and KL (no division) keep their code.
    constexpr bool HOIST = !KL && C >= 1;
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
    // HOIST: [half][w] - did every element of V that wavefront w of the half wrote in the last exchange lie in
    // [2^-100, 2^100)?  Written by its owner alone (no atomics), 0 from the tile's start to its first exchange.
    __shared__ __attribute__((aligned(16))) unsigned s_vok[HOIST ? 2 : 1][HOIST ? AW : 1];
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
    const double* const dL = s_dict + rowB + BL;      // LONE: bin BL of the lane's four exemplars (16-lane broadcasts)
    // QUAD: bins 16 (MT - 1) + 4 beta + (lane & 3) of the lane group's exemplars, beta in the immediate; the last block (bin BL
    // and the row's zero slot M, never the next row) has a base of its own
    constexpr int MTL = QUAD ? MT - 1 : MT;           // bin tiles of V' on 16x16x4 MFMAs
    constexpr int NQ = QUAD ? MSTEPS - 4 * MTL : 0;   // bin blocks of four on 4x4x4 MFMAs
    const double* const dQ = s_dict + rowB + 16 * MTL + (lane & 3);
    const double* const dQL = s_dict + rowB + min(BL + (lane & 3), a.M);
    // `lds`: std::true_type - fragments from s_dict, std::false_type - buffer loads from A1p / A2p.  (The compiler would
    // pair reads off one address into ds_read2_b64: 8 LDS cycles for 16-lane groups, where this layout is 2-way
    // conflicted, against 2 x 2 for two ds_read_b64 - an empty asm with a memory clobber between the reads keeps them apart.)
#define LDS_NO_PAIR() asm volatile("" ::: "memory")
    auto load_a1 = [&](double (&a1)[DS], int k, auto lds) {
        if constexpr (decltype(lds)::value) {
#pragma unroll
            for (int s = 0; s < DS; ++s) {
                a1[s] = (s == MSTEPS - 1 ? dAL : dA)[k * TPD + 16 * (s >> 2) + 4 * (s & 3)];
                LDS_NO_PAIR();
            }
            return;
        }
        if constexpr (!LONE) {
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
        }
    };
    auto load_lone = [&](double (&al)[4], int k) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            al[r] = dL[k * TPD + r * PR];
            LDS_NO_PAIR();
        }
    };
    auto load_a2 = [&](double (&a2)[MT][4], int k, auto lds) {
        if constexpr (decltype(lds)::value) {
#pragma unroll
            for (int u = 0; u < MTL; ++u)
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
    auto load_aq = [&](double (&aq)[NQ > 0 ? NQ : 1][4], int k) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int b = 0; b < NQ; ++b) {
                aq[b][r] = b < NQ - 1 ? dQ[k * TPD + r * PR + 4 * b] : dQL[k * TPD + r * PR];
                LDS_NO_PAIR();
            }
    };

    const int mode = a.eps_mode;
    const double eps = a.eps;
    const double d0 = a.l1 + (mode == EVC_EPS_ADD ? a.eps : 0.0);
    const f64x4 dinit = {d0, d0, d0, d0};
    const unsigned lo = fast_lo(mode, eps);
    unsigned seq = 0;                            // exchanges done by this half's group so far
    bool tame = false;                           // HOIST: the member's bound, found once per launch (below, in front of run)
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
    // QUAD, the same in every exchange of the launch and kept as lane masks: the lanes that watch a peer's word (lane m <->
    // member m), and the lanes whose pair of elements lies in a real bin (both elements lie in one lane group of one k-step;
    // bins >= M hold exact zeros)
    unsigned long long xq_peers = 0, xq_real = 0;
    if constexpr (QUAD) {
        xq_peers = __builtin_amdgcn_ballot_w64(lane < C && lane != member);
        xq_real = __builtin_amdgcn_ballot_w64(th < NE / 2 && bin_of((2 * th) >> 6, ((2 * th) & 63) >> 4) < a.M);
        asm volatile("" : "+s"(xq_peers), "+s"(xq_real));
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
        double a1[DS], a2[MT][4], al[4];
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
        if constexpr (HOIST) {                   // a tile's first sweep keeps the per-unit test
            if (lane == 0) s_vok[half][w] = 0u;
        }
        __syncthreads();
        if (valid && !KL) {                      // numerator tiles, once per frame tile
            double x[DS], xl = 0.0;
#pragma unroll
            for (int s = 0; s < DS; ++s) x[s] = xL[s * 64 + lane];
            if constexpr (LONE) xl = xL[DS * 64 + (lane & 15)];
            load_a1(a1, 0, lds);
            if constexpr (LONE) load_lone(al, 0);
#pragma unroll
            for (int k = 0; k < AKT; ++k) {
                f64x4 acc = {0, 0, 0, 0};
                if constexpr (LONE) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] = al[r] * xl;
                }
#pragma unroll
                for (int s = 0; s < DS; ++s) acc = Mma<double>::mma(a1[s], x[s], acc);
                if (!decltype(lds)::value || k + 1 < AKT) load_a1(a1, (k + 1) % AKT, lds);
                if constexpr (LONE) {
                    if (k + 1 < AKT) load_lone(al, k + 1);
                }
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
                double v[DS], vl = 0.0;
#pragma unroll
                for (int s = 0; s < DS; ++s) {
                    v[s] = KL ? rL[s * 64 + lane] : vL[s * 64 + lane];
                    // (two k-steps, dictionary in LDS, HOIST: the compiler lays this sweep straight behind the numerator
                    // pass, and tests/test_fused_all_lds_host.py, which takes MFMAs less than 200 lines apart for one run,
                    // then counts the sweep's head with the sweep: no paired read here either)
                    if constexpr (HOIST && MSTEPS == 2 && decltype(lds)::value) LDS_NO_PAIR();
                }
                if constexpr (LONE) vl = vL[DS * 64 + (lane & 15)];
                // HOIST: one scalar for the sweep's 8 units - the member is tame and the half's four wavefronts found
                // every element of this V in range (read behind the step barrier that orders the v[] reads above)
                bool safe = false;
                if constexpr (HOIST) {
                    static_assert(AW == 4, "the half's four words are one 16-byte read");
                    const all_u32x4 ok4 = *reinterpret_cast<const all_u32x4*>(s_vok[half]);
                    safe = tame && __builtin_amdgcn_readfirstlane((int)(ok4[0] & ok4[1] & ok4[2] & ok4[3])) != 0;
                }
                // (from LDS the first unit's fragments come at the start of the sweep: held across the exchange step
                // instead, they cost 14 registers there, and the compiler spilled around the sweep)
                if constexpr (decltype(lds)::value) load_a1(a1, 0, lds);
                // LONE: the start value of a unit's D chain is formed with the update of the unit before it (the first one
                // here): a vector instruction between the V' MFMAs and the next D chain would break their back-to-back
                // issue a second time per unit, which costs what the dropped MFMA saves (profiles/lone_bin_README.md)
                f64x4 dl = dinit;
                if constexpr (LONE) {
                    load_lone(al, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) dl[r] = __builtin_fma(al[r], vl, d0);
                }
                EVC_STAMP(3);                    // (stamps build: the sweep's head ends here)
                f64x4 vn[MT];
#pragma unroll
                for (int u = 0; u < MT; ++u) vn[u] = f64x4{0, 0, 0, 0};
                double vq[NQ > 0 ? NQ : 1] = {};     // QUAD: V' of the bin blocks 16 MTL + 4 beta ..
#pragma unroll
                for (int k = 0; k < AKT; ++k) {
                    __builtin_amdgcn_sched_barrier(0);
                    load_a2(a2, k, lds);
                    f64x4 d = KL ? f64x4{0, 0, 0, 0} : (LONE ? dl : dinit);
#pragma unroll
                    for (int s = 0; s < DS; ++s) d = Mma<double>::mma(a1[s], v[s], d);
                    if (!decltype(lds)::value || k + 1 < AKT)
                        load_a1(a1, (k + 1) % AKT, lds);  // the next unit's (streamed: or the next sweep's first) fragments
                    if constexpr (LONE) {
                        if (k + 1 < AKT) load_lone(al, k + 1);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    if constexpr (LONE) {
                        if (k + 1 < AKT) {
                            // (the four words waited for together: one s_waitcnt in front of the fold, not one per FMA)
                            asm volatile("" : "+v"(al[0]), "+v"(al[1]), "+v"(al[2]), "+v"(al[3]));
#pragma unroll
                            for (int r = 0; r < 4; ++r) dl[r] = __builtin_fma(al[r], vl, d0);
                        }
                    }
                    if (KL) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) h[k][r] *= d[r];
                    } else if constexpr (HOIST) {
                        mu_tile_hoisted(h[k], p[k], d, mode, eps, lo, safe);
                    } else {
                        mu_tile_guarded(h[k], p[k], d, mode, eps, lo);
                    }
                    // One vector phase per unit: the update is closed towards the V' MFMAs as well.  Left open, the
                    // compiler sinks the last h *= q behind the first V' MFMA and the next unit's fold behind the third - two
                    // more MFMA <-> vector switches per unit (profiles/step_chain_README.md).  Not in the reduce-scatter
                    // instances: their step is the exchange, which shares its SIMDs with this sweep, and with the MFMAs
                    // packed tighter C5 (32 members) ran 0.8 % slower - they keep the order the compiler chooses.
                    if constexpr (C >= 1) __builtin_amdgcn_sched_barrier(0);
                    [[maybe_unused]] double aq[NQ > 0 ? NQ : 1][4];
                    if constexpr (QUAD) load_aq(aq, k);
#pragma unroll
                    for (int u = 0; u < MTL; ++u)
#pragma unroll
                        for (int r = 0; r < 4; ++r) vn[u] = Mma<double>::mma(a2[u][r], h[k][r], vn[u]);
                    if constexpr (QUAD) {
                        // r-major, rotating over the blocks: an accumulator comes round every third instruction
#pragma unroll
                        for (int r = 0; r < 4; ++r)
#pragma unroll
                            for (int b = 0; b < NQ; ++b)
                                vq[b] = __builtin_amdgcn_mfma_f64_4x4x4f64(aq[b][r], h[k][r], vq[b], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int u = 0; u < MTL; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (u * 4 + r < MSTEPS) red[w * RSTR + (u * 4 + r) * 64 + lane] = vn[u][r];
                if constexpr (QUAD) {
#pragma unroll
                    for (int b = 0; b < NQ; ++b) red[w * RSTR + (4 * MTL + b) * 64 + lane] = vq[b];
                }
            } else if (QUAD && valid && !mine && step > 0) {
                // ---------------- k_fused_quad's exchange: the protocol of the next branch - buffers, offsets, 16-byte words,
                // one epoch bit per 8-byte half, watch phase, bounded polls, s_fail, the sums' orders - with the vector
                // instructions that the result does not need taken out (an f64 MFMA and a vector instruction of one SIMD do
                // not overlap: every one of them is time of the sweep beside it; profiles/lean_exchange_README.md):
                //  * every fetch round loads ALL C slots, the thread's own included.  The thread stored that word earlier in
                //    this exchange; a stale one carries the other epoch and is fetched again like a peer's, so nothing new
                //    rests on ordering.  No slot is zeroed or filled from registers first and nothing branches on `member`;
                //  * the epoch is wave-uniform, so the tag test is one chain per epoch value, two low words per three-input
                //    instruction: the OR of the words (epoch 0) or of their complements (epoch 1), then one test of bit 0.
                //    Each 8-byte half is still checked by itself;
                //  * the words are tagged and tested as 32-bit halves, the watched word comes through the exchange's buffer
                //    resource (its lane offset is the same in every exchange), and "every lane" is a test of the mask.
                constexpr int CQ = C > 0 ? C : 1;
                __builtin_amdgcn_s_setprio(ALL_EXCH_PRIO);
                const bool act = th < NE / 2;
                const int ep = act ? 2 * th : 0;
                unsigned vok = 1u;                  // (a wavefront that moves nothing vouches for nothing)
                if (w * 64 < NE / 2) {
                    f64x2 pv[AW], sm = {0.0, 0.0};
#pragma unroll
                    for (int ww = 0; ww < AW; ++ww) pv[ww] = *reinterpret_cast<const f64x2*>(red + ww * RSTR + ep);
                    static_assert(AW == 4, "the four partials are named one by one");
                    asm volatile("" : "+v"(pv[0]), "+v"(pv[1]), "+v"(pv[2]), "+v"(pv[3]));
#pragma unroll
                    for (int ww = 0; ww < AW; ++ww) sm += pv[ww];
                    unsigned tag = (seq >> 1) & 1;               // a buffer is reused every second exchange
                    all_u32x4 pw = __builtin_bit_cast(all_u32x4, sm);
                    pw[0] = (pw[0] & ~1u) | tag;
                    pw[2] = (pw[2] & ~1u) | tag;
                    const int xo = __builtin_amdgcn_readfirstlane((int)(((seq & 1) * (unsigned)a.groups + (unsigned)g) * (unsigned)(C * 4096)));
                    if (act) __builtin_amdgcn_raw_buffer_store_b128(pw, rx, ep * 8, xo + member * 4096, 16);
                    bool ok = true;
                    unsigned polls = 0;
                    // watch one word per peer (lane m <-> member m), as below
                    const int wo = (lane < C ? lane : 0) * 4096 + (NE - 1) * 8;
                    for (;;) {
                        asm volatile("" ::: "memory");      // (the builtin load is not volatile: it stays in the loop)
                        all_u32x2 b = __builtin_amdgcn_raw_buffer_load_b64(rx, wo, xo, 16);
                        asm volatile("" : "+v"(b));         // (the 8-byte word as the peer stored it, not its low half alone)
                        if ((__builtin_amdgcn_ballot_w64(((b[0] ^ tag) & 1) != 0) & xq_peers) == 0) break;
                        if (all_polls_out(polls, a.coop_abort)) {
                            ok = false;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(2);
                    }
                    // (no fetch round - a launch being voided, a thread without a pair: any value will do, at no instruction)
                    all_i64x2 b[CQ];
#pragma unroll
                    for (int m = 0; m < CQ; ++m) asm volatile("" : "=v"(b[m]));
                    unsigned rounds = 0;
                    while (__builtin_expect(ok && act, 1)) {        // (runs at least once: laid out in line)
                        asm volatile("" ::: "memory");      // (the builtin load is not volatile: it stays in the loop)
#pragma unroll
                        for (int m = 0; m < CQ; ++m)
                            b[m] = __builtin_bit_cast(all_i64x2, __builtin_amdgcn_raw_buffer_load_b128(rx, ep * 8, xo + m * 4096, 16));
                        unsigned stale = 0;
                        if (tag) {
#pragma unroll
                            for (int m = 0; m < CQ; ++m) stale |= ~(unsigned)b[m][0] | ~(unsigned)b[m][1];
                        } else {
#pragma unroll
                            for (int m = 0; m < CQ; ++m) stale |= (unsigned)b[m][0] | (unsigned)b[m][1];
                        }
                        if ((stale & 1) == 0) break;
                        // (the threads still fetching have all counted the same rounds)
                        unsigned r = __builtin_amdgcn_readfirstlane(rounds);
                        const bool out = all_polls_out(r, a.coop_abort);
                        rounds = r;
                        if (out) {
                            ok = false;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(2);
                    }
                    f64x2 v2 = {0.0, 0.0};
#pragma unroll
                    for (int m = 0; m < CQ; ++m) {                // member order: identical on every member
                        v2[0] += __longlong_as_double(b[m][0] & ~1LL);
                        v2[1] += __longlong_as_double(b[m][1] & ~1LL);
                    }
                    if (!ok) s_fail = 1;
                    vok = (__builtin_amdgcn_ballot_w64(!(range_v_ok(v2[0]) && range_v_ok(v2[1]))) & xq_real) == 0 ? 1u : 0u;
                    if (act) *reinterpret_cast<f64x2*>(vL + ep) = v2;
                }
                if (lane == 0) s_vok[half][w] = vok;
                ++seq;
                __builtin_amdgcn_s_setprio(0);
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
                unsigned vok = 1u;                  // (a wavefront that moves nothing vouches for nothing)
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
                    if constexpr (HOIST) {
                        // the pair's bin (both elements lie in one lane group of one k-step); bins >= M hold exact zeros
                        const bool real = act && bin_of(ep >> 6, (ep & 63) >> 4) < a.M;
                        vok = __all(!real || (range_v_ok(v2[0]) && range_v_ok(v2[1]))) ? 1u : 0u;
                    }
                    if (act) {
                        *reinterpret_cast<f64x2*>(vL + ep) = v2;
                        if (KL) {
                            const f64x2 x2 = *reinterpret_cast<const f64x2*>(xL + ep);
                            *reinterpret_cast<f64x2*>(rL + ep) =
                                f64x2{x2[0] / (v2[0] < a.eps ? a.eps : v2[0]), x2[1] / (v2[1] < a.eps ? a.eps : v2[1])};
                        }
                    }
                }
                if constexpr (HOIST) {
                    if (lane == 0) s_vok[half][w] = vok;
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
                if constexpr (HOIST) {               // (one member: threads from NE on write slots that nothing reads)
                    const bool real0 = e0 < NE && bin_of(e0 >> 6, (e0 & 63) >> 4) < a.M;
                    const bool real1 = has1 && bin_of(e1 >> 6, (e1 & 63) >> 4) < a.M;
                    const unsigned vok = __all((!real0 || range_v_ok(s0)) && (!real1 || range_v_ok(s1))) ? 1u : 0u;
                    if (lane == 0) s_vok[half][w] = vok;
                }
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

    if constexpr (HOIST) {
        // tame (mu_tile_hoisted): one thread per exemplar of the member, its M bins from A2p (the values the LDS dictionary
        // and A1p hold as well), once per launch
        static_assert(ATHREADS == 16 * ATILES, "one thread per exemplar of the member");
        const long j = (long)member * ATILES + (tid >> 4);
        const int e = tid & 15, q = e >> 2, r = e & 3;
        bool ok = a.range_hoist != 0 && a.M > 0 && a.M <= 16 * MT && 16 * j + e < a.N && d0 >= 0.0 && d0 <= RANGE_SUM_HI &&
                  lo <= RANGE_LO_MAX;
        if (ok) {
            double cs = 0.0;
            for (int b = 0; b < a.M; ++b) {
                const double x = A2p[((j * MT + (b >> 4)) * 2 + (r >> 1)) * 128 + (16 * q + (b & 15)) * 2 + (r & 1)];
                ok = ok && x >= 0.0;             // (a NaN fails here, an infinity at the sum)
                cs += x;
            }
            ok = ok && cs >= RANGE_SUM_LO && cs <= RANGE_SUM_HI;
        }
        tame = __builtin_amdgcn_readfirstlane(__syncthreads_and(ok)) != 0;
    }
    if constexpr (S::LDS_DICT) {
        if (LONE ? a.M == 4 * MSTEPS - 3 : (a.M > 0 && a.M < PR)) {
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
    if constexpr (!LONE) run(std::false_type{});
}
