// Microbenchmark: v_mfma_f64_4x4x4_4b_f64 for bins 16 .. 24 of V' += A_j H'_j at M = 25 (k_fused_lone's second bin tile).
// ONE wavefront per SIMD, s_memtime stamps around the timed loop (as mfma_chain_f64.hip and unit_sched.hip).
//
// a. Layout.  One-hot operands: lane la of A and lane lb of B are 1, every lane of D is read back - for all 64 x 64
//    pairs without broadcast, and with cbsz:2 abid:0..3.  The kernel needs the contraction index k in lane bits 4-5,
//        A[i][k] of block b in lane i + 4 b + 16 k,  B[k][j] in lane j + 4 b + 16 k,  D[i][j] in lane j + 4 b + 16 i,
//    so that the resident activations h[r] (lane l: exemplar 4 (l >> 4) + r of frame l & 15, contracted over l >> 4 by the
//    16x16x4 form) serve as B unmoved.  The four blocks are then the frame groups f >> 2, and A has to be the same in all
//    of them: either cbsz:2 abid:r hands block r of ONE fragment to all four (three fragments per unit), or - if the f64
//    form ignores cbsz, which this probe decides - the fragment is read replicated, one per (bin block, exemplar register):
//    twelve ds_read_b64 per unit whose lanes l, l + 4, l + 8, l + 12 share an address.
// b. Cost.  Per "unit", 8 units per repetition, three rounds of every variant:
//      0  twelve 4x4x4 in rotation over three accumulators (r-major, beta inner), alone
//      1  four dependent 16x16x4, alone
//      2  twelve 4x4x4 on ONE accumulator (the dependent issue interval)
//      3  the shipped unit: 6 D MFMAs, the update's f64 vector block, 4 + 4 V' MFMAs, fragments by ds_read_b64
//      4  the new unit, three fragments and cbsz:2 abid:r (timing only where the probe finds cbsz ignored)
//      5  the new unit, twelve replicated fragments read behind the update, no cbsz; the compiler orders reads and MFMAs
//      6  variant 5 with the order fixed: the twelve reads, the four 16x16x4, then the twelve 4x4x4
//    Break-even: 12 c4 < 4 c16, both from this run.  Go: unit 5 (unit 4 where cbsz works) shorter than unit 3 by more
//    than unit 3's range over the three rounds.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/ubench/bin/mfma64_quad tools/ubench/mfma64_quad.hip
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef double f64x4 __attribute__((ext_vector_type(4)));
#define MF(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0)
#define MQ(a, b, c, r) __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 2, r, 0)
#define MQ0(a, b, c) __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0)
#define SB __builtin_amdgcn_sched_barrier(0)
#define NO_PAIR() asm volatile("" ::: "memory")

// ---------------------------------------------------------------------------------------------------------- a. layout
// mode 0: no broadcast; 1 .. 4: cbsz:2 abid:mode-1.  out[(la * 64 + lb) * 64 + lane] = D
__global__ __launch_bounds__(64) void k_probe(int mode, double* out) {
    const int lane = threadIdx.x;
    for (int la = 0; la < 64; ++la)
        for (int lb = 0; lb < 64; ++lb) {
            const double a = lane == la ? 1.0 : 0.0, b = lane == lb ? 1.0 : 0.0;
            double d = 0.0;
            switch (mode) {
                case 0: d = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, 0.0, 0, 0, 0); break;
                case 1: d = MQ(a, b, 0.0, 0); break;
                case 2: d = MQ(a, b, 0.0, 1); break;
                case 3: d = MQ(a, b, 0.0, 2); break;
                default: d = MQ(a, b, 0.0, 3); break;
            }
            out[(la * 64 + lb) * 64 + lane] = d;
        }
}

// the expected D lane of (la, lb), -1: no product.  abid < 0: no broadcast
static int expect(int la, int lb, int abid) {
    const int ia = la & 3, ba = (la >> 2) & 3, ka = la >> 4, jb = lb & 3, bb = (lb >> 2) & 3, kb = lb >> 4;
    if (ka != kb) return -1;
    if (abid < 0 ? ba != bb : ba != abid) return -1;
    return jb + 4 * bb + 16 * ia;
}

// returns 0: the layout the kernel needs and cbsz:2 broadcasts, 1: that layout, cbsz ignored, -1: another layout
static int probe(double* dout) {
    std::vector<double> h(64 * 64 * 64);
    int wrong_total = 0, wrong_plain = 0, wrong_ignored = 0;
    for (int mode = 0; mode < 5; ++mode) {
        hipLaunchKernelGGL(k_probe, dim3(1), dim3(64), 0, 0, mode, dout);
        hipDeviceSynchronize();
        hipMemcpy(h.data(), dout, h.size() * 8, hipMemcpyDeviceToHost);
        int hits = 0, wrong = 0, shown = 0;
        for (int la = 0; la < 64; ++la)
            for (int lb = 0; lb < 64; ++lb) {
                int got = -1, n = 0;
                for (int l = 0; l < 64; ++l)
                    if (h[(la * 64 + lb) * 64 + l] != 0.0) { got = l; ++n; }
                if (n > 1) got = -2;
                hits += n;
                const int want = expect(la, lb, mode - 1);
                if (mode > 0 && got != expect(la, lb, -1)) ++wrong_ignored;
                if (got != want) {
                    ++wrong;
                    if (shown++ < 8) printf("  layout mode %d: A lane %d, B lane %d -> D lane %d (%d lanes), expected %d\n", mode, la, lb, got, n, want);
                }
            }
        if (mode == 0) printf("layout, no broadcast: %d products seen (256 expected), %d pairs off the expected map\n", hits, wrong);
        else printf("layout, cbsz:2 abid:%d: %d products seen (256 expected), %d pairs off the expected map\n", mode - 1, hits, wrong);
        wrong_total += wrong;
        if (mode == 0) wrong_plain = wrong;
    }
    printf("cbsz:2 abid:0..3 against the map WITHOUT broadcast: %d pairs off\n", wrong_ignored);
    if (wrong_plain == 0)
        printf("layout verdict: A in lane i + 4 block + 16 k, B in lane j + 4 block + 16 k, D in lane j + 4 block + 16 i - k in lane bits 4-5: GO\n");
    else
        printf("layout verdict: NOT the layout the kernel needs: NO-GO\n");
    if (wrong_plain == 0 && wrong_total != 0)
        printf("broadcast verdict: %s\n", wrong_ignored == 0 ? "cbsz:2 abid:r is IGNORED by the f64 form (every product is that of no broadcast): A is read replicated, twelve fragments"
                                                              : "cbsz:2 abid:r does something else than broadcast A's block r");
    else if (wrong_plain == 0)
        printf("broadcast verdict: cbsz:2 abid:r hands A's block r to all four blocks: three fragments\n");
    return wrong_plain ? -1 : (wrong_total == 0 ? 0 : (wrong_ignored == 0 ? 1 : -1));
}

// ------------------------------------------------------------------------------------------------------------ b. cost
constexpr int KT = 8, PR = 26, TPD = 16 * PR;

// the update's vector block: range test, batch inversion (one v_rcp_f64 + a Newton step), 8 products, and the next unit's
// lone-bin fold - about 24 f64 instructions in 9 dependent levels (unit_sched.hip's chain)
__device__ __forceinline__ unsigned hi_word(double x) { return (unsigned)(__double_as_longlong(x) >> 32); }
__device__ __forceinline__ unsigned update(double (&h)[4], const f64x4& p, const f64x4& d, unsigned lo) {
    const unsigned worst = max(max(hi_word(d[0]) - lo, hi_word(d[1]) - lo), max(hi_word(d[2]) - lo, hi_word(d[3]) - lo));
    const double a = d[0] * d[1], b = d[2] * d[3], ab = a * b;
    double R = __builtin_amdgcn_rcp(ab);
    const double e = __builtin_fma(-ab, R, 1.0);
    R = __builtin_fma(R, e, R);
    const double Ra = R * b, Rb = R * a;
    h[0] *= p[0] * (Ra * d[1]); h[1] *= p[1] * (Ra * d[0]);
    h[2] *= p[2] * (Rb * d[3]); h[3] *= p[3] * (Rb * d[2]);
    return worst;
}

template <int VARIANT>
__global__ __launch_bounds__(256) void k_cost(int reps, long long* cyc, double* out, unsigned* flag) {
    __shared__ double s_dict[4 * KT * TPD];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int x = threadIdx.x; x < 4 * KT * TPD; x += 256) s_dict[x] = 0.1 + 1e-5 * (x % 97);
    // the kernel's per-lane bases (rows by all_dict_row's pattern: only the bank pattern matters here)
    const int rowA = w * KT * TPD + ((4 * (lane & 3) + ((lane & 15) >> 2)) & 15) * PR;
    const int rowB = w * KT * TPD + (4 * (lane >> 4)) * PR;
    const double* const dA = s_dict + rowA + (lane >> 4);
    const double* const dB = s_dict + rowB + (lane & 15);
    const double* const dBL = s_dict + rowB + min(lane & 15, 25 - 16);
    const double* const dL = s_dict + rowB + 24;
    const int rowQ = w * KT * TPD + (4 * (lane >> 4) + ((lane >> 2) & 3)) * PR;
    const double* const dQ = s_dict + rowQ + 16 + (lane & 3);              // bins 16 .. 23: 4 beta in the immediate
    const double* const dQL = s_dict + rowQ + min(24 + (lane & 3), 25);    // bin 24, or the row's zero slot
    const double* const dR = s_dict + rowB + 16 + (lane & 3);               // replicated: exemplar 4 (l >> 4) + r, r in the immediate
    const double* const dRL = s_dict + rowB + min(24 + (lane & 3), 25);
    double h[KT][4];
    f64x4 p[KT];
    double v[6], vl = 0.5;
    for (int s = 0; s < 6; ++s) v[s] = 0.5 + 1e-3 * s;
    for (int k = 0; k < KT; ++k)
        for (int r = 0; r < 4; ++r) {
            h[k][r] = 1.0 + 1e-3 * (k + r);
            double x = 1.26 + 0.01 * r;          // ~ d: h stays near 1
            asm volatile("" : "+v"(x));
            p[k][r] = x;
        }
    const double d0 = 1e-3;
    const unsigned lo = 0x30500000u;
    unsigned bad = 0;
    double keep = 0.0;
    __syncthreads();
    const long long t0 = __builtin_amdgcn_s_memtime();
    for (int rep = 0; rep < reps; ++rep) {
#pragma unroll
        for (int s = 0; s < 6; ++s) asm volatile("" : "+v"(v[s]));
        f64x4 vn0 = {0, 0, 0, 0}, vn1 = {0, 0, 0, 0};
        double vq[3] = {0.0, 0.0, 0.0};
        if constexpr (VARIANT <= 2) {
            double a[4] = {0.1 + 1e-4 * lane, 0.2, 0.3, 0.4};
#pragma unroll
            for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(a[r]));
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                SB;
                if constexpr (VARIANT == 0) {
#define Q3(r) vq[0] = MQ(a[0], h[k][r], vq[0], r); vq[1] = MQ(a[1], h[k][r], vq[1], r); vq[2] = MQ(a[2], h[k][r], vq[2], r);
                    Q3(0) Q3(1) Q3(2) Q3(3)
                } else if constexpr (VARIANT == 1) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) vn1 = MF(a[r], h[k][r], vn1);
                } else {
#define Q1(r) vq[0] = MQ(a[0], h[k][r], vq[0], r); vq[0] = MQ(a[1], h[k][r], vq[0], r); vq[0] = MQ(a[2], h[k][r], vq[0], r);
                    Q1(0) Q1(1) Q1(2) Q1(3)
                }
                SB;
            }
        } else {
            double a1[6], al[4], a2[4], a3[4], aq[3], ar[3][4];
            f64x4 dl;
            auto load_a1 = [&](int k) {
#pragma unroll
                for (int s = 0; s < 6; ++s) { a1[s] = dA[k * TPD + 16 * (s >> 2) + 4 * (s & 3)]; NO_PAIR(); }
            };
            auto load_lone = [&](int k) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { al[r] = dL[k * TPD + r * PR]; NO_PAIR(); }
            };
            load_a1(0);
            load_lone(0);
#pragma unroll
            for (int r = 0; r < 4; ++r) dl[r] = __builtin_fma(al[r], vl, d0);
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                SB;
#pragma unroll
                for (int r = 0; r < 4; ++r) { a2[r] = dB[k * TPD + r * PR]; NO_PAIR(); }
                if constexpr (VARIANT == 3) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) { a3[r] = dBL[k * TPD + r * PR + 16]; NO_PAIR(); }
                } else if constexpr (VARIANT == 4) {
#pragma unroll
                    for (int b = 0; b < 3; ++b) { aq[b] = b < 2 ? dQ[k * TPD + 4 * b] : dQL[k * TPD]; NO_PAIR(); }
                }
                f64x4 d = dl;
#pragma unroll
                for (int s = 0; s < 6; ++s) d = MF(a1[s], v[s], d);
                if (k + 1 < KT) { load_a1(k + 1); load_lone(k + 1); }
                SB;
                if (k + 1 < KT) {
                    asm volatile("" : "+v"(al[0]), "+v"(al[1]), "+v"(al[2]), "+v"(al[3]));
#pragma unroll
                    for (int r = 0; r < 4; ++r) dl[r] = __builtin_fma(al[r], vl, d0);
                }
                bad |= update(h[k], p[k], d, lo);
                SB;
                if constexpr (VARIANT >= 5) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int b = 0; b < 3; ++b) { ar[b][r] = b < 2 ? dR[k * TPD + r * PR + 4 * b] : dRL[k * TPD + r * PR]; NO_PAIR(); }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) vn0 = MF(a2[r], h[k][r], vn0);
                if constexpr (VARIANT == 3) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) vn1 = MF(a3[r], h[k][r], vn1);
                } else if constexpr (VARIANT >= 5) {
                    if constexpr (VARIANT == 6) SB;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int b = 0; b < 3; ++b) vq[b] = MQ0(ar[b][r], h[k][r], vq[b]);
                } else {
#define Q3U(r) vq[0] = MQ(aq[0], h[k][r], vq[0], r); vq[1] = MQ(aq[1], h[k][r], vq[1], r); vq[2] = MQ(aq[2], h[k][r], vq[2], r);
                    Q3U(0) Q3U(1) Q3U(2) Q3U(3)
                }
            }
        }
        SB;
        // renormalise so that the values stay finite whatever the variant computes
#pragma unroll
        for (int k = 0; k < KT; ++k)
#pragma unroll
            for (int r = 0; r < 4; ++r) h[k][r] = h[k][r] > 2.0 ? 1.0 : (h[k][r] < 0.5 ? 1.0 : h[k][r]);
        keep += vn0[0] + vn0[3] + vn1[1] + vn1[2] + vq[0] + vq[1] + vq[2];
        v[0] += keep * 1e-300;
    }
    const long long t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0) cyc[blockIdx.x * 4 + w] = t1 - t0;
    double s = v[0] + keep;
    for (int k = 0; k < KT; ++k) s += h[k][0] + h[k][1] + h[k][2] + h[k][3];
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = s;
    if (bad == 0xFFFFFFFFu) *flag = 1;
}

template <int VARIANT>
static double run(const char* name, int reps, int round, long long* cyc, double* out, unsigned* flag) {
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL((k_cost<VARIANT>), dim3(256), dim3(256), 0, 0, reps, cyc, out, flag);
    hipEventRecord(e0);
    hipLaunchKernelGGL((k_cost<VARIANT>), dim3(256), dim3(256), 0, 0, reps, cyc, out, flag);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    std::vector<long long> hc(256 * 4);
    hipMemcpy(hc.data(), cyc, hc.size() * 8, hipMemcpyDeviceToHost);
    std::vector<double> per;
    for (long long c : hc) per.push_back((double)c / ((double)reps * KT));
    std::sort(per.begin(), per.end());
    const double med = per[per.size() / 2];
    printf("round %d  %-64s %8.1f ticks per unit (median of 1024 wavefronts; min %.1f max %.1f)  kernel %.3f ms = %.1f cycles per unit at 2.4 GHz\n",
           round, name, med, per.front(), per.back(), ms, ms * 1e-3 * 2.4e9 / ((double)reps * KT));
    hipEventDestroy(e0); hipEventDestroy(e1);
    return med;
}

int main(int argc, char** argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 2000;
    long long* cyc; double* out; unsigned* flag;
    if (hipMalloc(&cyc, 256 * 4 * 8) != hipSuccess || hipMalloc(&out, 64 * 64 * 64 * 8) != hipSuccess || hipMalloc(&flag, 4) != hipSuccess) {
        printf("no device memory\n");
        return 1;
    }
    const int layout = probe(out);
    double t[7][3];
    for (int round = 0; round < 3; ++round) {
        t[0][round] = run<0>("0 twelve 4x4x4, three accumulators in rotation, alone", reps, round, cyc, out, flag);
        t[1][round] = run<1>("1 four dependent 16x16x4, alone", reps, round, cyc, out, flag);
        t[2][round] = run<2>("2 twelve 4x4x4 on one accumulator, alone", reps, round, cyc, out, flag);
        t[3][round] = run<3>("3 shipped unit: 6 D | update | 4 + 4 V' (14 x 16x16x4)", reps, round, cyc, out, flag);
        t[4][round] = run<4>("4 new unit, 3 fragments + cbsz: 6 D | update | 4 V' + twelve 4x4x4", reps, round, cyc, out, flag);
        t[5][round] = run<5>("5 new unit, 12 replicated fragments: 6 D | update | 4 V' + twelve", reps, round, cyc, out, flag);
        t[6][round] = run<6>("6 new unit, 12 replicated fragments, 12 reads | 4 V' | twelve", reps, round, cyc, out, flag);
    }
    auto lo = [&](int v) { return std::min(t[v][0], std::min(t[v][1], t[v][2])); };
    auto hi = [&](int v) { return std::max(t[v][0], std::max(t[v][1], t[v][2])); };
    auto md = [&](int v) { return t[v][0] + t[v][1] + t[v][2] - lo(v) - hi(v); };
    const double c4 = md(0) / 12.0, c16 = md(1) / 4.0;
    printf("c4 = %.2f ticks (rotation), %.2f (dependent); c16 = %.2f: 12 c4 = %.1f against 4 c16 = %.1f\n", c4, md(2) / 12.0, c16, 12 * c4, 4 * c16);
    const int nv = layout == 0 ? 4 : (md(6) < md(5) ? 6 : 5);
    const double gain = md(3) - md(nv), range = hi(3) - lo(3);
    printf("shipped unit %.1f (range %.1f over three rounds), new unit (variant %d) %.1f (range %.1f): %.1f ticks per unit shorter\n", md(3), range, nv,
           md(nv), hi(nv) - lo(nv), gain);
    printf("verdict: %s\n", layout >= 0 && gain > range && gain > 0 ? "GO" : "NO-GO");
    return 0;
}
