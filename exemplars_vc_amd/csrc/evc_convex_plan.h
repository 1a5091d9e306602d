// evc_convex_plan.h - what evc_convex_learn decides on the host before its launches: the limits, the argument checks in the
// order of their statuses, convex_plan() (row-block width and k-splits of k_convex_sweep) and the workspace carving.  No
// device code: tests/convex_host_main.hip, a program of its own, includes it and runs it under the host sanitizers
// (tests/test_convex_host.py).
#pragma once
#include "evc_internal.h"

namespace evc {

constexpr int CONVEX_MAX_M = 1056;       // LEARN_MAX_M: M is only a contraction length here
constexpr int CONVEX_MAX_T = 16384;      // the Gram matrix is T x T: 2 GiB in float64 at this T
constexpr int CONVEX_MAX_R = 1024;
constexpr int CONVEX_MAX_SLOTS = MAX_SLOTS;
constexpr int CONVEX_MAX_WAVES = 8;      // wavefronts per workgroup of k_convex_sweep, each owning 16 exemplar rows
constexpr int CONVEX_MIN_WAVES = 2;
constexpr int CONVEX_BN = 16 * CONVEX_MAX_WAVES;     // rows of the widest workgroup; K is padded to a multiple in both directions
constexpr int CONVEX_BR = 64;            // columns (of G or H^T) per workgroup
constexpr int CONVEX_KS = 16;            // exemplars per k-slab
constexpr int CONVEX_MAX_S = 16;         // k-ranges per sweep (slabs of partial sums in the workspace)
constexpr int CONVEX_FILL_WGS = 512;     // two workgroups per compute unit of a 256-CU part
constexpr int CONVEX_MIN_SLABS = 4;      // k-slabs a range holds at least where the plan splits by itself

// The geometry of k_convex_sweep for a T x T Gram matrix against R columns: W wavefronts (16 W rows) per workgroup and S
// contiguous k-ranges.  S is what brings the grid to CONVEX_FILL_WGS workgroups, never ranges shorter than
// CONVEX_MIN_SLABS slabs and at most CONVEX_MAX_S of them; W is the widest row block that gets there within that cap,
// else the narrowest.  Splitting k comes first and narrowing second because that is what was measured (DESIGN.md §5.21:
// at equal workgroup counts 128-row blocks with more ranges beat narrower blocks, whose wavefronts share a slab of B among
// fewer of them).  A function of (T, R) alone, never of the device.  With S = 1 an output's bits do not depend on W: every
// wavefront runs the same k-ascending chain over all of T.
struct ConvexPlan {
    int W, S;
};
inline long convex_workgroups(int T_, int R, int W) {
    return (long)(round_up(T_, CONVEX_BN) / (16 * W)) * ((R + CONVEX_BR - 1) / CONVEX_BR);
}
inline ConvexPlan convex_plan(int T_, int R) {
    long cap = (((long)T_ + CONVEX_KS - 1) / CONVEX_KS) / CONVEX_MIN_SLABS;
    if (cap > CONVEX_MAX_S) cap = CONVEX_MAX_S;
    if (cap < 1) cap = 1;
    for (int W = CONVEX_MAX_WAVES; W >= CONVEX_MIN_WAVES; W /= 2) {
        const long wgs = convex_workgroups(T_, R, W), S = (CONVEX_FILL_WGS + wgs - 1) / wgs;
        if (S <= cap) return ConvexPlan{W, (int)S};
    }
    return ConvexPlan{CONVEX_MIN_WAVES, (int)cap};
}

// k-ranges of the R x R products that contract over all of T (k_convex_rr): what brings their ceil(R / 64)^2 tiles to 256
// workgroups, at most CONVEX_RR_MAX_Z ranges of at least CONVEX_MIN_SLABS slabs.  A function of (T, R) alone.
constexpr int CONVEX_RR_MAX_Z = 64;
inline int convex_rr_splits(int T_, int R) {
    const long tiles = (long)((R + 63) / 64) * ((R + 63) / 64);
    long Z = (256 + tiles - 1) / tiles, cap = (((long)T_ + CONVEX_KS - 1) / CONVEX_KS) / CONVEX_MIN_SLABS;
    if (cap > CONVEX_RR_MAX_Z) cap = CONVEX_RR_MAX_Z;
    if (Z > cap) Z = cap;
    return Z < 1 ? 1 : (int)Z;
}

inline bool convex_sizes_ok(int M, int R, int T_) {
    return M >= 1 && M <= CONVEX_MAX_M && T_ >= 1 && T_ <= CONVEX_MAX_T && R >= 1 && R <= CONVEX_MAX_R && R <= T_;
}

struct ConvexWs {
    char* K;            // [TP][TP] elements, TP = round_up(T, CONVEX_BN): X^T X, zero in the padding
    char* Np;           // [T][R] elements: pos(K) G
    char* Nn;           // [T][R]: neg(K) G
    char* Q1;           // [T][R]: H^T Sn, then Nn C
    char* Q2;           // [T][R]: H^T Sp, then Np C
    char* part;         // [S][2][T][R]: the k-ranges' partial sums (S > 1)
    char* rrpart;       // [Z][R][R]: the k-ranges' partial sums of an R x R product (Z = convex_rr_splits > 1)
    char* Sp;           // [R][R]: G^T Np, then C = H H^T
    char* Sn;           // [R][R]: G^T Nn
    char* Wm;           // [M][R]: X G at a check
    char* V;            // [T][M]: W H at a check
    double* err2;       // [T]: every exemplar's squared residual
    double* trace;      // [CONVEX_MAX_SLOTS]
    double* eprev;      // [1]
    int* stop;          // [1]: 0 running, else the iteration the loop stopped at
    size_t bytes;
};

// [K | Np | Nn | Q1 | Q2 | part | rrpart | Sp | Sn | Wm | V | err2 | trace | eprev | stop], each 256-byte aligned (ws == NULL: sizes only)
inline ConvexWs carve_convex(void* ws, int M, int R, int T_, int S, int dtype) {
    ConvexWs w;
    Carver c = Carver::rounded(ws);
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t TP = (size_t)round_up(T_, CONVEX_BN), tr = (size_t)T_ * R * es;
    w.K = c.take<char>(TP * TP * es);
    w.Np = c.take<char>(tr);
    w.Nn = c.take<char>(tr);
    w.Q1 = c.take<char>(tr);
    w.Q2 = c.take<char>(tr);
    w.part = c.take<char>(S > 1 ? 2 * (size_t)S * tr : 0);
    const int Z = convex_rr_splits(T_, R);
    w.rrpart = c.take<char>(Z > 1 ? (size_t)Z * R * R * es : 0);
    w.Sp = c.take<char>((size_t)R * R * es);
    w.Sn = c.take<char>((size_t)R * R * es);
    w.Wm = c.take<char>((size_t)M * R * es);
    w.V = c.take<char>((size_t)T_ * M * es);
    w.err2 = c.take<double>((size_t)T_);
    w.trace = c.take<double>((size_t)CONVEX_MAX_SLOTS);
    w.eprev = c.take<double>(1);
    w.stop = c.take<int>(1);
    w.bytes = c.bytes();
    return w;
}

// with the plan's own S; a forced S beyond it needs 2 (S - S_plan) T R elements more (S <= 1 counts as 1)
inline size_t convex_workspace_bytes(int M, int R, int T_, int dtype, int S = 0) {
    if (!convex_sizes_ok(M, R, T_) || (dtype != EVC_F64 && dtype != EVC_F32)) return 0;
    return carve_convex(nullptr, M, R, T_, S > 0 ? S : convex_plan(T_, R).S, dtype).bytes + 256;
}

// evc_convex_learn's argument checks, in the order of its statuses: ST_BADARG, ST_UNSUPPORTED, ST_WORKSPACE before any
// device work.  *plan_out: what the call runs with - convex_plan's choice, or the k-ranges forced by bits 8..15 of `reserved`
// and the wavefronts per workgroup forced by bits 16..23 (tuning and tests).
inline int convex_args_check(const void* X, int ldx, const void* G, int ldg, const void* H, int ldh, const void* W, int ldw,
                             int M, int R, int T_, const evc_convex_opts* opts, const void* workspace, size_t workspace_bytes,
                             ConvexPlan* plan_out) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_convex_opts)) return ST_BADARG;
    const evc_convex_opts& o = *opts;
    const int forced = (o.reserved >> 8) & 0xff, forced_w = (o.reserved >> 16) & 0xff;
    if (M < 1 || R < 1 || T_ < 1 || (o.dtype != EVC_F64 && o.dtype != EVC_F32)) return ST_BADARG;
    if (o.layout != EVC_FRAME_MAJOR && o.layout != EVC_BIN_MAJOR) return ST_BADARG;
    if ((o.reserved & ~0xffff00) != 0 || forced > CONVEX_MAX_S) return ST_BADARG;
    if (forced_w != 0 && forced_w != 2 && forced_w != 4 && forced_w != 8) return ST_BADARG;
    if (o.update != EVC_CONVEX_BOTH && o.update != EVC_CONVEX_H_ONLY && o.update != EVC_CONVEX_G_ONLY) return ST_BADARG;
    if (o.iters < 0 || o.check_every < 0) return ST_BADARG;
    if (!(o.tol >= 0.0) || !(o.eps >= 0.0) || !(o.eps - o.eps == 0.0)) return ST_BADARG;
    if (!X || !G || !H || !workspace) return ST_BADARG;
    if (bad_ld(o.layout, ldx, T_, M) || bad_ld(o.layout, ldh, T_, R) || ldg < R) return ST_BADARG;
    if (W && bad_ld(o.layout, ldw, R, M)) return ST_BADARG;
    if (o.check_every > 0 && o.iters / o.check_every + 1 > CONVEX_MAX_SLOTS) return ST_BADARG;
    if (!convex_sizes_ok(M, R, T_)) return ST_UNSUPPORTED;
    *plan_out = convex_plan(T_, R);
    if (forced) plan_out->S = forced;
    if (forced_w) plan_out->W = forced_w;
    if (workspace_bytes < convex_workspace_bytes(M, R, T_, o.dtype, plan_out->S)) return ST_WORKSPACE;
    return ST_OK;
}

}  // namespace evc
