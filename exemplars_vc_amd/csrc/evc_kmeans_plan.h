// evc_kmeans_plan.h - what evc_kmeans decides on the host before its launches: the limits, the argument checks in the order
// of their statuses, kmeans_splits() (centre ranges of k_km_assign) and the workspace carving.  No device code:
// tests/kmeans_host_main.hip, a program of its own, includes it and runs it under the host sanitizers
// (tests/test_kmeans_host.py).
#pragma once
#include "evc_internal.h"

namespace evc {

constexpr int KM_MAX_M = 1056;           // LEARN_MAX_M: M is only a contraction length here
constexpr int KM_MAX_T = 1 << 20;
constexpr int KM_MAX_R = 4096;
constexpr int KM_MAX_SLOTS = MAX_SLOTS;  // error slots: the start and one per round
constexpr int KM_BT = 64;                // samples per workgroup of k_km_assign: four wavefronts of 16
constexpr int KM_CT = 32;                // centres per MFMA step of a wavefront: two tiles of 16
constexpr int KM_KC = 64;                // bins per chunk staged in LDS; M <= KM_KC: the X tile is staged once
constexpr int KM_MAX_S = 16;             // centre ranges (slabs of partial results in the workspace)
constexpr int KM_FILL_WGS = 256;         // one workgroup per compute unit of a 256-CU part

// Centre ranges of the assignment: where the sample tiles alone are fewer than KM_FILL_WGS workgroups the ceil(R / KM_CT)
// centre tiles are split into S contiguous ranges, at most KM_MAX_S and never more than there are centre tiles.  A function
// of (R, T) alone, never of the device; the labels do not depend on S (the merge is lexicographic on (score, index)).
inline int kmeans_splits(int R, int T_) {
    const long tiles = ((long)T_ + KM_BT - 1) / KM_BT, ctiles = ((long)R + KM_CT - 1) / KM_CT;
    long S = (KM_FILL_WGS + tiles - 1) / tiles;
    if (S > ctiles) S = ctiles;
    if (S > KM_MAX_S) S = KM_MAX_S;
    return S < 1 ? 1 : (int)S;
}

// (more centres than samples: only the assignment alone, EVC_KM_ASSIGN_ONLY, takes them - kmeans_args_check)
inline bool kmeans_sizes_ok(int M, int R, int T_) {
    return M >= 1 && M <= KM_MAX_M && T_ >= 1 && T_ <= KM_MAX_T && R >= 1 && R <= KM_MAX_R;
}

struct KmWs {
    char* xn;           // [T] elements: ||x_t||^2
    char* wn;           // [R] elements: ||w_r||^2
    char* s1;           // [T] elements: the best expanded score
    char* s2;           // [T] elements: the second-best
    char* ps1;          // [S][T] elements: the ranges' best scores (S > 1)
    char* ps2;          // [S][T] elements: their second-best
    int* pi1;           // [S][T]: the ranges' best indices (S > 1)
    int* flag;          // [T]: 1 = re-decided by the direct form
    int* lab;           // [T]: the labels
    int* prev;          // [T]: the labels of the assignment before
    int* chg;           // [T]: 1 = the label changed in this round
    int* cnt;           // [R]: members per centre
    double* err2;       // [T]: every sample's squared distance to its centre
    double* trace;      // [KM_MAX_SLOTS]
    double* eprev;      // [1]
    int* stop;          // [1]: 0 running, else the round the loop stopped at
    size_t bytes;
};

// [xn | wn | s1 | s2 | ps1 | ps2 | pi1 | flag | lab | prev | chg | cnt | err2 | trace | eprev | stop], each 256-byte aligned
// (ws == NULL: sizes only)
inline KmWs carve_kmeans(void* ws, int R, int T_, int S, int dtype) {
    KmWs w;
    Carver c = Carver::rounded(ws);
    const size_t es = dtype == EVC_F64 ? 8 : 4;
    const size_t t = (size_t)T_, st = S > 1 ? (size_t)S * t : 0;
    w.xn = c.take<char>(t * es);
    w.wn = c.take<char>((size_t)R * es);
    w.s1 = c.take<char>(t * es);
    w.s2 = c.take<char>(t * es);
    w.ps1 = c.take<char>(st * es);
    w.ps2 = c.take<char>(st * es);
    w.pi1 = c.take<int>(st);
    w.flag = c.take<int>(t);
    w.lab = c.take<int>(t);
    w.prev = c.take<int>(t);
    w.chg = c.take<int>(t);
    w.cnt = c.take<int>((size_t)R);
    w.err2 = c.take<double>(t);
    w.trace = c.take<double>((size_t)KM_MAX_SLOTS);
    w.eprev = c.take<double>(1);
    w.stop = c.take<int>(1);
    w.bytes = c.bytes();
    return w;
}

// with the plan's own S; a forced S beyond it needs (S - S_plan) T (2 elements + 1 int) more (S <= 0: the plan's)
inline size_t kmeans_workspace_bytes(int M, int R, int T_, int dtype, int S = 0) {
    if (!kmeans_sizes_ok(M, R, T_) || (dtype != EVC_F64 && dtype != EVC_F32)) return 0;
    return carve_kmeans(nullptr, R, T_, S > 0 ? S : kmeans_splits(R, T_), dtype).bytes + 256;
}

// evc_kmeans' argument checks, in the order of its statuses: ST_BADARG, ST_UNSUPPORTED, ST_WORKSPACE before any device
// work.  *S_out: the centre ranges the call runs with - kmeans_splits' choice, or what bits 8..15 of `reserved` force.
inline int kmeans_args_check(const void* X, int ldx, const void* W, int ldw, int M, int R, int T_, const evc_kmeans_opts* opts,
                             const void* workspace, size_t workspace_bytes, int* S_out) {
    if (!opts || opts->struct_bytes != (int)sizeof(evc_kmeans_opts)) return ST_BADARG;
    const evc_kmeans_opts& o = *opts;
    const int forced = (o.reserved >> 8) & 0xff;
    if (M < 1 || R < 1 || T_ < 1 || (o.dtype != EVC_F64 && o.dtype != EVC_F32)) return ST_BADARG;
    if (o.layout != EVC_FRAME_MAJOR && o.layout != EVC_BIN_MAJOR) return ST_BADARG;
    if ((o.reserved & ~0xff01) != 0 || forced > KM_MAX_S) return ST_BADARG;
    if (o.update != EVC_KM_BOTH && o.update != EVC_KM_ASSIGN_ONLY) return ST_BADARG;
    if (o.stop_rule != EVC_KM_STOP_NONE && o.stop_rule != EVC_KM_STOP_PYMF && o.stop_rule != EVC_KM_STOP_LABELS) return ST_BADARG;
    if (o.iters < 0 || o.iters > KM_MAX_SLOTS - 1) return ST_BADARG;
    if (!(o.tol >= 0.0)) return ST_BADARG;
    if (!X || !W || !workspace) return ST_BADARG;
    if (bad_ld(o.layout, ldx, T_, M) || bad_ld(o.layout, ldw, R, M)) return ST_BADARG;
    if (!kmeans_sizes_ok(M, R, T_) || (o.update == EVC_KM_BOTH && R > T_)) return ST_UNSUPPORTED;
    *S_out = forced ? forced : kmeans_splits(R, T_);
    if (workspace_bytes < kmeans_workspace_bytes(M, R, T_, o.dtype, *S_out)) return ST_WORKSPACE;
    return ST_OK;
}

}  // namespace evc
