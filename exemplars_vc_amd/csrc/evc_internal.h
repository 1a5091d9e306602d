// Internal declarations shared by the translation units of libevc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/evc.h"
#include "evc_gemm_plan.h"

namespace evc {

// ------------------------------------------------------------------------------------------
// MFMA 16x16x4 wrappers.  One operand element per lane for A and B:
//   A-operand lane l holds Aop[i = l & 15][k = l >> 4]
//   B-operand lane l holds Bop[k = l >> 4][j = l & 15]
// C/D (4 values per lane, register r):  column j = l & 15 and
//   f64: row i = (l >> 4) + 4 r          (v_mfma_f64_16x16x4_f64)
//   f32: row i = 4 (l >> 4) + r          (v_mfma_f32_16x16x4_f32)
// ------------------------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <typename T> struct Mma;
template <> struct Mma<double> {
    typedef f64x4 acc_t;
    static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};
template <> struct Mma<float> {
    typedef f32x4 acc_t;
    static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int row(int lane, int r) { return 4 * (lane >> 4) + r; }
};

// ------------------------------------------------------------------------------------------
// The element-wise multiplicative update, one statement per reference surface.
//   h: current activation, p: numerator (A^T X), d: denominator (A^T A H)
// ------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T mu_update(T h, T p, T d, int eps_mode, T eps, T l1) {
    d += l1;                                        // sklearn _nmf.py:615-617 (l1 == 0: identity)
    switch (eps_mode) {
        case EVC_EPS_ADD:                           // pymf nmf.py:68-70
            return (h * p) / (d + eps);
        case EVC_EPS_ZERO_REPLACE:                  // sklearn _nmf.py:620-629
            d = (d == T(0)) ? eps : d;
            return h * (p / d);
        case EVC_EPS_CLAMP:                         // deComP batch_mu.py
            return h * (p / (d > eps ? d : eps));
        default:                                    // EVC_EPS_NONE, nmf_tool nmf.py:39
            return (h * p) / d;
    }
}

// per-utterance bookkeeping that lives in the workspace
struct UttState {
    int* frame_utt;      // [Tp]  utterance index of each frame (padding frames: -1)
    int* offsets;        // [n_utt+1]
    int* active;         // [n_utt + 1]: per utterance; [n_utt]: how many are active (the gate of the generic path's kernels)
    int* n_iter;         // [n_utt]
    double* err_init;    // [n_utt]
    double* err_prev;    // [n_utt]
    double* h0;          // [n_utt]   initial activation value (INIT_SKLEARN / CONST)
    double* trace;       // [n_utt][n_slots]
    int n_slots;
};

template <typename T> struct MuEpilogue {
    const T* Hin;        // [Tp][ldh]
    const T* P;          // [Tp][ldh]
    const int* frame_utt;
    const int* active;
    int ldh;
    int N, T_;           // true (unpadded) sizes
    int eps_mode;
    T eps, l1;
    int kl;              // 1: Hout = Hin * acc (the KL numerator over a pre-scaled dictionary); P unused
    const int* gate;     // optional: the kernel returns at once when *gate == 0 (no utterance is active any more)
};

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// ------------------------------------------------------------------------------------------
// Host pieces every entry's translation unit shares: statuses, padded sizes, workspace carving.
// ------------------------------------------------------------------------------------------
enum { ST_OK = 0, ST_BADARG = -1, ST_WORKSPACE = -2, ST_UNSUPPORTED = -3, ST_COOP_TIMEOUT = -4 };

// (expr: a hipError_t or one of the statuses above - both are 0 on success)
#define HIP_TRY(expr)                              \
    do {                                           \
        int e__ = (int)(expr);                     \
        if (e__) return e__;                       \
    } while (0)

// FRAME_MAJOR: rows_fm x cols_fm with ld >= cols_fm; BIN_MAJOR: the transpose
inline bool bad_ld(int layout, int ld, int rows_fm, int cols_fm) {
    return layout == EVC_FRAME_MAJOR ? ld < cols_fm : ld < rows_fm;
}

// The worst-case slot count is bounded by iters+1; evc_workspace_bytes has no iters argument,
// so the trace region is sized for MAX_SLOTS checks and evc_nmf_solve rejects more.
constexpr int MAX_SLOTS = 4097;
inline int n_slots_for(int iters, int check_every) { return 1 + (check_every > 0 ? iters / check_every : 0); }

// frames are padded to the contraction kernels' frame tile: 64 where k_gemm2 is in charge (float32) and for short
// float64 batches (<= 2048 frames: k_gemm_nt then runs 64-row blocks anyway, and one 688-frame utterance is 704
// rows instead of 768), 128 otherwise (diagnostic builds: see use_gemm2 in evc_gemm.hip)
inline int frame_pad(int esize, int T_) {
#if defined(EVC_DIAG_GEMM_V1)
    return round_up(T_, 128);
#elif defined(EVC_DIAG_GEMM2_F64)
    return round_up(T_, 64);
#else
    return round_up(T_, (esize == 4 || T_ <= 2048) ? 64 : 128);
#endif
}

// the padded sizes of the frames-as-rows arrays gemm_nt and dict_grad work on
struct Dims {
    int M, N, T_, n_utt, Mb;
    int Mk, Mj, Np, Tp;
};
inline Dims make_dims(int esize, int M, int N, int T_, int n_utt, int Mb = 0) {
    Dims d;
    d.M = M; d.N = N; d.T_ = T_; d.n_utt = n_utt; d.Mb = Mb;
    d.Mk = round_up(M, 16);
    d.Mj = round_up(M, 64);
    d.Np = round_up(N, 128);
    d.Tp = frame_pad(esize, T_);
    return d;
}

// Workspace carving.  take() first rounds `off` up to 256 bytes, so every array starts at a multiple of 256 bytes from
// `base`, `off` is the end of the last array, and bytes() is what the carving needs of the caller's pointer.  The base is
// one of two:
//   Carver{ws, skip}       the caller's pointer as given: the caller aligns it (evc_workspace_bytes, evc_dict_bytes and the
//                          entries built on them: the solves, the prepared images, evc_nmf_learn)
//   Carver::rounded(ws)    the caller's pointer rounded up to 256 bytes; bytes() counts the shift, and the size query -
//                          which carves from NULL, where there is none - adds 256 for it (evc_cd_solve, evc_beta_solve,
//                          evc_cd_learn, evc_beta_learn)
// base == NULL: sizes only, every take() gives NULL.
struct Carver {
    char* base;
    size_t off;
    size_t shift = 0;
    static Carver rounded(void* ws) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(ws), up = (p + 255) & ~uintptr_t(255);
        return Carver{reinterpret_cast<char*>(up), 0, (size_t)(up - p)};
    }
    template <typename U> U* take(size_t count) {
        off = (off + 255) & ~size_t(255);
        U* p = base ? reinterpret_cast<U*>(base + off) : nullptr;
        off += count * sizeof(U);
        return p;
    }
    size_t bytes() const { return shift + ((off + 255) & ~size_t(255)); }
};

// utterance u is frames [utt_offsets[u], utt_offsets[u + 1]) of the call's T_; NULL: the call is one utterance
// (evc_nmf_solve / evc_nmf_convert, evc_cd_solve, evc_beta_solve)
inline bool utt_offsets_ok(const int* utt_offsets, int n_utt, int T_) {
    if (!utt_offsets) return n_utt == 1;
    if (utt_offsets[0] != 0 || utt_offsets[n_utt] != T_) return false;
    for (int i = 0; i < n_utt; ++i)
        if (utt_offsets[i + 1] < utt_offsets[i]) return false;
    return true;
}

// The frame-tile table of k_cd_sweep and the beta kernels: every utterance starts a tile of its own, a tile is up to F of
// its frames, {x: utterance, y: first frame, z: frames, w: first tile of the utterance}.  k_cd_sweep reads .w; the beta
// kernels ignore it.  utt_tile0[u] is utterance u's first tile ([n_utt]: the tile count), utt_frames[u] its frames.
// The count is at most frame_tile_cap whatever the split into utterances.
inline int frame_tile_cap(int T_, int F, int n_utt) { return (T_ + F - 1) / F + n_utt; }

// The table on the host: no HIP call, no global state.  Returns the tile count; tiles == NULL only counts, and either of
// the other two arrays may be NULL.
inline int frame_tiles(int F, const int* utt_offsets, int n_utt, int T_, int4* tiles, int* utt_tile0, int* utt_frames) {
    int t = 0;
    for (int u = 0; u < n_utt; ++u) {
        const int f0 = utt_offsets ? utt_offsets[u] : 0;
        const int tu = utt_offsets ? utt_offsets[u + 1] - f0 : T_;
        const int t0 = t;
        if (utt_tile0) utt_tile0[u] = t0;
        if (utt_frames) utt_frames[u] = tu;
        for (int i = 0; i < tu; i += F, ++t)
            if (tiles) tiles[t] = make_int4(u, f0 + i, tu - i < F ? tu - i : F, t0);
    }
    if (utt_tile0) utt_tile0[n_utt] = t;
    return t;
}

// ... and staged to the device arrays (d_utt_frames may be NULL) on `s`, from pageable memory: HIP has copied the bytes by
// the time hipMemcpyAsync returns, so the host table is freed here.  ST_OK, ST_BADARG (more tiles than the workspace was
// carved for) or a hipError_t.
inline int frame_tiles_stage(int F, const int* utt_offsets, int n_utt, int T_, int4* d_tiles, int* d_utt_tile0,
                             int* d_utt_frames, hipStream_t s, int* n_tiles_out) {
    const int n_tiles = frame_tiles(F, utt_offsets, n_utt, T_, nullptr, nullptr, nullptr);
    if (n_tiles > frame_tile_cap(T_, F, n_utt)) return ST_BADARG;
    int4* h_tiles = static_cast<int4*>(malloc(sizeof(int4) * (n_tiles > 0 ? n_tiles : 1) + sizeof(int) * (2 * n_utt + 1)));
    if (!h_tiles) return (int)hipErrorOutOfMemory;
    int* h_t0 = reinterpret_cast<int*>(h_tiles + (n_tiles > 0 ? n_tiles : 1));
    int* h_fr = h_t0 + n_utt + 1;
    frame_tiles(F, utt_offsets, n_utt, T_, h_tiles, h_t0, h_fr);
    hipError_t e = hipSuccess;
    if (n_tiles > 0) e = hipMemcpyAsync(d_tiles, h_tiles, sizeof(int4) * n_tiles, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_utt_tile0, h_t0, sizeof(int) * (n_utt + 1), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && d_utt_frames)
        e = hipMemcpyAsync(d_utt_frames, h_fr, sizeof(int) * n_utt, hipMemcpyHostToDevice, s);
    free(h_tiles);
    *n_tiles_out = n_tiles;
    return (int)e;
}

// ----- evc_gemm.hip -----
// C[I x J] = L[I x Kd] * R[J x Kd]^T, all row-major, I % 128 == 0, J % 64 == 0, Kd % 16 == 0.
// scratch (optional, scratch_elems elements): lets a small-grid, long-K product be split over K.
template <typename T>
hipError_t gemm_nt(const T* L, int ldl, const T* R, int ldr, T* C, int ldc, int I, int J, int Kd,
                   hipStream_t s, T* scratch = nullptr, size_t scratch_elems = 0, int* splits_out = nullptr,
                   int j_valid = 0, const int* gate = nullptr, GemmPlan* plan_out = nullptr);
// plan_out: optional; what was launched (evc_gemm_plan.h; kernel 0 when nothing was)
// gate: optional device word; the launched kernels return at once when it is 0 (the stop rules have stopped every
// utterance: the launches the host has still queued cost a few microseconds each instead of a contraction)
// j_valid: rows of R from j_valid on are known to be zero (padding up to the block width); their products are skipped
// splits_out: when the contraction was split over k into slabs in `scratch` (slab z at scratch + z * I * ldc),
// *splits_out = their number and C is NOT written - the caller's next kernel sums them in order; else 0.
// Same contraction with the multiplicative update as epilogue: C = mu(Hin, P, L R^T).
template <typename T>
hipError_t gemm_nt_mu(const T* L, int ldl, const T* R, int ldr, T* Hout, int I, int J, int Kd,
                      const MuEpilogue<T>& ep, hipStream_t s, GemmPlan* plan_out = nullptr);
// ----- evc_gemm2.hip: second-generation contraction kernel (swizzled row-major LDS, 16-byte fragment reads,
// vector epilogue); gemm_nt / gemm_nt_mu route to it whenever shapes and alignment allow -----
template <typename T>
bool gemm2_ok(const T* L, int ldl, const T* R, int ldr, const T* C, int ldc, int I, int J, int Kd);
template <typename T>
hipError_t gemm2(const T* L, int ldl, const T* R, int ldr, T* C, int ldc, int I, int J, int Kd, hipStream_t s,
                 T* scratch, size_t scratch_elems, int* splits_out, int n_cus, int j_valid, const int* gate = nullptr,
                 GemmPlan* plan_out = nullptr);
template <typename T>
hipError_t gemm2_mu(const T* L, int ldl, const T* R, int ldr, T* Hout, int I, int J, int Kd,
                    const MuEpilogue<T>& ep, hipStream_t s, GemmPlan* plan_out = nullptr);
// C = sum_z part[z * slab + .]  (fixed order)
template <typename T>
hipError_t sum_slabs(const T* part, long slab, int splits, T* C, hipStream_t s, const int* gate = nullptr);
// Bounds-checked general-stride contraction on caller memory (used by evc_synthesize):
// C[i*csi + j*csj] = sum_k L[i*lsi + k*lsk] * R[j*rsj + k*rsk]
template <typename T>
hipError_t gemm_strided(const T* L, long lsi, long lsk, const T* R, long rsj, long rsk, T* C,
                        long csi, long csj, int I, int J, int Kd, hipStream_t s);
// Y = B H for Mb <= 64 bins (evc_synthesize): H(t,n) = H[t hst + n hsn], B(n,mb) = B[n bsn + mb bsm], Y(t,mb) = Y[t yst + mb ysm]
template <typename T>
hipError_t synth_skinny(const T* H, long hst, long hsn, const T* B, long bsn, long bsm, T* Y, long yst,
                        long ysm, int T_, int Mb, int N, hipStream_t s);

// ----- evc_aux.hip -----
// dst (dst_rows x dst_cols, row stride dst_ld) = src (src_rows x src_cols), zero outside src.
// src_trans: element (r,c) of the logical matrix is src[c*src_ld + r] instead of src[r*src_ld + c];
// dst_trans likewise for the destination.
// element-type conversion of a row-major matrix (the float32 surfaces ride the float64 fused path)
template <typename S, typename D>
hipError_t cvt2d(const S* src, long lds_, long rows, long cols, D* dst, long ldd, hipStream_t s);
template <typename T>
hipError_t copy2d(const T* src, long src_ld, int src_rows, int src_cols, int src_trans, T* dst,
                  long dst_ld, int dst_rows, int dst_cols, int dst_trans, hipStream_t s);
hipError_t utt_single(const UttState& u, int T_, hipStream_t s);
hipError_t utt_setup(const UttState& u, int n_utt, int T_, int Tp, int iters, hipStream_t s);
template <typename T>
hipError_t utt_sklearn_h0(const T* Xt, int ldx, int M, int N, const UttState& u, int n_utt,
                          hipStream_t s);
hipError_t utt_const_h0(const UttState& u, int n_utt, double v, hipStream_t s);
template <typename T>
hipError_t fill_h0(T* Ht, int ldh, int Tp, int N, int T_, const UttState& u, hipStream_t s);
template <typename T>
hipError_t frame_err2(const T* Xt, int ldx, const T* Vt, int ldv, int M, int T_, double* err2,
                      hipStream_t s);
// generalised KL variant: dictionary scaled by 1/colsum, ratio X / max(V, eps), per-frame 2*KL
template <typename T>
hipError_t kl_scale_dict(const T* At, int ld, int M, int rows, double eps, T* Akl, hipStream_t s);
template <typename T>
hipError_t kl_ratio(const T* Xt, int ldx, const T* Vt, int ldv, int M, long Tp, double eps, T* Rt, int ldr,
                    hipStream_t s);
template <typename T>
hipError_t frame_err_kl(const T* Xt, int ldx, const T* Vt, int ldv, int M, int T_, double eps, double* err2,
                        hipStream_t s);
// evaluate the stopping rule after check number `c` (c == 0: error at init)
hipError_t utt_check(const double* err2, const UttState& u, int n_utt, int c, int check_every,
                     int stop_rule, double tol, hipStream_t s);

// ----- evc_fused.hip -----
// Persistent fused FACTORED kernel for small dictionaries heights (M <= 32), float64.
struct FusedLayout {
    int NT;              // exemplar tiles of 16
    int TT, TTp;         // frame tiles of 16 (TTp: padded to a multiple of 4)
    int msteps;          // k-steps of 4 bins actually issued
    int mtiles;          // 1 (M <= 16) or 2
    int M;               // bins
    size_t a1, a2, xp, hp, vp;   // element counts of the packed arrays
};
constexpr int COOP_MAX_TILES = 256;       // frame tiles x cooperating workgroups never exceeds this (one per CU)
constexpr int ALL_MAX_WGS = 1024;         // resident workgroups of k_fused_all the exchange buffers are sized for
// k_fused_all with more than 8 members per group: the summed slices live behind the partials in coop_buf
constexpr int ALL_MAX_MEMBERS = 128;      // members per frame tile (N <= 65536)
constexpr int ALL_RS_STRIDE = 640;        // words per member in a group's partials: C slices x ceil(NE / C) <= NE + C - 1
constexpr long ALL_SLICE_OFFSET = 2L * ALL_MAX_WGS * ALL_RS_STRIDE;
constexpr long ALL_SLICE_ELEMS = 2L * (ALL_MAX_WGS / 2) * 512;    // [2][groups <= ALL_MAX_WGS / 2][512]
int fused_res_coop_factor(int NT, int TT, int n_cus);
// workgroups per frame tile the all-resident kernel (k_fused_all) uses for this problem; 0: it does not apply
int fused_all_members(int NT, int N, int eps_mode, int exact_div, int loss);
// workgroups per PAIR of frame tiles k_fused_xy (evc_fused_xy.hip) uses for this problem; 0: it does not apply
int fused_xy_members(int NT, int N, int eps_mode, int exact_div, int loss);
bool fused_res_supported(int N, int eps_mode, int exact_div);
// The M <= 32 part of a solve's route: decided once per attempt (plan_route, evc_solve_plan.h); fused_iterate launches what it
// says and evc_solve_info reports the same fields
struct FusedRoute {
    int kernel;            // EVC_KERNEL_FUSED_MU | FUSED_RES | FUSED_ALL | FUSED_XY
    int members;           // workgroups per frame tile (k_fused_xy: per pair of frame tiles); > 1: they exchange partial sums
    int c_req;             // k_fused_mu's frame tiles per workgroup: 0 = automatic, 1 / 2 (tests, A/B timing)
    int exact_div;         // correctly rounded quotients (general kernel only; see exact_div() in evc_fused_common.h)
    int init_const;        // 1: the first launch forms H = h0 and V = h0 rowsum(A) itself (no fill, no pre-pass)
    int direct_export;     // 1: nothing can stop, so the last launch may write the caller's H itself (k_fused_all)
    int n_cus;             // compute units of the device (sizes k_fused_all's persistent grid)
};
struct FusedBuffers {
    double *A1p, *A2p, *Xp, *Hp, *Vp;
    double* coop_buf;      // exchange buffers of the cooperative launch (see k_fused_res)
    int* coop_cnt;         // [COOP_MAX_TILES] arrival counters, then one abort flag
    double* rsum;          // [32] row sums of the dictionary (k_fused_all's in-kernel start)
};
// What the last launch of a solve in which nothing can stop does beyond the updates (plan_fused_tail, evc_solve_plan.h,
// decides; every other launch passes none); see FusedArgs
struct FusedLaunchTail {
    double* Hx;            // the launch also writes the caller's H (NULL: off); ldhx, hx_frame_major
    long ldhx;
    int hx_frame_major;
    // k_fused_all only: the launch also forms the members' shares of Y = B H (Yslab NULL: off)
    const double* Yb2p;
    double* Yslab;
    long y_stride;
    int y_mt;
    int skip_hp;           // 1: that launch does not store the packed activations (nothing reads them after it)
};
bool fused_supported(int M, int N, int T_, int dtype);
FusedLayout fused_layout(int M, int N, int T_);
// At[n][m] / Xt[t][m]: the zero-padded frames-as-rows workspace arrays
// (either destination may be NULL: only the other fragment order is written); At has n_rows rows: the exemplar
// slots of the (possibly further padded) tile grid beyond them are written as zeros
// ones_bin >= 0: that (padding) bin of the D-operand image holds 1.0 in every exemplar slot, so that a constant placed in
// the same bin of V's image is added to every denominator by the D product itself (k_fused_xy; the images of X and V
// hold zeros there otherwise, so every other kernel is unaffected)
hipError_t fused_pack_dict(const FusedLayout& f, double* A1p, double* A2p, const double* At, int ldA, int n_rows,
                           hipStream_t s, int ones_bin = -1);
hipError_t fused_pack_frames(const FusedLayout& f, double* Xp, const double* Xt, int ldx, hipStream_t s);
// rsum[m] = sum_n At[n][m] for m < M (fixed order), 0 for M <= m < 32
hipError_t fused_rowsum(const double* At, int ldA, int M, int N, double* rsum, hipStream_t s);
// packed activations <-> the caller's H (frame_major: H[t*ldh+n], else H[n*ldh+t]); per-utterance constant fill
hipError_t fused_import_h(const FusedLayout& f, double* Hp, const double* H, long ldh, int frame_major, int T_,
                          int N, hipStream_t s);
hipError_t fused_export_h(const FusedLayout& f, const double* Hp, double* H, long ldh, int frame_major, int T_,
                          int N, hipStream_t s);
hipError_t fused_fill_h(const FusedLayout& f, double* Hp, int N, int T_, const UttState& u, hipStream_t s);
// Y = B H from the packed activations (fB: layout for (Mb, N, T); B2p: B's V'-operand fragments)
hipError_t fused_synthesize(const FusedLayout& fB, const double* B2p, const double* Hp, double* Yp,
                            const UttState& u, int N, int T_, int Mb, double* Y, long ldy, int frame_major,
                            hipStream_t s);
// Y (caller layout) from `members` images of B H in the Yp format, `stride` doubles apart, added in member order
hipError_t fused_unpack_y(const FusedLayout& fB, const double* Yp, int members, long stride, int T_, int Mb, double* Y,
                          long ldy, int frame_major, hipStream_t s);
// `iters` updates in one launch.  first: V is built from H by a pre-pass (else carried over in
// Vp from the previous launch); write_err: per-frame squared residuals of the final H -> err2.
// lone_bin: k_fused_all at M = 25 runs as k_fused_lone where fused_all_launch has an instance (false: EVC_FLAG_NO_LONE_BIN).
// quad_rows: k_fused_lone's shapes run as k_fused_quad (false: EVC_FLAG_NO_QUAD_ROWS).
// range_hoist: k_fused_all / k_fused_lone decide the update's range test once per sweep (false: EVC_FLAG_NO_RANGE_HOIST).
hipError_t fused_iterate(const FusedLayout& f, const FusedBuffers& b, const FusedRoute& r, const UttState& u, int N,
                         int T_, int iters, int first, int write_err, double* err2, int eps_mode, double eps, double l1,
                         int all_live_known, int loss, hipStream_t s, const FusedLaunchTail* tail, bool lone_bin = true,
                         bool range_hoist = true, bool quad_rows = true);

// ----- evc_wide.hip -----
// Fused FACTORED kernel for wide spectra (32 < M <= 208 bins, float32): k_fused_wide, a task queue over
// (iteration, frame group, exemplar range).
struct WideLayout {
    int MT;              // bin tiles of 16 (template instance: >= ceil(M / 16))
    int W;               // wavefronts (= frame tiles of 16) per workgroup: 4 or 8
    int NB;              // exemplar blocks of 16
    int TT, G;           // frame tiles, frame groups of W tiles
    int c, rmode;        // exemplar ranges per group; 1: a reduce task sums the partial V' (c > 4)
    int tagged;          // 1: static schedule with reduce slices - the hand-offs carry their arrival flag in the data (evc_wide.hip)
    size_t aw, xw, hw, vpart, vsum;      // element counts (Pw has hw elements)
};
struct WideBuffers {
    float *Aw, *Xw, *Hw, *Pw, *Vpart, *Vsum;
    unsigned* ctl;       // [4 + 2 G]: ticket, abort flag, -, -, done[G], done_r[G]
    // several stop checks per launch (round 4): snapshots of the activations at the checks inside a launch and the
    // residuals the following iteration's tasks leave (NULL / 0: one check per launch)
    float* Hs;           // [snap_slots][hs_stride]
    size_t hs_stride;
    double* err2s;       // [snap_slots][err_stride]
    long err_stride;
    int snap_slots;
};
bool wide_supported(int M, int N, int T_, int dtype, int algo);
// c_req / w_req: 0 = automatic (tuning and tests: ranges per group, wavefronts per workgroup)
WideLayout wide_layout(int M, int N, int T_, int n_cus, int c_req, int w_req);
size_t wide_ctl_words(const WideLayout& f);
struct WideCaps { size_t aw, xw, hw, vpart, vsum, ctl; int c_cap; };
WideCaps wide_caps(int M, int N, int T_, int n_cus);
bool wide_fits(const WideLayout& f, const WideCaps& k);
// evc_solve_info.variant of a solve on this layout: bit 0 static schedule, bit 1 reduce slices, bit 2 tagged hand-offs,
// bits 8..15 wavefronts per workgroup, bits 16..23 MT (include/evc.h).  wide_iterate schedules by the same bits.
int wide_variant(const WideLayout& f, int n_cus);
// At1: the dictionary the numerator / denominator contraction uses (A, or A / colsum for KL), At2: A; exemplars as rows
hipError_t wide_pack_dict(const WideLayout& f, const float* At1, const float* At2, int ld, int n_rows, float* Aw,
                          hipStream_t s);
hipError_t wide_pack_x(const WideLayout& f, const float* Xt, int ld, int rows, float* Xw, hipStream_t s);
hipError_t wide_import_h(const WideLayout& f, float* Hw, const float* H, long ldh, int frame_major, int T_, int N,
                         hipStream_t s);
hipError_t wide_export_h(const WideLayout& f, const float* Hw, float* H, long ldh, int frame_major, int T_, int N,
                         const int* abort, hipStream_t s);
hipError_t wide_begin(const WideLayout& f, const WideBuffers& b, hipStream_t s);
// snap_every > 0: the iterations snap_first, snap_first + snap_every, ... < it_end - 1 are stop checks inside the launch
// (b.Hs / b.err2s receive the activations and the residuals of check k in slot k; wide_restore puts a slot back)
hipError_t wide_iterate(const WideLayout& f, const WideBuffers& b, const UttState& u, int N, int T_, int it_begin,
                        int it_end, int mode, double eps, double l1, int init_const, int n_cus, hipStream_t s,
                        int snap_every = 0, int snap_first = 0);
hipError_t wide_restore(const WideLayout& f, const WideBuffers& b, const UttState& u, int slot, int target_iter, int T_,
                        hipStream_t s);
hipError_t wide_err2(const WideLayout& f, const WideBuffers& b, const UttState& u, int N, int T_, int it, int kl,
                     double eps, double* err2, hipStream_t s);

// ----- evc_wide64.hip -----
// The same task queue for wide float64 spectra (144 < M <= 528, Frobenius): k_fused_wide64; a workgroup of four
// wavefronts owns 32 frames, the bins are split over its wavefronts.
struct Wide64Layout {
    int TPW;             // whole bin tiles of 16 per wavefront (template instance: 64 TPW + 16 >= M; the last tile is split)
    int NB;              // exemplar blocks of 16
    int TT, G;           // frame tiles, frame groups of 2 tiles
    int c, rmode;        // exemplar ranges per group; 1: a reduce task sums the partial V' (c > 4)
    size_t aw, xw, hw, vpart, vsum;      // element counts (Pw has hw elements)
};
struct Wide64Buffers {
    double *Aw, *Xw, *Hw, *Pw, *Vpart, *Vsum;
    unsigned* ctl;       // [4 + 2 G]: ticket, abort flag, -, -, done[G], done_r[G]
};
struct Wide64Caps { size_t aw, xw, hw, vpart, vsum, ctl; int c_cap; };
bool wide64_supported(int M, int N, int T_, int dtype, int algo, int loss);
// c_req: 0 = automatic; tpw_req: 0 = the narrowest instance that holds M bins (tests: a wider one)
Wide64Layout wide64_layout(int M, int N, int T_, int n_cus, int c_req, int tpw_req);
size_t wide_ctl_words(const Wide64Layout& f);
Wide64Caps wide64_caps(int M, int N, int T_, int n_cus);
bool wide_fits(const Wide64Layout& f, const Wide64Caps& k);
// evc_solve_info.variant: bit 0 static schedule, bit 1 reduce slices, bits 8..15 TPW, bits 16..23 4 TPW + 1 bin tiles
int wide_variant(const Wide64Layout& f, int n_cus);
// (the second dictionary pointer, the KL-scaled rows of the float32 kernel, is unused: Frobenius only)
hipError_t wide_pack_dict(const Wide64Layout& f, const double* At, const double* unused, int ld, int n_rows, double* Aw,
                          hipStream_t s);
hipError_t wide_pack_x(const Wide64Layout& f, const double* Xt, int ld, int rows, double* Xw, hipStream_t s);
hipError_t wide_import_h(const Wide64Layout& f, double* Hw, const double* H, long ldh, int frame_major, int T_, int N,
                           hipStream_t s);
hipError_t wide_export_h(const Wide64Layout& f, const double* Hw, double* H, long ldh, int frame_major, int T_, int N,
                           const int* abort, hipStream_t s);
hipError_t wide_begin(const Wide64Layout& f, const Wide64Buffers& b, hipStream_t s);
hipError_t wide_iterate(const Wide64Layout& f, const Wide64Buffers& b, const UttState& u, int N, int T_, int it_begin,
                          int it_end, int mode, double eps, double l1, int init_const, int n_cus, hipStream_t s);
hipError_t wide_err2(const Wide64Layout& f, const Wide64Buffers& b, const UttState& u, int N, int T_, int it, int kl,
                     double eps, double* err2, hipStream_t s);

// ----- evc_gl.hip (Griffin-Lim, STFT), evc_mfcc.hip, evc_dtw.hip: entries and drivers sit with their kernels -----
// W_f with the periodic window alone: the table of evc_mfcc.hip's contraction
hipError_t stft_forward_table(int F, int hop, double* Wf, hipStream_t s);

// ----- evc_cd.hip: coordinate-descent activation solve (evc_cd_solve) -----
constexpr int CD_MAX_M = 1024;        // 64 lanes x 16 bins per lane
constexpr int CD_TRACE_CAP = 256;     // device ring of per-iteration violations (copied out in chunks)
struct CdGeometry {
    int L;      // lanes per frame (0: M unsupported)
    int mpl;    // bins per lane, ceil(M / L)
    int Mr;     // L * mpl: row stride of the packed dictionary and of the residual
    int F;      // frames per tile (one wavefront): 64 / L
};
CdGeometry cd_geometry(int M);
size_t cd_workspace_bytes(int M, int N, int T_, int n_utt, int esize);

// evc_cd_learn (entry and driver in evc_cd.hip): the alternating form
constexpr int CD_LEARN_MAX_R = 1024;  // 64 lanes x 16 components per lane; keeps learn_bin_tiles(R) within evc_nmf_learn's

// ----- evc_learn.hip: the dictionary update of evc_nmf_learn -----
constexpr int LEARN_MAX_M = 1056;     // 66 bin tiles of 16
constexpr int LEARN_MAX_R = 4096;
constexpr int LEARN_MAX_SPLITS = 64;  // frame ranges (slabs of partial sums) per launch
constexpr int DG_MB = 4;              // bin tiles of 16 per workgroup of k_dict_grad
constexpr int DG_RB = 2;              // component tiles of 16 per wavefront
constexpr int DG_WAVES = 4;           // wavefronts per workgroup: DG_WAVES * DG_RB * 16 = 128 components
// bin tiles per operand, padded to whole workgroups
inline int learn_bin_tiles(int M) { return round_up(round_up(M, 16) / 16, DG_MB); }
// frame ranges of the split-T contraction: a function of the sizes only (never of the device)
int learn_splits(int M, int R, int T_);
// part[s][which][m][r] = sum over the s-th frame range of L[t][m] Ht[t][r], L = Xt (which 0) | Vt (which 1); frames as
// rows, Ht padded to ldh = round_up(R, 128) columns; a slab (one `which` of one s) is learn_bin_tiles(M) * 16 * ldh elements
template <typename T>
hipError_t dict_grad(const T* Xt, int ldx, const T* Vt, int ldv, const T* Ht, int ldh, int M, int T_, int S, T* part,
                     hipStream_t s);
// Kullback-Leibler: Vt[t][m] <- Xt[t][m] / max(Vt[t][m], eps) in place for t < T_ (m < M; zero up to ldx columns)
template <typename T>
hipError_t dict_quot(const T* Xt, int ldx, T* Vt, int ldv, int M, int T_, double eps, hipStream_t s);
// ... and the one-operand contraction of that quotient: part[s][0][m][r] = sum over the s-th frame range of
// Qt[t][m] Ht[t][r], part[s][1][0][r] = sum over the range of Ht[t][r] (the rest of the second slab is not written);
// half the workgroups of dict_grad at the same S
template <typename T>
hipError_t dict_grad_kl(const T* Qt, int ldq, const T* Ht, int ldh, int M, int T_, int S, T* part, hipStream_t s);
// W <- update(W, sum_s part[s][0], sum_s part[s][1]) in the surface's literal operation order (EVC_LEARN_*), on the
// caller's W (bin_major: W[m ldw + r], else W[r ldw + m]); pymf: then every column divided by its Euclidean norm.
// loss EVC_LOSS_KL (sklearn surface): W[m][r] <- W[m][r] * (sum_s part[s][0][m][r] / s_r), s_r = sum_s part[s][1][0][r],
// s_r == 0 -> 1
template <typename T>
hipError_t dict_apply(const T* part, int S, int ldp, T* W, long ldw, int bin_major, int M, int R, int surface, int loss,
                      hipStream_t s);
// *out = sqrt(max(sum_t err2[t], 0)), summed in a fixed order
hipError_t err_total(const double* err2, int T_, double* out, hipStream_t s);

// ----- the host skeleton of the entries that learn both factors (evc_nmf_learn in evc_learn.hip, evc_cd_learn in
// evc_cd.hip, evc_beta_learn in evc_beta_learn.hip) -----
// What the three entries check alike, after their own look at `opts`: ST_OK or ST_BADARG.  reserved: bits 8..15 force the
// frame ranges (*forced; 0: learn_splits decides), no bit outside `allowed` may be set.
inline int learn_args_ok(int M, int R, int T_, int dtype, int layout, const void* X, const void* W, const void* H,
                         const void* ws, int ldx, int ldw, int ldh, int reserved, int allowed, int* forced) {
    *forced = (reserved >> 8) & 0xff;
    if (M < 1 || R < 1 || T_ < 1 || (dtype != EVC_F64 && dtype != EVC_F32)) return ST_BADARG;
    if (layout != EVC_FRAME_MAJOR && layout != EVC_BIN_MAJOR) return ST_BADARG;
    if ((reserved & ~allowed) != 0 || *forced > LEARN_MAX_SPLITS) return ST_BADARG;
    if (!X || !W || !H || !ws) return ST_BADARG;
    if (bad_ld(layout, ldx, T_, M) || bad_ld(layout, ldw, R, M) || bad_ld(layout, ldh, T_, R)) return ST_BADARG;
    return ST_OK;
}

// ... and what evc_cd_solve and evc_beta_solve check alike.  The struct_bytes test, the option ranges, the NULL rule of X
// and H (evc_cd_solve refuses NULL even without frames, evc_beta_solve does not) and the limits stay with each entry.
inline int solve_args_ok(int M, int N, int T_, int n_utt, int dtype, int layout, const void* A, const void* ws, int lda,
                         int ldx, int ldh, const int* utt_offsets) {
    if (M < 1 || N < 1 || T_ < 0 || n_utt < 1 || (dtype != EVC_F64 && dtype != EVC_F32)) return ST_BADARG;
    if (layout != EVC_FRAME_MAJOR && layout != EVC_BIN_MAJOR) return ST_BADARG;
    if (!A || !ws) return ST_BADARG;
    if (bad_ld(layout, lda, N, M) || bad_ld(layout, ldx, T_, M) || bad_ld(layout, ldh, T_, N)) return ST_BADARG;
    return utt_offsets_ok(utt_offsets, n_utt, T_) ? ST_OK : ST_BADARG;
}

// The check-and-stop loop of the two multiplicative-update drivers.  step() runs one iteration; error_now(slot, &err)
// evaluates the error of the current factors and waits for it (slot 0: the start, before ev_start; slot c: after
// iteration c * check_every); stop(c, err, err_prev, err_init) is the surface's rule, asked only when tol > 0 (tol = 0
// never stops, as in scikit-learn; a NaN error compares false in both rules and never stops, as in both references).
// The errors are evaluated at all only when somebody reads them: err_out (NaN where not evaluated) or the rule.
template <typename Step, typename ErrorNow, typename Stop>
int learn_loop(int iters, int check_every, double tol, double* err_out, int* n_iter_out, void* ev_start, void* ev_stop,
               hipStream_t s, Step step, ErrorNow error_now, Stop stop) {
    const bool want_err = check_every > 0 && (err_out || tol > 0.0);
    if (err_out) for (int i = 0; i < n_slots_for(iters, check_every); ++i) err_out[i] = __builtin_nan("");
    double err_init = 0.0, err_prev = 0.0, err = 0.0;
    if (want_err) {
        HIP_TRY(error_now(0, &err_init));
        err_prev = err_init;
        if (err_out) err_out[0] = err_init;
    }
    if (ev_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(ev_start), s));
    int n_iter = 0;
    for (int it = 1; it <= iters; ++it) {
        HIP_TRY(step());
        n_iter = it;
        if (!want_err || it % check_every != 0) continue;
        const int c = it / check_every;
        HIP_TRY(error_now(c, &err));
        if (err_out) err_out[c] = err;
        if (tol > 0.0 && stop(c, err, err_prev, err_init)) break;
        err_prev = err;
    }
    if (ev_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(ev_stop), s));
    if (n_iter_out) *n_iter_out = n_iter;
    return ST_OK;
}

}  // namespace evc
