// evc_deconv_learn.hip - evc_deconv_learn: convolutive NMF, the multi-frame model of evc_deconv_solve learnt in both factors.
// DESIGN.md §5.15; the statement is in include/evc.h.
//
// Per iteration the activation half is evc_deconv_solve's own (evc_deconv_kernels.h: k_deconv_pack_dict on the current W,
// k_deconv_v, k_deconv_update), then k_deconv_v once more leaves, for the new H, the tile images [tile][MP][16] the
// dictionary half contracts: Qn = X and Qd = V under Frobenius, Qn = X / max(V, EPS) under Kullback-Leibler, exact zeros in the
// padding bins and frame slots.  Every tap uses these images, so V is formed once.
//   k_deconv_dict_grad<T, ONE>  C_tau[m][r] = sum_t L[t][m] H[t - tau][r] on the 16x16x4 MFMA, k_dict_grad's shape
//                       (evc_learn.hip): a workgroup owns DG_MB bin tiles of one operand x 128 components x one contiguous
//                       range of frame tiles x one tap (the taps are a grid dimension: measured, §5.15), keeps its
//                       accumulators in registers for the whole range and leaves them as one slab per range and tap by
//                       plain stores.  The left operand comes straight from the tile
//                       images - a lane reads the four consecutive frame slots 4 g .. 4 g + 3 of its bin in one 16- or
//                       32-byte load, and the four MFMAs of a tile take one slot each - so X, V and Q are never transposed.
//                       The right operand is the caller's H at the row shifted back by the tap: a clamped address, then a
//                       select that zeroes the frames whose position in their utterance is below the tap (and the padding
//                       slots), as deconv_form_v does.  ONE (Kullback-Leibler): Qn alone, and the workgroups of the first
//                       bin block also sum the masked right operand's registers over the range, s_tau[r]; the mask is what
//                       truncates that sum at each utterance's end.
//   k_deconv_dict_apply adds the S slabs of every element in the order s = 0 .. S-1 and updates the caller's W_tau in place.
//   k_deconv_learn_v    EVC_DCL_DICT_ONLY: V, the images and the error shares a group of BT_GT bin tiles at a time, straight
//                       from the caller's W (deconv_form_v<T, false>, as k_deconv_synth): 16 KB of LDS whatever M is.
//   k_dcl_pack_x, k_dcl_tile_pos, k_dcl_err_total  the packed X, the per-tile {first frame, frames, frames before} table and
//                       the fixed-order float64 sum of the error shares.
// Nothing here exchanges data between workgroups inside a launch, uses atomics or assumes residency.
#include "evc_deconv_kernels.h"
#include "evc_deconv_learn_plan.h"

#include <math.h>

namespace evc {

namespace {

template <typename T> struct DclGrad {
    const T *Qn, *Qd;       // [n_tiles][MP][16]
    const T* H;
    long hs_t, hs_r;        // H(r, t) = H[t * hs_t + r * hs_r]
    const int4* tpos;       // per tile {first frame, frames, frames of its utterance before it, 0}
    T* part;                // [S][ntap][2][MTp * 16][Rp]
    int MP, MT, MTp, R, Rp, n_tiles, S;
    int tap0, ntap;         // the taps of this launch
};

template <typename T, bool ONE>
__global__ __launch_bounds__(64 * DG_WAVES) void k_deconv_dict_grad(DclGrad<T> a) {
    typedef typename Mma<T>::acc_t acc_t;
    typedef typename DcVec4<T>::type vec_t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int bpo = a.MTp / DG_MB;                 // workgroups per operand along the bins
    const int which = ONE ? 0 : blockIdx.y / bpo;
    const int tile0 = (ONE ? blockIdx.y : blockIdx.y % bpo) * DG_MB;
    const bool sums = ONE && blockIdx.y == 0;
    const int sp = blockIdx.z / a.ntap, k = blockIdx.z % a.ntap;            // k: the tap's index within this launch
    const int tau = a.tap0 + k;
    const int tb = (int)((long)sp * a.n_tiles / a.S), te = (int)((long)(sp + 1) * a.n_tiles / a.S);
    const T* __restrict__ Limg = which ? a.Qd : a.Qn;
    const long img = (long)a.MP * BT_F;
    int moff[DG_MB];
#pragma unroll
    for (int i = 0; i < DG_MB; ++i) {              // tiles past the last one repeat it: their sums land in padding
        const int tile = tile0 + i < a.MT ? tile0 + i : a.MT - 1;
        moff[i] = (tile * 16 + c) * BT_F + 4 * g;
    }
    const int r0 = (blockIdx.x * DG_WAVES + wave) * DG_RB * 16;
    long hoff[DG_RB];
    bool rok[DG_RB];
#pragma unroll
    for (int j = 0; j < DG_RB; ++j) {
        const int r = r0 + 16 * j + c;
        rok[j] = r < a.R;
        hoff[j] = (long)(rok[j] ? r : a.R - 1) * a.hs_r;
    }
    acc_t acc[DG_MB][DG_RB];
    T hs[DG_RB];
#pragma unroll
    for (int j = 0; j < DG_RB; ++j) {
        hs[j] = T(0);
#pragma unroll
        for (int i = 0; i < DG_MB; ++i) acc[i][j] = acc_t{0, 0, 0, 0};
    }
    // one step = one frame tile = 4 MFMAs per accumulator; the next tile's operands are loaded before the current tile's
    // MFMAs are issued
    auto load = [&](int tile, vec_t (&av)[DG_MB], T (&bv)[DG_RB][4]) {
        const int4 tp = a.tpos[tile];
        const T* __restrict__ li = Limg + tile * img;
#pragma unroll
        for (int i = 0; i < DG_MB; ++i) av[i] = *reinterpret_cast<const vec_t*>(li + moff[i]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {              // clamped address, then select
            const int f = 4 * g + s;
            const bool valid = f < tp.y && tau <= tp.z + f;
            const T* __restrict__ hrow = a.H + (long)(tp.x + (valid ? f - tau : 0)) * a.hs_t;
#pragma unroll
            for (int j = 0; j < DG_RB; ++j) {
                const T v = hrow[hoff[j]];
                bv[j][s] = (valid && rok[j]) ? v : T(0);
            }
        }
    };
    vec_t av[DG_MB];
    T bv[DG_RB][4];
    if (tb < te) load(tb, av, bv);
#pragma unroll 1
    for (int tile = tb; tile < te; ++tile) {
        vec_t an[DG_MB];
        T bn[DG_RB][4];
        load(tile + 1 < te ? tile + 1 : tile, an, bn);      // past the end: this tile again, never used
        if (sums) {                                // this lane's frame slots 4 g .. 4 g + 3 of every tile, in order
#pragma unroll
            for (int j = 0; j < DG_RB; ++j)
#pragma unroll
                for (int s = 0; s < 4; ++s) hs[j] += bv[j][s];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < DG_MB; ++i)
#pragma unroll
                for (int j = 0; j < DG_RB; ++j) acc[i][j] = Mma<T>::mma(av[i][s], bv[j][s], acc[i][j]);
#pragma unroll
        for (int i = 0; i < DG_MB; ++i) av[i] = an[i];
#pragma unroll
        for (int j = 0; j < DG_RB; ++j)
#pragma unroll
            for (int s = 0; s < 4; ++s) bv[j][s] = bn[j][s];
    }
    const long slab = (long)a.MTp * 16 * a.Rp;
    T* __restrict__ out = a.part + (((long)sp * a.ntap + k) * 2 + which) * slab;
#pragma unroll
    for (int i = 0; i < DG_MB; ++i)
#pragma unroll
        for (int j = 0; j < DG_RB; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                out[(long)((tile0 + i) * 16 + Mma<T>::row(lane, r)) * a.Rp + r0 + 16 * j + c] = acc[i][j][r];
    if (sums) {                                    // the four lane groups of a component, added in ascending order
#pragma unroll
        for (int j = 0; j < DG_RB; ++j) {
            const T s01 = __shfl(hs[j], c, 64) + __shfl(hs[j], c + 16, 64);
            const T sv = (s01 + __shfl(hs[j], c + 32, 64)) + __shfl(hs[j], c + 48, 64);
            if (lane < 16) out[slab + r0 + 16 * j + c] = sv;
        }
    }
}

// W_tau <- W_tau * (Num / Den) for the ntap taps from tap0 on, the slabs added in the order s = 0 .. S-1
template <typename T>
__global__ __launch_bounds__(256) void k_deconv_dict_apply(const T* __restrict__ part, int S, int tap0, int ntap, long slab, int Rp,
                                                           T* __restrict__ W, long ldw, long tap_stride, int bin_major, int M,
                                                           int R, int kl) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long per_tap = (long)M * R;
    if (idx >= per_tap * ntap) return;
    const int k = (int)(idx / per_tap);
    const long e = idx % per_tap;
    // the caller's inner index is the fastest one here
    const int m = bin_major ? (int)(e / R) : (int)(e % M);
    const int r = bin_major ? (int)(e % R) : (int)(e / M);
    const long step = (long)ntap * 2 * slab;       // from one frame range to the next
    const T* __restrict__ pn = part + (long)k * 2 * slab + (long)m * Rp + r;
    const T* __restrict__ pd = kl ? part + ((long)k * 2 + 1) * slab + r : pn + slab;      // KL: s_r, the second slab's first row
    T num = T(0), den = T(0);
    for (int s = 0; s < S; ++s) {
        num += pn[s * step];
        den += pd[s * step];
    }
    den = den == T(0) ? (kl ? T(1) : (T)BETA_EPS) : den;
    T* w = W + (long)(tap0 + k) * tap_stride + (bin_major ? m * ldw + r : r * ldw + m);
    *w = *w * (num / den);
}

// EVC_DCL_DICT_ONLY: one group of BT_GT bin tiles of V, Qn | Qd and (want_err) the group's share of every frame's error;
// blockIdx.x the frame tile, blockIdx.y the group
template <typename T>
__global__ __launch_bounds__(BT_THREADS) void k_deconv_learn_v(const T* __restrict__ W, long ws_tap, long ws_m, long ws_r, int M,
                                                               int R, const T* __restrict__ H, long hs_t, long hs_r,
                                                               const T* __restrict__ Xp, T* __restrict__ Qn,
                                                               T* __restrict__ Qd, const int4* __restrict__ tiles, int MP,
                                                               int taps, int kl, int want_err, double* __restrict__ errf,
                                                               int n_tiles) {
    __shared__ __attribute__((aligned(16))) T Vs[BT_GT * 16 * BT_F];
    __shared__ double red[256];
    const int tile = blockIdx.x;
    const int4 tl = tiles[tile];
    const int back = tl.y - tiles[tl.w].y;
    const int MT = MP / 16, bt0 = blockIdx.y * BT_GT;
    const int nb = MT - bt0 < BT_GT ? MT - bt0 : BT_GT;
    deconv_form_v<T, false>(W, ws_tap, ws_m, ws_r, M, H, hs_t, hs_r, R, taps, tl.y, tl.z, back, bt0, nb, Vs);
    const long base = ((long)tile * MP + bt0 * 16) * BT_F;
    const T eps = (T)BETA_EPS;
    for (int e = threadIdx.x; e < nb * 16 * BT_F; e += BT_THREADS) {
        T n = T(0), d = T(0);
        if (bt0 * 16 + (e >> 4) < M && (e & 15) < tl.z) {
            const T v = Vs[e], x = Xp[base + e];
            if (kl) {
                n = x / (v < eps ? eps : v);
                d = T(1);
            } else {
                n = x;
                d = v;
            }
        }
        Qn[base + e] = n;
        Qd[base + e] = d;
    }
    if (!want_err) return;
    const int f = threadIdx.x & 15, part = threadIdx.x >> 4;
    double s0 = 0.0;
    for (int m = part; m < nb * 16 && bt0 * 16 + m < M; m += 16) {
        const double x = (double)Xp[base + m * BT_F + f], v = (double)Vs[m * BT_F + f];
        if (kl) {
            const double vv = v < BETA_EPS ? BETA_EPS : v;
            s0 += v;
            if (x > BETA_EPS) s0 += x * log(x / vv) - x;
        } else {
            s0 += (x - v) * (x - v);
        }
    }
    red[part * 16 + f] = s0;
    __syncthreads();
    if (threadIdx.x < 16) {
        double t0 = 0.0;
        for (int p = 0; p < 16; ++p) t0 += red[p * 16 + f];
        errf[((long)blockIdx.y * n_tiles + tile) * BT_F + f] = f < tl.z ? (kl ? t0 : 0.5 * t0) : 0.0;
    }
}

// Xp[tile][m][f] = X(m, first frame + f), zero in the padding bins and frame slots
template <typename T>
__global__ __launch_bounds__(256) void k_dcl_pack_x(const T* __restrict__ X, int ldx, int fm, int M, int MP,
                                                    const int4* __restrict__ tiles, int n_tiles, T* __restrict__ Xp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n_tiles * MP * BT_F) return;
    const int f = (int)(i % BT_F), m = (int)((i / BT_F) % MP);
    const int4 tl = tiles[i / ((long)MP * BT_F)];
    T v = T(0);
    if (m < M && f < tl.z) v = fm ? X[(long)(tl.y + f) * ldx + m] : X[(long)m * ldx + tl.y + f];
    Xp[i] = v;
}

__global__ __launch_bounds__(256) void k_dcl_tile_pos(const int4* __restrict__ tiles, int n_tiles, int4* __restrict__ tpos) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_tiles) return;
    const int4 tl = tiles[i];
    tpos[i] = make_int4(tl.y, tl.z, tl.y - tiles[tl.w].y, 0);
}

// *out = sqrt(2 max(sum of the n shares, 0)), in a fixed order
__global__ __launch_bounds__(256) void k_dcl_err_total(const double* __restrict__ errf, long n, double* __restrict__ out) {
    __shared__ double red[256];
    double acc = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) acc += errf[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sqrt(2.0 * fmax(red[0], 0.0));
}

// arguments already validated by evc_deconv_learn; returns 0, -2 or a hipError_t
template <typename T>
int deconv_learn(const T* X, int ldx, T* W, int ldw, long tap_stride, T* H, int ldh, int M, int R, int T_,
                 const int* utt_offsets, int n_utt, const evc_deconv_learn_opts& o, int forced, void* ws, size_t ws_bytes,
                 int* n_iter_out, double* err_out, hipStream_t s) {
    const DclWs w = carve_deconv_learn(ws, M, R, T_, n_utt, o.taps, o.update, o.dtype);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const bool fm = o.layout == EVC_FRAME_MAJOR, both = o.update == EVC_DCL_BOTH, kl = o.loss == EVC_LOSS_KL;
    const int taps = o.taps, MP = round_up(M, 16), RP = round_up(R, 16);
    const DclPlan plan = dcl_plan(M, R, T_, taps, forced);
    int4* tiles = reinterpret_cast<int4*>(w.tiles);
    int4* tpos = reinterpret_cast<int4*>(w.tpos);
    double* errf = reinterpret_cast<double*>(w.errf);
    double* ring = reinterpret_cast<double*>(w.ring);
    T* Xp = reinterpret_cast<T*>(w.Xp);

    int n_tiles;
    HIP_TRY(frame_tiles_stage(BT_F, utt_offsets, n_utt, T_, tiles, reinterpret_cast<int*>(w.utt_tile0), nullptr, s, &n_tiles));
    HIP_TRY(hipMemsetAsync(w.stop, 0, sizeof(int) * n_utt, s));
    hipLaunchKernelGGL(k_dcl_tile_pos, dim3(dc_blocks_of(n_tiles)), dim3(256), 0, s, tiles, n_tiles, tpos);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_dcl_pack_x<T>, dim3(dc_blocks_of((long)n_tiles * MP * BT_F)), dim3(256), 0, s, X, ldx, fm ? 1 : 0, M, MP,
                       tiles, n_tiles, Xp);
    HIP_TRY(hipGetLastError());

    DcArgs<T> a;                                   // the activation half's kernels (EVC_DCL_BOTH)
    a.Ap1 = reinterpret_cast<T*>(w.Ap1); a.Ap3 = reinterpret_cast<T*>(w.Ap3); a.Xp = Xp;
    a.Qn = reinterpret_cast<T*>(w.Qn); a.Qd = reinterpret_cast<T*>(w.Qd);
    a.H = H; a.hs_t = fm ? ldh : 1; a.hs_n = fm ? 1 : ldh;
    a.tiles = tiles; a.stop = reinterpret_cast<const int*>(w.stop); a.errf = errf;
    a.M = M; a.MP = MP; a.N = R; a.NP = RP; a.taps = taps; a.kl = kl ? 1 : 0; a.n_tiles = n_tiles;
    a.l1 = (T)o.l1_h; a.l2 = (T)o.l2_h;
    if (both)       // per function and process-wide: always the limit of DC_MAX_M, as evc_deconv_solve sets it
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_deconv_update<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)dc_lds_update<T>(DC_MAX_M)));
    const int groups = dcl_bin_groups(M, o.update);

    DclGrad<T> q;
    q.Qn = a.Qn; q.Qd = a.Qd; q.H = H; q.hs_t = a.hs_t; q.hs_r = a.hs_n; q.tpos = tpos;
    q.part = reinterpret_cast<T*>(w.part);
    q.MP = MP; q.MT = MP / 16; q.MTp = learn_bin_tiles(M); q.R = R; q.Rp = round_up(R, 128); q.n_tiles = n_tiles; q.S = plan.S;
    const long slab = (long)q.MTp * 16 * q.Rp;

    auto pack_w = [&]() -> int {
        hipLaunchKernelGGL(k_deconv_pack_dict<T>, dim3(dc_blocks_of((long)taps * RP * MP)), dim3(256), 0, s, W, ldw, tap_stride,
                           fm ? 1 : 0, M, R, RP, MP, taps, reinterpret_cast<T*>(w.Ap1), reinterpret_cast<T*>(w.Ap3));
        return (int)hipGetLastError();
    };
    // the images (and, on a check, the error shares) of the current W and H; packed: W's images are those of the current W
    auto form_v = [&](int want_err, bool packed) -> int {
        if (both) {
            if (!packed) HIP_TRY(pack_w());
            hipLaunchKernelGGL(k_deconv_v<T>, dim3(n_tiles), dim3(BT_THREADS), dc_lds_v<T>(MP), s, a, want_err);
        } else {
            hipLaunchKernelGGL(k_deconv_learn_v<T>, dim3(n_tiles, groups), dim3(BT_THREADS), 0, s, W, tap_stride,
                               fm ? 1L : (long)ldw, fm ? (long)ldw : 1L, M, R, H, a.hs_t, a.hs_n, Xp, a.Qn, a.Qd, tiles, MP, taps,
                               kl ? 1 : 0, want_err, errf, n_tiles);
        }
        return (int)hipGetLastError();
    };
    auto update_w = [&]() -> int {                 // from the images of the current factors, a chunk of taps at a time
        for (int t0 = 0; t0 < taps; t0 += plan.chunk) {
            q.tap0 = t0;
            q.ntap = taps - t0 < plan.chunk ? taps - t0 : plan.chunk;
            const dim3 grid(q.Rp / (DG_WAVES * DG_RB * 16), (kl ? 1 : 2) * q.MTp / DG_MB, plan.S * q.ntap);
            if (kl) hipLaunchKernelGGL((k_deconv_dict_grad<T, true>), grid, dim3(64 * DG_WAVES), 0, s, q);
            else hipLaunchKernelGGL((k_deconv_dict_grad<T, false>), grid, dim3(64 * DG_WAVES), 0, s, q);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_deconv_dict_apply<T>, dim3(dc_blocks_of((long)q.ntap * M * R)), dim3(256), 0, s, q.part, plan.S,
                               t0, q.ntap, slab, q.Rp, W, (long)ldw, tap_stride, fm ? 0 : 1, M, R, kl ? 1 : 0);
            HIP_TRY(hipGetLastError());
        }
        return ST_OK;
    };
    bool fresh = false;                            // the images are those of the current W and H (a check has just formed them)
    auto step = [&]() -> int {
        if (both) {
            if (!fresh) HIP_TRY(form_v(0, false));
            hipLaunchKernelGGL(k_deconv_update<T>, dim3(n_tiles), dim3(BT_THREADS), dc_lds_update<T>(MP), s, a);
            HIP_TRY(hipGetLastError());
            HIP_TRY(form_v(0, true));              // the new H under the same W
        } else if (!fresh) {
            HIP_TRY(form_v(0, false));
        }
        fresh = false;
        return update_w();
    };
    auto error_now = [&](int slot, double* host) -> int {
        HIP_TRY(form_v(1, false));
        fresh = true;
        double* dst = ring + slot % DCL_RING;
        hipLaunchKernelGGL(k_dcl_err_total, dim3(1), dim3(256), 0, s, errf, (long)groups * n_tiles * BT_F, dst);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host, dst, sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return ST_OK;
    };
    auto stop = [&](int, double err, double err_prev, double err_init) { return (err_prev - err) / err_init < o.tol; };
    return learn_loop(o.iters, o.check_every, o.tol, err_out, n_iter_out, o.ev_loop_start, o.ev_loop_stop, s, step, error_now,
                      stop);
}

}  // namespace

}  // namespace evc

extern "C" {

size_t evc_deconv_learn_workspace_bytes(int M, int R, int T, int n_utt, int taps, int update, int dtype) {
    return evc::deconv_learn_workspace_bytes(M, R, T, n_utt, taps, update, dtype);
}

int evc_deconv_learn_splits(int M, int R, int T, int n_utt, int taps) { return evc::deconv_learn_splits(M, R, T, n_utt, taps); }

int evc_deconv_learn(const void* X, int ldx, void* W, int ldw, long tap_stride, void* H, int ldh, int M, int R, int T,
                     const int* utt_offsets, int n_utt, const evc_deconv_learn_opts* opts, void* workspace,
                     size_t workspace_bytes, int* n_iter_out, double* err_out, evc_stream_t stream) {
    using namespace evc;
    int forced;
    HIP_TRY(deconv_learn_args_check(X, ldx, W, ldw, tap_stride, H, ldh, M, R, T, utt_offsets, n_utt, opts, workspace,
                                    workspace_bytes, &forced));
    const evc_deconv_learn_opts& o = *opts;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (o.dtype == EVC_F64)
        return deconv_learn<double>(static_cast<const double*>(X), ldx, static_cast<double*>(W), ldw, tap_stride,
                                    static_cast<double*>(H), ldh, M, R, T, utt_offsets, n_utt, o, forced, workspace,
                                    workspace_bytes, n_iter_out, err_out, s);
    return deconv_learn<float>(static_cast<const float*>(X), ldx, static_cast<float*>(W), ldw, tap_stride,
                               static_cast<float*>(H), ldh, M, R, T, utt_offsets, n_utt, o, forced, workspace, workspace_bytes,
                               n_iter_out, err_out, s);
}

}  // extern "C"
