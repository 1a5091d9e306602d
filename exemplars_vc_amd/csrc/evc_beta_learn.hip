// evc_beta_learn.hip - evc_beta_learn: multiplicative updates of BOTH factors under any beta-divergence: scikit-learn's
// _fit_multiplicative_update with update_H=True for beta_loss = 'itakura-saito' or any float (_nmf.py:526-893).
// DESIGN.md §5.11.
//
// Per iteration: the activations by one k_beta_sweep on the current dictionary (evc_beta.hip; its two packed images
// are rebuilt from W every iteration), with the flush H[H < 2^-52] = 0 at the store when beta < 1; then the dictionary
// with the new H, EPS = 2^-23:
//   V = W H;  Vn = V, below EPS -> EPS if beta < 2;  Vd = the same if beta < 1;  Q1 = X * Vn^(beta-2);  Q2 = Vd^(beta-1)
//   Num = Q1 H^T;  Den = Q2 H^T + l1_w + l2_w W, 0 -> EPS;  W <- W * (Num / Den)^gamma;  W[W < 2^-52] = 0 if beta <= 1
// Num and Den are sums over the frames, taken in S contiguous frame ranges (learn_splits) whose partial sums leave as
// slabs and are added in ascending order by k_beta_dict_apply.  Two routes form the slabs:
//   unfused  V by the generic contraction on frames-as-rows copies, k_beta_dict_q turns it into Q1 (in place) and Q2,
//            k_dict_grad (evc_learn.hip, two-operand form) contracts both against H.  Any R.
//   fused    k_beta_dict_grad: a workgroup owns ONE bin tile x BDG_RB component tiles x one frame range, its four
//            wavefronts a quarter of the range each.  Per step of 16 frames a wavefront forms the tile V^T (16 frames x 16
//            bins) = Ht W^T over all R on the 16x16x4 MFMA with W's tile rows in LDS, turns the accumulator into Q1 and Q2
//            in registers and feeds them back as the LEFT operand of the Num / Den MFMAs: accumulator register r of lane
//            (bin = lane & 15, g = lane >> 4) holds frame row(lane, r), and the k index of an MFMA is only a summation
//            index, so step r contracts the four frames {row(lane, r)} against Ht[that frame][component] with no
//            transpose.  X is read once; V, Q1 and Q2 never reach memory.  The four quarters are added through LDS in
//            wavefront order.  Components beyond the workgroup's BDG_RB tiles go to other workgroups, each of which
//            RECOMPUTES V (no exchange: the V MFMAs are R / 4 per step against 16 for Num and Den).  R <= BDG_MAX_R.
// Nothing here exchanges data between workgroups inside a launch, uses float atomics or assumes residency: the same
// call gives bitwise the same W and H every time.
#include "evc_beta_common.h"

#include <math.h>

namespace evc {

namespace {

constexpr int BDG_LD = 20;            // LDS row length of W's tile image: 4 x 20 elements shift the four lane groups by 16 banks
constexpr int BDG_RB = 2;             // component tiles of 16 per workgroup of k_beta_dict_grad
constexpr int BDG_WAVES = 4;          // wavefronts per workgroup: each takes a quarter of the frame range

template <typename T> struct Vec4;
template <> struct Vec4<double> { typedef f64x4 type; };
template <> struct Vec4<float> { typedef f32x4 type; };

// Vt[t][m] <- Q1, Q2t[t][m] <- Q2 for t < T_, m < Mk (zero from M on), frames as rows
template <typename T>
__global__ __launch_bounds__(256) void k_beta_dict_q(const T* __restrict__ Xt, int ldx, T* __restrict__ Vt,
                                                     T* __restrict__ Q2t, int ldv, int M, int Mk, long rows, int clamp_n,
                                                     int clamp_d, PowSpec p1, PowSpec p2) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= rows * Mk) return;
    const long t = gid / Mk;
    const int m = (int)(gid % Mk);
    const T eps = (T)BETA_EPS;
    T q1 = T(0), q2 = T(0);
    if (m < M) {
        const T v = Vt[t * ldv + m];
        const T vn = (clamp_n && v < eps) ? eps : v;
        const T vd = (clamp_d && v < eps) ? eps : v;
        q1 = pw(vn, p1) * Xt[t * ldx + m];
        q2 = pw(vd, p2);
    }
    Vt[t * ldv + m] = q1;
    Q2t[t * ldv + m] = q2;
}

template <typename T> struct BetaDictArgs {
    const T* Xt;            // [Tp][ldx] frames as rows, zero-padded
    const T* Ht;            // [Tp][ldh] frames as rows, zero-padded, ldh a multiple of 128
    const T* Am;            // [>= M][ldh] bins as rows: the dictionary
    T* part;                // [S][2][MTp * 16][ldh]
    int ldx, ldh;
    int M, R, RP16, MTp, T_, S;
    int clamp_n, clamp_d;
    PowSpec p1, p2;
};

// grid (component groups of BDG_RB tiles, bin tiles, frame ranges); the four wavefronts split the frame range
template <typename T>
__global__ __launch_bounds__(64 * BDG_WAVES) void k_beta_dict_grad(BetaDictArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bdg_lds[];
    typedef typename Mma<T>::acc_t acc_t;
    typedef typename Vec4<T>::type vec_t;
    T* Ws = reinterpret_cast<T*>(bdg_lds);         // [RP16][BDG_LD]: Ws[k][b] = W[bin b of the tile][component k]
    T* red = Ws + a.RP16 * BDG_LD;                 // [BDG_WAVES - 1][2 BDG_RB x 4][64]: the other wavefronts' partial sums
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b16 = lane & 15, g = lane >> 4;
    const int r0 = blockIdx.x * BDG_RB * 16;
    const int m0 = blockIdx.y * 16;
    const int sp = blockIdx.z;
    const int rb = (int)((long)sp * a.T_ / a.S), re = (int)((long)(sp + 1) * a.T_ / a.S);
    // this wavefront's quarter of the range
    const int tb = rb + (int)((long)(re - rb) * wave / BDG_WAVES), te = rb + (int)((long)(re - rb) * (wave + 1) / BDG_WAVES);
    for (int e = threadIdx.x; e < a.RP16 * 16; e += 64 * BDG_WAVES) {
        const int k = e % a.RP16, m = m0 + e / a.RP16;
        const T v = a.Am[(long)(m < a.M ? m : a.M - 1) * a.ldh + (k < a.R ? k : a.R - 1)];
        Ws[k * BDG_LD + e / a.RP16] = (m < a.M && k < a.R) ? v : T(0);
    }
    __syncthreads();
    const int moff = m0 + b16;
    const bool mlive = moff < a.M;
    acc_t num[BDG_RB], den[BDG_RB];
#pragma unroll
    for (int j = 0; j < BDG_RB; ++j) num[j] = den[j] = acc_t{0, 0, 0, 0};
    const int hoff = r0 + b16;
    const int NC = a.RP16 / 16;
    const T eps = (T)BETA_EPS;
#pragma unroll 1
    for (int t0 = tb; t0 < te; t0 += 16) {
        // the frame this lane supplies to V's MFMAs (left operand row b16) and the four its accumulator registers hold;
        // a ragged range: clamped addresses, then a select
        const bool vlive = t0 + b16 < te;
        const T* __restrict__ hv_row = a.Ht + (long)(vlive ? t0 + b16 : te - 1) * a.ldh + 4 * g;
        bool live[4];
        T hb[4][BDG_RB], x[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int fr = t0 + Mma<T>::row(lane, r);
            live[r] = fr < te;
            const long frow = live[r] ? fr : te - 1;
#pragma unroll
            for (int j = 0; j < BDG_RB; ++j) {
                const T h = a.Ht[frow * a.ldh + hoff + 16 * j];
                hb[r][j] = live[r] ? h : T(0);
            }
            x[r] = a.Xt[frow * a.ldx + moff];
        }
        acc_t v = acc_t{0, 0, 0, 0};
#pragma unroll 1
        for (int c = 0; c < NC; ++c) {
            vec_t hv = *reinterpret_cast<const vec_t*>(hv_row + 16 * c);
            const T* __restrict__ wr = Ws + (16 * c + 4 * g) * BDG_LD + b16;
#pragma unroll
            for (int s = 0; s < 4; ++s) v = Mma<T>::mma(vlive ? hv[s] : T(0), wr[s * BDG_LD], v);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const T vn = (a.clamp_n && v[r] < eps) ? eps : v[r];
            const T vd = (a.clamp_d && v[r] < eps) ? eps : v[r];
            const bool on = live[r] && mlive;
            const T q1 = on ? pw(vn, a.p1) * x[r] : T(0);
            const T q2 = on ? pw(vd, a.p2) : T(0);
#pragma unroll
            for (int j = 0; j < BDG_RB; ++j) {
                num[j] = Mma<T>::mma(q1, hb[r][j], num[j]);
                den[j] = Mma<T>::mma(q2, hb[r][j], den[j]);
            }
        }
    }
    // the four quarters, added in wavefront order
    if (wave > 0) {
        T* mine = red + (wave - 1) * (2 * BDG_RB * 4 * 64) + lane;
#pragma unroll
        for (int j = 0; j < BDG_RB; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                mine[(j * 8 + r) * 64] = num[j][r];
                mine[(j * 8 + 4 + r) * 64] = den[j][r];
            }
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll 1
    for (int w = 1; w < BDG_WAVES; ++w) {
        const T* theirs = red + (w - 1) * (2 * BDG_RB * 4 * 64) + lane;
#pragma unroll
        for (int j = 0; j < BDG_RB; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                num[j][r] += theirs[(j * 8 + r) * 64];
                den[j][r] += theirs[(j * 8 + 4 + r) * 64];
            }
    }
    const long slab = (long)a.MTp * 16 * a.ldh;
    T* __restrict__ out = a.part + (long)sp * 2 * slab;
#pragma unroll
    for (int j = 0; j < BDG_RB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long o = (long)(m0 + Mma<T>::row(lane, r)) * a.ldh + hoff + 16 * j;
            out[o] = num[j][r];
            out[slab + o] = den[j][r];
        }
}

// sums the slabs in the order s = 0 .. S-1 and applies the update to the caller's W
template <typename T>
__global__ __launch_bounds__(256) void k_beta_dict_apply(const T* __restrict__ part, int S, long slab, int ldp,
                                                         T* __restrict__ W, long ldw, int bin_major, int M, int R, T l1, T l2,
                                                         int gamma_one, PowSpec pg, T flush) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)M * R) return;
    // the caller's inner index is the fastest one here
    const int m = bin_major ? (int)(idx / R) : (int)(idx % M);
    const int r = bin_major ? (int)(idx % R) : (int)(idx / M);
    const T* __restrict__ p = part + (long)m * ldp + r;
    T num = T(0), den = T(0);
    for (int s = 0; s < S; ++s) {
        num += p[(long)s * 2 * slab];
        den += p[((long)s * 2 + 1) * slab];
    }
    T* wp = W + (bin_major ? m * ldw + r : r * ldw + m);
    const T w = *wp;
    T d = den + l1;
    d = d + l2 * w;
    d = d == T(0) ? (T)BETA_EPS : d;
    T q = num / d;
    if (!gamma_one) q = pw(q, pg);
    T wn = w * q;
    if (flush > T(0) && wn < flush) wn = T(0);
    *wp = wn;
}

template <typename T> size_t bdg_lds_bytes(int RP16) {
    return ((size_t)RP16 * BDG_LD + (size_t)(BDG_WAVES - 1) * 2 * BDG_RB * 4 * 64) * sizeof(T);
}

}  // namespace

template <typename T> int beta_dict_sums_prepare(bool fused) {
    if (fused)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_beta_dict_grad<T>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)bdg_lds_bytes<T>(BDG_MAX_R)));
    return 0;
}

template <typename T> int beta_dict_sums(const BetaDictSums<T>& q, hipStream_t s) {
    const int Mk = round_up(q.M, 16), Mj = round_up(q.M, 64), Np = round_up(q.R, 128), MTp = learn_bin_tiles(q.M);
    const PowSpec p1 = pow_spec(q.beta - 2.0), p2 = pow_spec(q.beta - 1.0);
    const int clamp_n = q.beta - 2.0 < 0 ? 1 : 0, clamp_d = q.beta - 1.0 < 0 ? 1 : 0;
    if (q.fused) {
        BetaDictArgs<T> a;
        a.Xt = q.Xt; a.Ht = q.Ht; a.Am = q.Am; a.part = q.part;
        a.ldx = Mk; a.ldh = Np;
        a.M = q.M; a.R = q.R; a.RP16 = round_up(q.R, 16); a.MTp = MTp; a.T_ = q.T_; a.S = q.S;
        a.clamp_n = clamp_n; a.clamp_d = clamp_d; a.p1 = p1; a.p2 = p2;
        const dim3 grid(round_up(q.R, BDG_RB * 16) / (BDG_RB * 16), Mk / 16, q.S);
        hipLaunchKernelGGL(k_beta_dict_grad<T>, grid, dim3(64 * BDG_WAVES), bdg_lds_bytes<T>(a.RP16), s, a);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    HIP_TRY(gemm_nt<T>(q.Ht, Np, q.Am, Np, q.Vt, Mj, q.Tp, Mj, Np, s, nullptr, 0, nullptr, Mk));
    const long n = (long)q.T_ * Mk;
    hipLaunchKernelGGL(k_beta_dict_q<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, q.Xt, Mk, q.Vt, q.Q2t, Mj, q.M, Mk,
                       (long)q.T_, clamp_n, clamp_d, p1, p2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(dict_grad<T>(q.Vt, Mj, q.Q2t, Mj, q.Ht, Np, q.M, q.T_, q.S, q.part, s));
    return 0;
}

template int beta_dict_sums_prepare<double>(bool);
template int beta_dict_sums_prepare<float>(bool);
template int beta_dict_sums<double>(const BetaDictSums<double>&, hipStream_t);
template int beta_dict_sums<float>(const BetaDictSums<float>&, hipStream_t);

namespace {

template <typename T> struct BlWs {
    T *Xt, *Am, *Ht, *Vt, *Q2t, *part;
    char* beta_ws;
    size_t beta_bytes, bytes;
};

// [Xt | Am | Ht | Vt | Q2t | part | the activation half's workspace], each 256-byte aligned (ws == NULL: sizes only)
template <typename T> BlWs<T> carve_bl(void* ws, const Dims& d) {
    BlWs<T> w;
    Carver c = Carver::rounded(ws);
    w.Xt = c.take<T>((size_t)d.Tp * d.Mk);
    w.Am = c.take<T>((size_t)d.Mj * d.Np);
    w.Ht = c.take<T>((size_t)d.Tp * d.Np);
    w.Vt = c.take<T>((size_t)d.Tp * d.Mj);
    w.Q2t = c.take<T>((size_t)d.Tp * d.Mj);
    w.part = c.take<T>((size_t)LEARN_MAX_SPLITS * 2 * learn_bin_tiles(d.M) * 16 * d.Np);
    w.beta_bytes = beta_workspace_bytes(d.M, d.N, d.T_, 1, sizeof(T) == 8 ? EVC_F64 : EVC_F32);
    w.beta_ws = c.take<char>(w.beta_bytes);
    w.bytes = c.bytes();
    return w;
}

bool bl_sizes_ok(int M, int R, int T_, int dtype) {
    return M >= 1 && R >= 1 && T_ >= 1 && M <= BETA_MAX_M && R <= LEARN_MAX_R && (dtype == EVC_F64 || dtype == EVC_F32);
}

size_t bl_workspace_bytes(int M, int R, int T_, int dtype) {
    if (!bl_sizes_ok(M, R, T_, dtype)) return 0;
    return (dtype == EVC_F64 ? carve_bl<double>(nullptr, make_dims(8, M, R, T_, 1)).bytes
                             : carve_bl<float>(nullptr, make_dims(4, M, R, T_, 1)).bytes) + 256;
}

// arguments already validated by evc_beta_learn; returns ST_OK, ST_WORKSPACE or a hipError_t
template <typename T>
int beta_learn(const void* X_, int ldx, void* W_, int ldw, void* H_, int ldh, int M, int R, int T_,
               const evc_beta_learn_opts& o, int S, bool fused, void* ws, size_t ws_bytes, int* n_iter_out, double* err_out,
               hipStream_t s) {
    const Dims d = make_dims((int)sizeof(T), M, R, T_, 1);
    const BlWs<T> w = carve_bl<T>(ws, d);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const int MTp = learn_bin_tiles(M);
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    const T* X = static_cast<const T*>(X_);
    T* W = static_cast<T*>(W_);
    T* H = static_cast<T*>(H_);
    const double beta = o.beta;

    BetaCtx<T> c;
    HIP_TRY(beta_begin<T>(c, X, ldx, H, ldh, M, R, T_, nullptr, 1, o.layout, beta, o.l1_h, o.l2_h, beta < 1.0 ? BETA_E64 : 0.0,
                          n_slots_for(o.iters, o.check_every), w.beta_ws, w.beta_bytes, s));
    const double gamma = beta_gamma(beta);
    const PowSpec pg = pow_spec(gamma);

    BetaDictSums<T> q;
    q.Xt = w.Xt; q.Ht = w.Ht; q.Am = w.Am; q.Vt = w.Vt; q.Q2t = w.Q2t; q.part = w.part;
    q.M = M; q.R = R; q.T_ = T_; q.Tp = d.Tp; q.S = S; q.fused = fused; q.beta = beta;
    auto update_w = [&]() -> int {
        // frames-as-rows copies of the current factors (Ht is the right operand of the sums over the frames)
        HIP_TRY(copy2d<T>(W, ldw, M, R, fm ? 1 : 0, w.Am, d.Np, d.Mj, d.Np, 0, s));
        HIP_TRY(copy2d<T>(H, ldh, T_, R, fm ? 0 : 1, w.Ht, d.Np, d.Tp, d.Np, 0, s));
        HIP_TRY(beta_dict_sums<T>(q, s));
        const long n = (long)M * R;
        hipLaunchKernelGGL(k_beta_dict_apply<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w.part, S,
                           (long)MTp * 16 * d.Np, d.Np, W, (long)ldw, fm ? 0 : 1, M, R, (T)o.l1_w, (T)o.l2_w,
                           gamma == 1.0 ? 1 : 0, pg, (T)(beta <= 1.0 ? BETA_E64 : 0.0));
        HIP_TRY(hipGetLastError());
        return 0;
    };
    // the error of the current factors: the activation half's error kernels on freshly packed dictionary images
    auto error_now = [&](int slot, double* host) -> int {
        HIP_TRY(beta_pack_dict<T>(c, W, ldw, s));
        HIP_TRY(beta_check<T>(c, slot, o.check_every, EVC_STOP_NONE, 0.0, s));
        HIP_TRY(hipMemcpyAsync(host, c.w.trace + slot, sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return 0;
    };

    HIP_TRY(copy2d<T>(X, ldx, T_, M, fm ? 0 : 1, w.Xt, d.Mk, d.Tp, d.Mk, 0, s));
    HIP_TRY(beta_dict_sums_prepare<T>(fused));
    auto step = [&]() -> int {
        HIP_TRY(beta_pack_dict<T>(c, W, ldw, s));
        HIP_TRY(beta_sweep<T>(c, s));
        return update_w();
    };
    auto stop = [&](int, double err, double err_prev, double err_init) { return (err_prev - err) / err_init < o.tol; };
    return learn_loop(o.iters, o.check_every, o.tol, err_out, n_iter_out, o.ev_loop_start, o.ev_loop_stop, s, step, error_now,
                      stop);
}

}  // namespace

}  // namespace evc

extern "C" {

size_t evc_beta_learn_workspace_bytes(int M, int R, int T, int dtype) { return evc::bl_workspace_bytes(M, R, T, dtype); }

int evc_beta_learn_splits(int M, int R, int T) {
    return evc::bl_sizes_ok(M, R, T, EVC_F64) ? evc::learn_splits(M, R, T) : 0;
}

int evc_beta_learn_route(int M, int R, int T) {
    if (!evc::bl_sizes_ok(M, R, T, EVC_F64)) return 0;
    return R <= evc::BDG_ROUTE_R ? evc::ROUTE_FUSED : evc::ROUTE_UNFUSED;
}

int evc_beta_learn(const void* X, int ldx, void* W, int ldw, void* H, int ldh, int M, int R, int T,
                   const evc_beta_learn_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out, double* err_out,
                   evc_stream_t stream) {
    using namespace evc;
    if (!opts || opts->struct_bytes != (int)sizeof(evc_beta_learn_opts)) return ST_BADARG;
    const evc_beta_learn_opts& o = *opts;
    int forced;
    HIP_TRY(learn_args_ok(M, R, T, o.dtype, o.layout, X, W, H, workspace, ldx, ldw, ldh, o.reserved, 0x3ff00, &forced));
    const int route = (o.reserved >> 16) & 3;
    if (o.iters < 0 || o.check_every < 0 || route == 3) return ST_BADARG;
    if (!(o.beta - o.beta == 0.0)) return ST_BADARG;               // NaN or infinite
    if (!(o.tol >= 0.0) || !(o.l1_h >= 0.0) || !(o.l2_h >= 0.0) || !(o.l1_w >= 0.0) || !(o.l2_w >= 0.0)) return ST_BADARG;
    if (o.check_every > 0 && o.iters / o.check_every + 1 > BETA_MAX_SLOTS) return ST_BADARG;
    if (M > BETA_MAX_M || R > LEARN_MAX_R) return ST_UNSUPPORTED;
    if (route == ROUTE_FUSED && R > BDG_MAX_R) return ST_UNSUPPORTED;
    if (workspace_bytes < bl_workspace_bytes(M, R, T, o.dtype)) return ST_WORKSPACE;
    const int S = forced ? forced : learn_splits(M, R, T);
    const bool fused = route == ROUTE_FUSED || (route == ROUTE_AUTO && R <= BDG_ROUTE_R);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return (o.dtype == EVC_F64 ? beta_learn<double> : beta_learn<float>)(X, ldx, W, ldw, H, ldh, M, R, T, o, S, fused,
                                                                          workspace, workspace_bytes, n_iter_out, err_out, s);
}

}  // extern "C"
