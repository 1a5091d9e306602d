// evc_mu_masked.hip - evc_mu_masked_solve: multiplicative updates of the activations with a weight per bin of every frame
// (missing data), the dictionary fixed: deComP's Likelihood.update_x (decomp/nmf_methods/grads.py:77-84, 108-115, 143-150), the
// activation half of nmf.solve(method='mu', likelihood='l2' | 'kl', mask=...) - and evc_mu_masked_learn, that nmf.solve itself
// (the dictionary half sits below the solve's driver).  DESIGN.md §5.22.
//
// Per iteration and frame, with J = 1e-15 (deComP's _JITTER, in both element types) and mask = 1 without one:
//   l2:  V = A h;      Num = A^T (mask . x);          Den = A^T (mask . V)
//   kl:  V = A h + J;  Num = A^T ((mask . x) / V);    Den = A^T mask
//   h <- (h * max(Num, 0)) / max(Den, J)              (the product first, then the quotient; a NaN passes both maxima)
// A^T (mask . (A h)) is not (A^T A) h: the update needs the factored sweep with the weights applied between the two
// contractions - k_beta_sweep's geometry (evc_beta.hip): one launch per iteration, a workgroup of four wavefronts owns a tile
// of 16 frames of ONE utterance, the dictionary is streamed from k_beta_sweep's two packed images.
//   phase 1  V = A H over all N on the matrix cores into the LDS image V[bin][frame] (beta_form_v, evc_beta_common.h)
//   phase 2  V -> Q1 | Q2 in place: l2 XM | mask . V, kl XM / (V + J) | mask, with XM = mask . X and mask packed once per
//            call in the tile's own order (k_mum_pack)
//   phase 3  the wavefronts split the exemplar tiles of 16; a tile's Num and Den are one pass A_tile^T [Q1 | Q2] over the
//            bins, then H is updated in place in the caller's memory (either layout, any leading dimension)
// In the KL solve Den = A^T mask does not change while the dictionary is fixed; keeping the first iteration's in memory and
// loading it instead of the second MFMA chain was measured and is slower: Den is formed every iteration.
// A frame's arithmetic depends on no other frame: a batch gives bitwise the per-utterance results, a NaN stays in its
// frame's column, and a frame whose mask is all zero gets (h * 0) / J = 0.  No exchange between workgroups, no float atomics,
// no residency assumption: the same call gives the same bits every time.
//
// k_mum_err forms V the same way and leaves every frame's share of the error (float64); k_mum_check sums an utterance's
// shares in a fixed order, records the error and applies the family's stop rule on the device, as k_beta_check does.
#include "evc_mu_masked_common.h"
#include "evc_solve_state.h"

namespace evc {

static_assert(MUM_F == BT_F && MUM_MAX_M == BETA_MAX_M && MUM_MAX_SLOTS == BETA_MAX_SLOTS, "evc_mu_masked_plan.h restates evc_beta_common.h");

namespace {

template <typename T, int LOSS>
__global__ __launch_bounds__(BT_THREADS) void k_mum_sweep(MumArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mum_lds[];
    typedef typename Mma<T>::acc_t acc_t;
    typedef typename Vec4<T>::type vec_t;
    const int tile = blockIdx.x;
    const int4 tl = a.tiles[tile];
    if (a.stop[tl.x] != 0) return;
    T* Q1 = reinterpret_cast<T*>(mum_lds);
    T* Q2 = Q1 + a.MP * BT_F;
    const T jit = (T)MUM_J;
    beta_form_v<T>(a, tl, Q1);
    // phase 2: V -> Q1 | Q2
    {
        const T* XMt = a.XMp + (long)tile * a.MP * BT_F;
        const T* Mt = a.Mp + (long)tile * a.MP * BT_F;
        for (int e = threadIdx.x; e < a.MP * BT_F; e += BT_THREADS) {
            T q1 = T(0), q2 = T(0);
            if ((e >> 4) < a.M) {
                const T v = Q1[e];
                if (LOSS == EVC_LOSS_KL) {
                    q1 = XMt[e] / (v + jit);
                    q2 = Mt[e];
                } else {
                    q1 = XMt[e];
                    q2 = Mt[e] * v;
                }
            }
            Q1[e] = q1;
            Q2[e] = q2;
        }
    }
    __syncthreads();
    // phase 3: Num | Den of an exemplar tile, then the update
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int f = lane & 15, g = lane >> 4;
    const bool fvalid = f < tl.z;
    T* Hf = a.H + (long)(tl.y + (fvalid ? f : 0)) * a.hs_t;
    const int NT = a.NP / 16, MC = a.MP / 16;
#pragma unroll 1
    for (int nt = wave; nt < NT; nt += BT_WAVES) {
        acc_t num = acc_t{0, 0, 0, 0}, den = acc_t{0, 0, 0, 0};
        const T* Ar = a.Ap3 + (long)(nt * 16 + f) * a.MP + g * 4;
        for (int c = 0; c < MC; ++c) {
            const vec_t av = *reinterpret_cast<const vec_t*>(Ar + c * 16);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int row = c * 16 + s * 4 + g;
                num = Mma<T>::mma(av[s], Q1[row * BT_F + f], num);
                den = Mma<T>::mma(av[s], Q2[row * BT_F + f], den);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = nt * 16 + Mma<T>::row(lane, r);
            if (fvalid && n < a.N) {
                T* hp = Hf + (long)n * a.hs_n;
                const T hp_num = *hp * max_nan(num[r], T(0));
                *hp = hp_num / max_nan(den[r], jit);
            }
        }
    }
}

// errf[slot] = the frame's share of the error: l2 sum_m mask (x - V)^2, kl sum_m mask (x log(x / V) - x + V) with
// V = A h + J (x = 0: mask V), float64
template <typename T>
__global__ __launch_bounds__(BT_THREADS) void k_mum_err(MumArgs<T> a, int loss) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mum_lds[];
    const int tile = blockIdx.x;
    const int4 tl = a.tiles[tile];
    if (a.stop[tl.x] != 0) return;
    T* Vs = reinterpret_cast<T*>(mum_lds);
    double* red = reinterpret_cast<double*>(mum_lds + (size_t)a.MP * BT_F * sizeof(T));      // [16 parts][16 frames]
    beta_form_v<T>(a, tl, Vs);
    const T* Xt = a.Xp + (long)tile * a.MP * BT_F;
    const T* Mt = a.Mp + (long)tile * a.MP * BT_F;
    const int f = threadIdx.x & 15, part = threadIdx.x >> 4;
    double s0 = 0.0;
    for (int m = part; m < a.M; m += 16) {
        const double x = (double)Xt[m * BT_F + f], v = (double)Vs[m * BT_F + f], w = (double)Mt[m * BT_F + f];
        if (loss == EVC_LOSS_KL) {
            const double vj = v + MUM_J;
            s0 += w * (x > 0.0 ? x * log(x / vj) - x + vj : vj);
        } else {
            const double d = x - v;
            s0 += w * (d * d);
        }
    }
    red[part * 16 + f] = s0;
    __syncthreads();
    if (threadIdx.x < 16) {
        double t0 = 0.0;
        for (int p = 0; p < 16; ++p) t0 += red[p * 16 + f];
        a.errf[(long)tile * BT_F + f] = f < tl.z ? t0 : 0.0;
    }
}

// one block per utterance: the shares summed in a fixed order, err = sqrt(sum) (l2) or sqrt(2 max(sum, 0)) (kl; a NaN
// passes the maximum); check c (0: the start)
__global__ __launch_bounds__(256) void k_mum_check(const double* __restrict__ errf, const int* __restrict__ utt_tile0,
                                                   int* stop, double* einit, double* eprev, double* trace, int n_slots, int c,
                                                   int check_every, int stop_rule, double tol, int loss) {
    __shared__ double red[256];
    const int u = blockIdx.x;
    const long i0 = (long)utt_tile0[u] * BT_F, i1 = (long)utt_tile0[u + 1] * BT_F;
    if (stop[u] != 0 || i0 == i1) return;       // uniform per block
    double acc = 0.0;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) acc += errf[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double err = loss == EVC_LOSS_KL ? sqrt(2.0 * max_nan(red[0], 0.0)) : sqrt(red[0]);
    trace[(long)u * n_slots + c] = err;
    if (c == 0) {
        einit[u] = err;
        eprev[u] = err;
        return;
    }
    if (stop_rule == EVC_STOP_SKLEARN && (eprev[u] - err) / einit[u] < tol) stop[u] = c * check_every;
    else eprev[u] = err;
}

// Xp | XMp | Mp: X, mask . X and mask (NULL: 1) in the tile's order [tile][bin][frame slot], zero in the padding
template <typename T>
__global__ void k_mum_pack(const T* __restrict__ X, int ldx, const T* __restrict__ mask, int ldm, int fm, int M, int MP,
                           const int4* __restrict__ tiles, int n_tiles, T* __restrict__ Xp, T* __restrict__ XMp,
                           T* __restrict__ Mp) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n_tiles * MP * BT_F) return;
    const int4 tl = tiles[i / ((long)MP * BT_F)];
    const int m = (int)((i / BT_F) % MP), f = (int)(i % BT_F);
    T x = T(0), w = T(0), xm = T(0);
    if (m < M && f < tl.z) {
        x = fm ? X[(long)(tl.y + f) * ldx + m] : X[(long)m * ldx + tl.y + f];
        w = !mask ? T(1) : fm ? mask[(long)(tl.y + f) * ldm + m] : mask[(long)m * ldm + tl.y + f];
        xm = x * w;
    }
    Xp[i] = x;
    XMp[i] = xm;
    Mp[i] = w;
}

// every activation of the call's frames starts at `value` (EVC_INIT_CONST)
template <typename T>
__global__ void k_mum_fill(T* __restrict__ H, long hs_t, long hs_n, int N, const int4* __restrict__ tiles, int n_tiles,
                           double value) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n_tiles * BT_F * N) return;
    const long slot = i / N;
    const int n = (int)(i % N), f = (int)(slot % BT_F);
    const int4 tl = tiles[slot / BT_F];
    if (f < tl.z) H[(long)(tl.y + f) * hs_t + (long)n * hs_n] = (T)value;
}

// stop = 0 (running), trace = NaN (not evaluated); n_slots >= 1
__global__ void k_mum_state(int* stop, double* trace, int n_utt, int n_slots) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_utt) stop[i] = 0;
    if (i < (long)n_utt * n_slots) trace[i] = __builtin_nan("");
}

unsigned mum_blocks(long n) { return (unsigned)((n + 255) / 256); }

template <typename T> size_t mum_sweep_lds(int MP) { return (size_t)2 * MP * BT_F * sizeof(T); }
template <typename T> size_t mum_err_lds(int MP) { return (size_t)MP * BT_F * sizeof(T) + 256 * sizeof(double); }

}  // namespace

// ----- the host steps evc_mu_stoch_learn shares (evc_mu_masked_common.h) -----
template <typename T> int mum_sweep(const MumArgs<T>& a, int loss, int n_tiles, hipStream_t s) {
    if (loss == EVC_LOSS_KL)
        hipLaunchKernelGGL((k_mum_sweep<T, EVC_LOSS_KL>), dim3(n_tiles), dim3(BT_THREADS), mum_sweep_lds<T>(a.MP), s, a);
    else
        hipLaunchKernelGGL((k_mum_sweep<T, EVC_LOSS_FROBENIUS>), dim3(n_tiles), dim3(BT_THREADS), mum_sweep_lds<T>(a.MP), s, a);
    return (int)hipGetLastError();
}

// the attribute is per function and process-wide: always the limit of MUM_MAX_M (see beta_begin)
template <typename T> int mum_sweep_prepare() {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mum_sweep<T, EVC_LOSS_FROBENIUS>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)mum_sweep_lds<T>(MUM_MAX_M)));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mum_sweep<T, EVC_LOSS_KL>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)mum_sweep_lds<T>(MUM_MAX_M)));
    return 0;
}

// the two dictionary images are k_beta_sweep's: packed by its host step (A addressed as in evc_beta_solve)
template <typename T> int mum_pack_dict(const MumCtx<T>& c, const T* A, int lda, hipStream_t s) {
    BetaCtx<T> bc{};
    bc.n_tiles = c.n_tiles; bc.fm = c.fm;
    bc.a.M = c.a.M; bc.a.MP = c.a.MP; bc.a.N = c.a.N; bc.a.NP = c.a.NP;
    bc.w.Ap1 = reinterpret_cast<T*>(c.w.Ap1); bc.w.Ap3 = reinterpret_cast<T*>(c.w.Ap3);
    return beta_pack_dict<T>(bc, A, lda, s);
}

namespace {

// carves the workspace, stages the tile table, clears the stop state and the trace, packs X | mask . X | mask and fills the
// kernel arguments; returns 0, -2 or a hipError_t
template <typename T>
int mum_begin(MumCtx<T>& c, const T* X, int ldx, const T* mask, int ldm, T* H, int ldh, int M, int N, int T_,
              const int* utt_offsets, int n_utt, int layout, int n_slots, void* ws, size_t ws_bytes, hipStream_t s) {
    c.w = carve_mum(ws, M, N, T_, n_utt, sizeof(T) == 8 ? EVC_F64 : EVC_F32);
    const MumWs& w = c.w;
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const bool fm = layout == EVC_FRAME_MAJOR;
    const int MP = round_up(M, 16), NP = round_up(N, 16);
    c.n_utt = n_utt; c.n_slots = n_slots; c.fm = fm ? 1 : 0;
    HIP_TRY(frame_tiles_stage(BT_F, utt_offsets, n_utt, T_, w.tiles, w.utt_tile0, nullptr, s, &c.n_tiles));
    hipLaunchKernelGGL(k_mum_state, dim3(mum_blocks((long)n_utt * n_slots)), dim3(256), 0, s, w.stop, w.trace, n_utt, n_slots);
    HIP_TRY(hipGetLastError());
    MumArgs<T>& a = c.a;
    a.Ap1 = reinterpret_cast<T*>(w.Ap1); a.Ap3 = reinterpret_cast<T*>(w.Ap3);
    a.Xp = reinterpret_cast<T*>(w.Xp); a.XMp = reinterpret_cast<T*>(w.XMp); a.Mp = reinterpret_cast<T*>(w.Mp);
    a.H = H;
    a.hs_t = fm ? ldh : 1; a.hs_n = fm ? 1 : ldh;
    a.tiles = w.tiles; a.stop = w.stop; a.errf = w.errf;
    a.M = M; a.MP = MP; a.N = N; a.NP = NP;
    if (c.n_tiles == 0) return 0;
    HIP_TRY(mum_sweep_prepare<T>());
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mum_err<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)mum_err_lds<T>(MUM_MAX_M)));
    hipLaunchKernelGGL(k_mum_pack<T>, dim3(mum_blocks((long)c.n_tiles * MP * BT_F)), dim3(256), 0, s, X, ldx, mask, ldm,
                       fm ? 1 : 0, M, MP, (const int4*)w.tiles, c.n_tiles, reinterpret_cast<T*>(w.Xp),
                       reinterpret_cast<T*>(w.XMp), reinterpret_cast<T*>(w.Mp));
    return (int)hipGetLastError();
}

// check number `chk` (0: the start): every utterance's error into its trace slot, then the stop rule on the device
template <typename T>
int mum_check(const MumCtx<T>& c, int chk, int check_every, int stop_rule, double tol, int loss, hipStream_t s) {
    if (c.n_tiles == 0) return 0;
    const MumWs& w = c.w;
    hipLaunchKernelGGL(k_mum_err<T>, dim3(c.n_tiles), dim3(BT_THREADS), mum_err_lds<T>(c.a.MP), s, c.a, loss);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_mum_check, dim3(c.n_utt), dim3(256), 0, s, (const double*)w.errf, (const int*)w.utt_tile0, w.stop,
                       w.einit, w.eprev, w.trace, c.n_slots, chk, check_every, stop_rule, tol, loss);
    return (int)hipGetLastError();
}

// arguments already validated by evc_mu_masked_solve; returns 0, -2 or a hipError_t
template <typename T>
int mum_solve(const T* A, int lda, const T* X, int ldx, const T* mask, int ldm, T* H, int ldh, int M, int N, int T_,
              const int* utt_offsets, int n_utt, const evc_mu_masked_opts& o, void* ws, size_t ws_bytes, int* n_iter_out,
              double* err_out, hipStream_t s) {
    const int n_slots = mum_slots(o.iters, o.check_every);
    MumCtx<T> c;
    HIP_TRY(mum_begin<T>(c, X, ldx, mask, ldm, H, ldh, M, N, T_, utt_offsets, n_utt, o.layout, n_slots, ws, ws_bytes, s));
    const int n_tiles = c.n_tiles;
    const bool checks = o.check_every > 0;
    if (n_tiles > 0) {
        HIP_TRY(mum_pack_dict<T>(c, A, lda, s));
        if (o.init_mode == EVC_INIT_CONST) {
            hipLaunchKernelGGL(k_mum_fill<T>, dim3(mum_blocks((long)n_tiles * BT_F * N)), dim3(256), 0, s, H, c.a.hs_t, c.a.hs_n, N,
                               (const int4*)c.w.tiles, n_tiles, o.init_value);
            HIP_TRY(hipGetLastError());
        }
        if (checks) HIP_TRY(mum_check<T>(c, 0, o.check_every, o.stop_rule, o.tol, o.loss, s));
    }
    if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
    for (int it = 1; n_tiles > 0 && it <= o.iters; ++it) {
        HIP_TRY(mum_sweep<T>(c.a, o.loss, n_tiles, s));
        if (checks && it % o.check_every == 0) HIP_TRY(mum_check<T>(c, it / o.check_every, o.check_every, o.stop_rule, o.tol, o.loss, s));
    }
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    return solve_read_back(c.w.stop, c.w.trace, n_utt, n_slots, o.iters, n_iter_out, err_out, s);
}

// ----- evc_mu_masked_learn: the dictionary half (deComP's Likelihood.update_d, then utils/normalize.py l2_strict) on the
// unfused route of evc_beta_learn - V by the generic contraction on frames-as-rows copies, k_mum_dict_q turns it into Q1 | Q2,
// k_dict_grad (evc_learn.hip, two-operand form) contracts both against H over S frame ranges, k_mum_dict_apply sums the slabs
// in order and updates, normalises and compares one atom per workgroup -----

// Q1t | Q2t [Tp][ldq] from Vt and the caller's X and mask: l2 mask . X | mask . V, kl (mask . X) / (V + J) | mask; zero where
// m >= M or t >= T_
template <typename T, int LOSS>
__global__ __launch_bounds__(256) void k_mum_dict_q(const T* __restrict__ X, int ldx, const T* __restrict__ mask, int ldm, int fm,
                                                    const T* __restrict__ Vt, T* __restrict__ Q1t, T* __restrict__ Q2t, int ldq,
                                                    int M, int T_, long rows) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= rows * ldq) return;
    const long t = gid / ldq;
    const int m = (int)(gid % ldq);
    T q1 = T(0), q2 = T(0);
    if (m < M && t < T_) {
        const T x = fm ? X[t * ldx + m] : X[(long)m * ldx + t];
        const T w = !mask ? T(1) : fm ? mask[t * ldm + m] : mask[(long)m * ldm + t];
        const T v = Vt[gid];
        if (LOSS == EVC_LOSS_KL) {
            q1 = (x * w) / (v + (T)MUM_J);
            q2 = w;
        } else {
            q1 = x * w;
            q2 = w * v;
        }
    }
    Q1t[gid] = q1;
    Q2t[gid] = q2;
}

}  // namespace

template <typename T>
int mum_dict_q(int loss, const T* X, int ldx, const T* mask, int ldm, int fm, const T* Vt, T* Q1t, T* Q2t, int ldq, int M, int T_,
               long rows, hipStream_t s) {
    const long n = rows * ldq;
    if (loss == EVC_LOSS_KL)
        hipLaunchKernelGGL((k_mum_dict_q<T, EVC_LOSS_KL>), dim3(mum_blocks(n)), dim3(256), 0, s, X, ldx, mask, ldm, fm, Vt, Q1t, Q2t,
                           ldq, M, T_, rows);
    else
        hipLaunchKernelGGL((k_mum_dict_q<T, EVC_LOSS_FROBENIUS>), dim3(mum_blocks(n)), dim3(256), 0, s, X, ldx, mask, ldm, fm, Vt,
                           Q1t, Q2t, ldq, M, T_, rows);
    return (int)hipGetLastError();
}

namespace {

constexpr int MDA_PER = (MUM_MAX_M + 255) / 256;      // bins per thread of k_mum_dict_apply

// One workgroup per atom r.  update: w <- (w max(Num, 0)) / max(Den, J) with Num | Den the slabs summed in the order
// s = 0 .. S-1 (else w is kept: the normalisation of the start).  Then the atom is divided by its Euclidean norm (the squares
// summed per thread over its bins in ascending order, then a tree over the threads: a zero atom becomes NaN, as in numpy) and
// astat[r] = max_m |w_old - w_new|; both reductions in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void k_mum_dict_apply(const T* __restrict__ part, int S, long slab, int ldp, T* __restrict__ W,
                                                        long ldw, int bin_major, int M, int update, double* __restrict__ astat) {
    __shared__ double red[256];
    const int r = blockIdx.x;
    T wo[MDA_PER], wn[MDA_PER];
    T ss = T(0);
#pragma unroll
    for (int i = 0; i < MDA_PER; ++i) {
        const int m = threadIdx.x + 256 * i;
        wo[i] = wn[i] = T(0);
        if (m < M) {
            const T w = W[bin_major ? (long)m * ldw + r : (long)r * ldw + m];
            T v = w;
            if (update) {
                const T* __restrict__ p = part + (long)m * ldp + r;
                T num = T(0), den = T(0);
                for (int s = 0; s < S; ++s) {
                    num += p[(long)s * 2 * slab];
                    den += p[((long)s * 2 + 1) * slab];
                }
                const T wp = w * max_nan(num, T(0));
                v = wp / max_nan(den, (T)MUM_J);
            }
            wo[i] = w;
            wn[i] = v;
            ss += v * v;
        }
    }
    red[threadIdx.x] = (double)ss;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] = (double)((T)red[threadIdx.x] + (T)red[threadIdx.x + k]);
        __syncthreads();
    }
    const T norm = sqrt((T)red[0]);
    __syncthreads();
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < MDA_PER; ++i) {
        const int m = threadIdx.x + 256 * i;
        if (m < M) {
            const T v = wn[i] / norm;
            W[bin_major ? (long)m * ldw + r : (long)r * ldw + m] = v;
            d = max_pass_nan(d, fabs((double)(wo[i] - v)));
        }
    }
    red[threadIdx.x] = d;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] = max_pass_nan(red[threadIdx.x], red[threadIdx.x + k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) astat[r] = red[0];
}

// *stat = max_r astat[r] in a fixed order (a NaN passes)
__global__ __launch_bounds__(256) void k_mum_stat(const double* __restrict__ astat, int R, double* __restrict__ stat) {
    __shared__ double red[256];
    double d = 0.0;
    for (int r = threadIdx.x; r < R; r += 256) d = max_pass_nan(d, astat[r]);
    red[threadIdx.x] = d;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] = max_pass_nan(red[threadIdx.x], red[threadIdx.x + k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *stat = red[0];
}

// arguments already validated by evc_mu_masked_learn; returns ST_OK, ST_WORKSPACE or a hipError_t
template <typename T>
int mum_learn(const void* X_, int ldx, const void* mask_, int ldm, void* W_, int ldw, void* H_, int ldh, int M, int R, int T_,
              const evc_mu_masked_learn_opts& o, int S, void* ws, size_t ws_bytes, int* n_iter_out, double* stat_out,
              hipStream_t s) {
    const Dims d = make_dims((int)sizeof(T), M, R, T_, 1);
    const MumLearnWs w = carve_mum_learn(ws, M, R, T_, o.dtype);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    const T* X = static_cast<const T*>(X_);
    const T* mask = static_cast<const T*>(mask_);
    T* W = static_cast<T*>(W_);
    T* H = static_cast<T*>(H_);
    T *Am = reinterpret_cast<T*>(w.Am), *Ht = reinterpret_cast<T*>(w.Ht), *Vt = reinterpret_cast<T*>(w.Vt);
    T *Q1t = reinterpret_cast<T*>(w.Q1t), *Q2t = reinterpret_cast<T*>(w.Q2t), *part = reinterpret_cast<T*>(w.part);
    const long slab = (long)learn_bin_tiles(M) * 16 * d.Np;

    MumCtx<T> c;
    HIP_TRY(mum_begin<T>(c, X, ldx, mask, ldm, H, ldh, M, R, T_, nullptr, 1, o.layout, 1, w.solve_ws, w.solve_bytes, s));
    auto apply = [&](int update) -> int {
        hipLaunchKernelGGL(k_mum_dict_apply<T>, dim3(R), dim3(256), 0, s, (const T*)part, S, slab, d.Np, W, (long)ldw, fm ? 0 : 1, M,
                           update, w.astat);
        return (int)hipGetLastError();
    };
    auto step = [&]() -> int {
        HIP_TRY(mum_pack_dict<T>(c, W, ldw, s));
        HIP_TRY(mum_sweep<T>(c.a, o.loss, c.n_tiles, s));
        // frames-as-rows copies of the current factors (Ht is the right operand of the sums over the frames)
        HIP_TRY(copy2d<T>(W, ldw, M, R, fm ? 1 : 0, Am, d.Np, d.Mj, d.Np, 0, s));
        HIP_TRY(copy2d<T>(H, ldh, T_, R, fm ? 0 : 1, Ht, d.Np, d.Tp, d.Np, 0, s));
        HIP_TRY(gemm_nt<T>(Ht, d.Np, Am, d.Np, Vt, d.Mj, d.Tp, d.Mj, d.Np, s, nullptr, 0, nullptr, d.Mk));
        HIP_TRY(mum_dict_q<T>(o.loss, X, ldx, mask, ldm, fm ? 1 : 0, (const T*)Vt, Q1t, Q2t, d.Mj, M, T_, (long)d.Tp, s));
        HIP_TRY(dict_grad<T>(Q1t, d.Mj, Q2t, d.Mj, Ht, d.Np, M, T_, S, part, s));
        return apply(1);
    };
    // slot 0 has no statistic; slot c: max |D - D_new| of iteration c * check_every, read back from the device
    auto stat_now = [&](int slot, double* host) -> int {
        if (slot == 0) {
            *host = __builtin_nan("");
            return 0;
        }
        hipLaunchKernelGGL(k_mum_stat, dim3(1), dim3(256), 0, s, (const double*)w.astat, R, w.stat);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host, w.stat, sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return 0;
    };
    HIP_TRY(apply(0));                                               // nmf.solve normalises the start dictionary
    auto stop = [&](int, double stat, double, double) { return stat < o.tol; };
    return learn_loop(o.iters, o.check_every, o.tol, stat_out, n_iter_out, o.ev_loop_start, o.ev_loop_stop, s, step, stat_now,
                      stop);
}

}  // namespace

#define MUM_STEP_INSTANTIATE(T)                                                                                          \
    template int mum_sweep_prepare<T>();                                                                                 \
    template int mum_pack_dict<T>(const MumCtx<T>&, const T*, int, hipStream_t);                                         \
    template int mum_sweep<T>(const MumArgs<T>&, int, int, hipStream_t);                                                 \
    template int mum_dict_q<T>(int, const T*, int, const T*, int, int, const T*, T*, T*, int, int, int, long, hipStream_t);
MUM_STEP_INSTANTIATE(double)
MUM_STEP_INSTANTIATE(float)

}  // namespace evc

extern "C" {

size_t evc_mu_masked_workspace_bytes(int M, int N, int T, int n_utt, int dtype) {
    return evc::mum_workspace_bytes(M, N, T, n_utt, dtype);
}

int evc_mu_masked_solve(const void* A, int lda, const void* X, int ldx, const void* mask, int ldm, void* H, int ldh, int M,
                        int N, int T, const int* utt_offsets, int n_utt, const evc_mu_masked_opts* opts, void* workspace,
                        size_t workspace_bytes, int* n_iter_out, double* err_out, evc_stream_t stream) {
    using namespace evc;
    HIP_TRY(mum_args_check(A, lda, X, ldx, mask, ldm, H, ldh, M, N, T, utt_offsets, n_utt, opts, workspace, workspace_bytes));
    const evc_mu_masked_opts& o = *opts;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (o.dtype == EVC_F64)
        return mum_solve<double>(static_cast<const double*>(A), lda, static_cast<const double*>(X), ldx,
                                 static_cast<const double*>(mask), ldm, static_cast<double*>(H), ldh, M, N, T, utt_offsets, n_utt,
                                 o, workspace, workspace_bytes, n_iter_out, err_out, s);
    return mum_solve<float>(static_cast<const float*>(A), lda, static_cast<const float*>(X), ldx, static_cast<const float*>(mask),
                            ldm, static_cast<float*>(H), ldh, M, N, T, utt_offsets, n_utt, o, workspace, workspace_bytes,
                            n_iter_out, err_out, s);
}

size_t evc_mu_masked_learn_workspace_bytes(int M, int R, int T, int dtype) {
    return evc::mum_learn_workspace_bytes(M, R, T, dtype);
}

int evc_mu_masked_learn_splits(int M, int R, int T) {
    return evc::mum_learn_workspace_bytes(M, R, T, EVC_F64) ? evc::learn_splits(M, R, T) : 0;
}

int evc_mu_masked_learn(const void* X, int ldx, const void* mask, int ldm, void* W, int ldw, void* H, int ldh, int M, int R,
                        int T, const evc_mu_masked_learn_opts* opts, void* workspace, size_t workspace_bytes, int* n_iter_out,
                        double* stat_out, evc_stream_t stream) {
    using namespace evc;
    int forced;
    HIP_TRY(mum_learn_args_check(X, ldx, mask, ldm, W, ldw, H, ldh, M, R, T, opts, workspace, workspace_bytes, &forced));
    const evc_mu_masked_learn_opts& o = *opts;
    const int S = forced ? forced : learn_splits(M, R, T);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return (o.dtype == EVC_F64 ? mum_learn<double> : mum_learn<float>)(X, ldx, mask, ldm, W, ldw, H, ldh, M, R, T, o, S, workspace,
                                                                        workspace_bytes, n_iter_out, stat_out, s);
}

}  // extern "C"
