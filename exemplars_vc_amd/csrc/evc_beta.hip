// evc_beta.hip - evc_beta_solve: multiplicative updates of the activations under any beta-divergence with the dictionary
// fixed: scikit-learn's non_negative_factorization(..., update_H=False, solver='mu', beta_loss=beta) for beta_loss =
// 'itakura-saito' (0) or any float (_multiplicative_update_w, _nmf.py:526-631; _beta_divergence, :85-189).  DESIGN.md §5.10.
//
// Per iteration and frame, with EPS = 2^-23 (numpy's float32 epsilon, in both element types):
//   V  = A h;  Vd = V, below EPS -> EPS if beta < 1;  Vn = V, below EPS -> EPS if beta < 2
//   Q1 = x * Vn^(beta-2);  Q2 = Vd^(beta-1);  Num = A^T Q1;  Den = A^T Q2 + l1 + l2 h, 0 -> EPS
//   h <- h * (Num / Den)^gamma,  gamma = 1/(2-beta) if beta < 1, 1/(beta-1) if beta > 2, else 1
// beta = 1 and beta = 2 run the same generic statement (evc_nmf_solve special-cases them: not bit-compatible).
//
// k_beta_sweep<T>: one launch per iteration, a workgroup of four wavefronts owns a tile of 16 frames of ONE utterance
// (utterances start at a tile boundary) for the whole iteration; the dictionary is streamed from its two packed images.
//   phase 1  V = A H over all N on the matrix cores (16x16x4): the wavefronts split the exemplars (chunks of 16), every
//            wavefront passes over the bin tiles in groups of 8 and the four partial sums are added in wavefront order
//            into the LDS image V[bin][frame]
//   phase 2  V -> Q1 | Q2 in place (two images of round_up(M, 16) x 16 elements: 135 KB at M = 528 in float64)
//   phase 3  the wavefronts split the exemplar tiles of 16; a tile's Num and Den are one pass A_tile^T [Q1 | Q2] over the
//            bins, then H is updated in place in the caller's memory
// H is written once per iteration and read once in phase 3 and once per group of 8 bin tiles in phase 1 (twice in all up
// to M = 128, 3 times at M = 201, 6 at M = 513); V, Q1, Q2, Num and Den never leave the compute unit.  The k index of
// an MFMA is only a summation index: lane group g of chunk c takes the four consecutive elements 16 c + 4 g + s of its
// operand row, so that every global operand read is contiguous per lane; phase 3's dictionary image is stored with the
// bins of a chunk permuted (slot 4 g + s holds bin 16 c + 4 s + g) so that the LDS rows the four lane groups read in one
// step are consecutive (conflict-free at the unpadded row length of 16).
// A frame's arithmetic depends on no other frame: a batch gives bitwise the per-utterance results, and a NaN stays in
// its frame's column.  Exponents that are multiples of 1/2 are evaluated with products, sqrt and one division (the power
// first, then the reciprocal: beta = 0 forms Q1 = x * (1 / (V V)), not sklearn's x * (1 / V)^2); pow only serves the
// general float beta.
//
// k_beta_err<T> forms V the same way and leaves every frame's share of the divergence (float64); k_beta_check sums an
// utterance's shares in a fixed order, records sqrt(2 max(res, 0)) and applies sklearn's stop rule on the device
// (stop[u] = the iteration the utterance stopped at; the sweeps of a stopped utterance return at once).
//
// k_beta_sweep<T, true> is the change variant of the sweep: the same phases and the same stored h_new, plus every frame's
// shares of sum (h_new - h_old)^2 and sum h_new^2 in float64; k_beta_change_check sums an utterance's shares, records
// ||H_new - H_old|| / ||H_new|| and stops the utterance on the device once it is <= tol: MiniBatchNMF._solve_W, behind
// evc_online_transform and evc_online_learn_fresh (beta_sweep_change, beta_restart, beta_flush).
//
// The host steps (beta_begin, beta_pack_dict, beta_sweep, beta_check; evc_beta_common.h) also serve evc_beta_learn, which
// repacks the dictionary every iteration and sets BetaArgs.flush (an updated activation below it is stored as 0);
// evc_beta_solve passes 0 and its results are bitwise what they were without the field.  evc_online_learn hands its
// batches in as utterances and launches k_beta_sweep / k_beta_err over one batch's tiles (BetaArgs.tile0, 0 elsewhere).
#include "evc_beta_common.h"

namespace evc {

namespace {

// CHG: the change variant (evc_online_transform).  The same phases and the same stored h_new; phase 3 also forms, per frame
// of the tile, sum_n (h_new - h_old)^2 and sum_n h_new^2 in float64 in a fixed order - per lane its exemplar tiles in
// ascending order (rows r = 0..3 inside a tile), then the four lane groups of the frame by wave shuffles in the order 0, 1,
// 2, 3, then the four wavefronts through LDS in wavefront order - and writes them to chg[slot][0 | 1] (padding slots: 0).
template <typename T, bool CHG = false>
__global__ __launch_bounds__(BT_THREADS) void k_beta_sweep(BetaArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char beta_lds[];
    typedef typename Mma<T>::acc_t acc_t;
    typedef typename Vec4<T>::type vec_t;
    const int tile = a.tile0 + blockIdx.x;
    const int4 tl = a.tiles[tile];
    if (a.stop[tl.x] != 0) return;
    T* Q1 = reinterpret_cast<T*>(beta_lds);
    T* Q2 = Q1 + a.MP * BT_F;
    beta_form_v<T>(a, tl, Q1);
    // phase 2: V -> Q1 | Q2
    {
        const T* Xt = a.Xp + (long)tile * a.MP * BT_F;
        const T eps = (T)BETA_EPS;
        for (int e = threadIdx.x; e < a.MP * BT_F; e += BT_THREADS) {
            T q1 = T(0), q2 = T(0);
            if ((e >> 4) < a.M) {
                const T v = Q1[e];
                const T vn = (a.clamp_n && v < eps) ? eps : v;
                const T vd = (a.clamp_d && v < eps) ? eps : v;
                q1 = pw(vn, a.p1) * Xt[e];
                q2 = pw(vd, a.p2);
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
    const T eps = (T)BETA_EPS;
    double d2 = 0.0, n2 = 0.0;
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
                const T h = *hp;
                T d = den[r] + a.l1;
                d = d + a.l2 * h;
                d = d == T(0) ? eps : d;
                T q = num[r] / d;
                if (!a.gamma_one) q = pw(q, a.pg);
                T hn = h * q;
                if (a.flush > T(0) && hn < a.flush) hn = T(0);
                *hp = hn;
                if constexpr (CHG) {
                    const double dh = (double)hn - (double)h;
                    d2 += dh * dh;
                    n2 += (double)hn * (double)hn;
                }
            }
        }
    }
    if constexpr (CHG) {
        double* red = reinterpret_cast<double*>(beta_lds + (size_t)2 * a.MP * BT_F * sizeof(T));      // [4 waves][2][16 frames]
        const double s2 = ((__shfl(d2, f) + __shfl(d2, f + 16)) + __shfl(d2, f + 32)) + __shfl(d2, f + 48);
        const double q2 = ((__shfl(n2, f) + __shfl(n2, f + 16)) + __shfl(n2, f + 32)) + __shfl(n2, f + 48);
        if (lane < 16) {
            red[wave * 32 + f] = s2;
            red[wave * 32 + 16 + f] = q2;
        }
        __syncthreads();
        if (threadIdx.x < 32) {
            const int j = threadIdx.x & 15, k = threadIdx.x >> 4;
            const double v = ((red[k * 16 + j] + red[32 + k * 16 + j]) + red[64 + k * 16 + j]) + red[96 + k * 16 + j];
            a.chg[((long)tile * BT_F + j) * 2 + k] = j < tl.z ? v : 0.0;
        }
    }
}

// errf[slot] = the frame's share of _beta_divergence(X, H, A, beta): see the header comment of evc_beta_solve
template <typename T>
__global__ __launch_bounds__(BT_THREADS) void k_beta_err(BetaArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char beta_lds[];
    const int tile = a.tile0 + blockIdx.x;
    const int4 tl = a.tiles[tile];
    if (a.stop[tl.x] != 0) return;
    T* Vs = reinterpret_cast<T*>(beta_lds);
    double* red = reinterpret_cast<double*>(beta_lds + (size_t)a.MP * BT_F * sizeof(T));      // [3][16 parts][16 frames]
    beta_form_v<T>(a, tl, Vs);
    const T* Xt = a.Xp + (long)tile * a.MP * BT_F;
    const int f = threadIdx.x & 15, part = threadIdx.x >> 4;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int m = part; m < a.M; m += 16) {
        const double x = (double)Xt[m * BT_F + f], v = (double)Vs[m * BT_F + f];
        const double vv = v < BETA_EPS ? BETA_EPS : v;
        switch (a.err_mode) {
            case BETA_ERR_IS:
                if (x > BETA_EPS) {
                    const double d = x / vv;
                    s0 += d - log(d);
                }
                break;
            case BETA_ERR_KL:
                s0 += v;
                if (x > BETA_EPS) s0 += x * log(x / vv) - x;
                break;
            case BETA_ERR_FROB:
                s0 += (x - v) * (x - v);
                break;
            default:
                s2 += pw(v, a.pb);
                if (x > BETA_EPS) {
                    s0 += pw(x, a.pb);
                    s1 += x * pw(vv, a.p2);
                }
        }
    }
    red[part * 16 + f] = s0;
    red[256 + part * 16 + f] = s1;
    red[512 + part * 16 + f] = s2;
    __syncthreads();
    if (threadIdx.x < 16) {
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        for (int p = 0; p < 16; ++p) {
            t0 += red[p * 16 + f];
            t1 += red[256 + p * 16 + f];
            t2 += red[512 + p * 16 + f];
        }
        double res;
        if (a.err_mode == BETA_ERR_IS) res = t0 - (double)a.M;
        else if (a.err_mode == BETA_ERR_KL) res = t0;
        else if (a.err_mode == BETA_ERR_FROB) res = 0.5 * t0;
        else res = (t0 - a.beta * t1 + (a.beta - 1.0) * t2) / (a.beta * (a.beta - 1.0));
        a.errf[(long)tile * BT_F + f] = f < tl.z ? res : 0.0;
    }
}

// one block per utterance: err = sqrt(2 max(sum of the shares, 0)) in a fixed order; check c (0: the start)
__global__ __launch_bounds__(256) void k_beta_check(const double* __restrict__ errf, const int* __restrict__ utt_tile0,
                                                    int* stop, double* einit, double* eprev, double* trace, int n_slots,
                                                    int c, int check_every, int stop_rule, double tol) {
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
    const double err = sqrt(2.0 * fmax(red[0], 0.0));
    trace[(long)u * n_slots + c] = err;
    if (c == 0) {
        einit[u] = err;
        eprev[u] = err;
        return;
    }
    if (stop_rule == EVC_STOP_SKLEARN && (eprev[u] - err) / einit[u] < tol) stop[u] = c * check_every;
    else eprev[u] = err;
}

// one block per utterance: the shares of the change variant summed in index order (per thread strided, then a tree, as
// k_beta_check), ratio = sqrt(d2) / sqrt(n2) into trace slot it - 1, and the stop of MiniBatchNMF._solve_W: a NaN ratio (0 / 0
// among them) compares false and the utterance runs on, as in numpy
__global__ __launch_bounds__(256) void k_beta_change_check(const double* __restrict__ chg, const int* __restrict__ utt_tile0,
                                                           int utt0, int* stop, double* trace, int n_slots, int it,
                                                           double tol) {
    __shared__ double red[2][256];
    const int u = utt0 + blockIdx.x;
    const long i0 = (long)utt_tile0[u] * BT_F, i1 = (long)utt_tile0[u + 1] * BT_F;
    if (stop[u] != 0 || i0 == i1) return;       // uniform per block
    const double2* __restrict__ pair = reinterpret_cast<const double2*>(chg);
    double d2 = 0.0, n2 = 0.0;
    // eight loads in flight per thread, added in index order: a long utterance is one workgroup's latency-bound sum
#pragma unroll 8
    for (long i = i0 + threadIdx.x; i < i1; i += 256) {
        const double2 v = pair[i];
        d2 += v.x;
        n2 += v.y;
    }
    red[0][threadIdx.x] = d2;
    red[1][threadIdx.x] = n2;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double ratio = sqrt(red[0][0]) / sqrt(red[1][0]);
    trace[(long)u * n_slots + it - 1] = ratio;
    if (tol > 0.0 && ratio <= tol) stop[u] = it;
}

// the stop words of utterances [u0, u0 + n) back to "running" (evc_online_learn_fresh revisits its batches every pass)
__global__ void k_beta_stop_reset(int* stop, int u0, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) stop[u0 + i] = 0;
}

__global__ void k_beta_state_init(int* stop, double* trace, int n_utt, int n_slots) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_utt) stop[i] = 0;
    if (i < (long)n_utt * n_slots) trace[i] = __builtin_nan("");
}

template <typename T>
__global__ void k_beta_pack_dict(const T* __restrict__ A, int lda, int fm, int M, int N, int NP, int MP,
                                 T* __restrict__ Ap1, T* __restrict__ Ap3) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)NP * MP) return;
    const int n = (int)(i / MP), p = (int)(i % MP);
    const int m3 = (p & ~15) + (p & 3) * 4 + ((p >> 2) & 3);       // slot 4 g + s holds bin 4 s + g of its chunk
    T v1 = T(0), v3 = T(0);
    if (n < N) {
        if (p < M) v1 = fm ? A[(long)n * lda + p] : A[(long)p * lda + n];
        if (m3 < M) v3 = fm ? A[(long)n * lda + m3] : A[(long)m3 * lda + n];
    }
    Ap1[i] = v1;
    Ap3[i] = v3;
}

template <typename T>
__global__ void k_beta_pack_x(const T* __restrict__ X, int ldx, int fm, int M, int MP, const int4* __restrict__ tiles,
                              int n_tiles, T* __restrict__ Xp) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n_tiles * MP * BT_F) return;
    const int4 tl = tiles[i / ((long)MP * BT_F)];
    const int m = (int)((i / BT_F) % MP), f = (int)(i % BT_F);
    T v = T(0);
    if (m < M && f < tl.z) v = fm ? X[(long)(tl.y + f) * ldx + m] : X[(long)m * ldx + tl.y + f];
    Xp[i] = v;
}

// h0[u] = sqrt(mean(X_u) / N) (sklearn's start, _nmf.py:1228-1231), summed in a fixed order over the packed frames
template <typename T>
__global__ __launch_bounds__(256) void k_beta_h0(const T* __restrict__ Xp, const int* __restrict__ utt_tile0,
                                                 const int* __restrict__ utt_frames, int M, int MP, int N,
                                                 double* __restrict__ h0) {
    __shared__ double red[256];
    const int u = blockIdx.x;
    const long i0 = (long)utt_tile0[u] * MP * BT_F, i1 = (long)utt_tile0[u + 1] * MP * BT_F;
    double acc = 0.0;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) acc += (double)Xp[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double cnt = (double)utt_frames[u] * (double)M;
        h0[u] = cnt > 0.0 ? sqrt(red[0] / cnt / (double)N) : 0.0;
    }
}

// every activation of utterance u starts at h0[u] (h0 == NULL: at `value`)
template <typename T>
__global__ void k_beta_fill(T* __restrict__ H, long hs_t, long hs_n, int N, const int4* __restrict__ tiles, int n_tiles,
                            const double* __restrict__ h0, double value) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n_tiles * BT_F * N) return;
    const long slot = i / N;
    const int n = (int)(i % N), f = (int)(slot % BT_F);
    const int4 tl = tiles[slot / BT_F];
    if (f < tl.z) H[(long)(tl.y + f) * hs_t + (long)n * hs_n] = (T)(h0 ? h0[tl.x] : value);
}

// H < thr -> 0 over the columns of n_tiles tiles: a pass of its own AFTER a solve (MiniBatchNMF._minibatch_step, beta < 1);
// BetaArgs.flush during the solve's sweeps would pin an entry at 0 that the next update could still have raised
template <typename T>
__global__ void k_beta_flush(T* __restrict__ H, long hs_t, long hs_n, int N, const int4* __restrict__ tiles, int n_tiles,
                             T thr) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)n_tiles * BT_F * N) return;
    const long slot = i / N;
    const int n = (int)(i % N), f = (int)(slot % BT_F);
    const int4 tl = tiles[slot / BT_F];
    if (f < tl.z) {
        T* hp = H + (long)(tl.y + f) * hs_t + (long)n * hs_n;
        if (*hp < thr) *hp = T(0);
    }
}

unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

// [Ap1 | Ap3 | Xp | errf | tiles | utt_tile0 | utt_frames | stop | h0 | einit | eprev | trace], each 256-byte aligned
// (ws == NULL: sizes only)
template <typename T>
BetaWs<T> carve_beta(void* ws, int M, int N, int T_, int n_utt) {
    BetaWs<T> w;
    Carver c = Carver::rounded(ws);
    const size_t MP = (size_t)round_up(M, 16), NP = (size_t)round_up(N, 16);
    const size_t nt = (size_t)frame_tile_cap(T_, BT_F, n_utt);
    w.Ap1 = c.take<T>(NP * MP);
    w.Ap3 = c.take<T>(NP * MP);
    w.Xp = c.take<T>(nt * MP * BT_F);
    w.errf = c.take<double>(nt * BT_F);
    w.tiles = c.take<int4>(nt);
    w.utt_tile0 = c.take<int>((size_t)n_utt + 1);
    w.utt_frames = c.take<int>(n_utt);
    w.stop = c.take<int>(n_utt);
    w.h0 = c.take<double>(n_utt);
    w.einit = c.take<double>(n_utt);
    w.eprev = c.take<double>(n_utt);
    w.trace = c.take<double>((size_t)n_utt * BETA_MAX_SLOTS);
    w.bytes = c.bytes();
    return w;
}

}  // namespace

size_t beta_workspace_bytes(int M, int N, int T_, int n_utt, int dtype) {
    if (M < 1 || M > BETA_MAX_M || N < 1 || T_ < 0 || n_utt < 1) return 0;
    if (dtype == EVC_F64) return carve_beta<double>(nullptr, M, N, T_, n_utt).bytes + 256;
    if (dtype == EVC_F32) return carve_beta<float>(nullptr, M, N, T_, n_utt).bytes + 256;
    return 0;
}

template <typename T>
int beta_begin(BetaCtx<T>& c, const T* X, int ldx, T* H, int ldh, int M, int N, int T_, const int* utt_offsets, int n_utt,
               int layout, double beta, double l1, double l2, double flush, int n_slots, void* ws, size_t ws_bytes,
               hipStream_t s) {
    c.w = carve_beta<T>(ws, M, N, T_, n_utt);
    const BetaWs<T>& w = c.w;
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const bool fm = layout == EVC_FRAME_MAJOR;
    const int MP = round_up(M, 16), NP = round_up(N, 16);
    c.n_utt = n_utt;
    c.utt0 = 0;
    c.n_slots = n_slots;
    c.fm = fm ? 1 : 0;

    int n_tiles;
    HIP_TRY(frame_tiles_stage(BT_F, utt_offsets, n_utt, T_, w.tiles, w.utt_tile0, w.utt_frames, s, &n_tiles));
    c.n_tiles = n_tiles;
    hipLaunchKernelGGL(k_beta_state_init, dim3(blocks_of((long)n_utt * n_slots)), dim3(256), 0, s, w.stop, w.trace, n_utt,
                       n_slots);
    HIP_TRY(hipGetLastError());

    BetaArgs<T>& a = c.a;
    a.Ap1 = w.Ap1; a.Ap3 = w.Ap3; a.Xp = w.Xp; a.H = H;
    a.hs_t = fm ? ldh : 1; a.hs_n = fm ? 1 : ldh;
    a.tiles = w.tiles; a.stop = w.stop; a.errf = w.errf;
    a.M = M; a.MP = MP; a.N = N; a.NP = NP;
    a.beta = beta;
    a.clamp_n = beta - 2.0 < 0 ? 1 : 0;
    a.clamp_d = beta - 1.0 < 0 ? 1 : 0;
    const double gamma = beta_gamma(beta);
    a.gamma_one = gamma == 1.0 ? 1 : 0;
    a.p1 = pow_spec(beta - 2.0); a.p2 = pow_spec(beta - 1.0); a.pg = pow_spec(gamma); a.pb = pow_spec(beta);
    a.err_mode = beta == 0.0 ? BETA_ERR_IS : beta == 1.0 ? BETA_ERR_KL : beta == 2.0 ? BETA_ERR_FROB : BETA_ERR_GENERIC;
    a.l1 = (T)l1; a.l2 = (T)l2;
    a.flush = (T)flush;
    a.tile0 = 0;
    a.chg = nullptr;
    if (n_tiles > 0) {
        hipLaunchKernelGGL(k_beta_pack_x<T>, dim3(blocks_of((long)n_tiles * MP * BT_F)), dim3(256), 0, s, X, ldx, fm ? 1 : 0, M,
                           MP, w.tiles, n_tiles, w.Xp);
        HIP_TRY(hipGetLastError());
        // the attribute is per function and process-wide: always the limit of BETA_MAX_M, so that concurrent calls at
        // different M never shrink it under one another
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_beta_sweep<T>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)(2 * BETA_MAX_M * BT_F * sizeof(T))));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_beta_sweep<T, true>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(2 * BETA_MAX_M * BT_F * sizeof(T) + BETA_CHG_LDS)));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_beta_err<T>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(BETA_MAX_M * BT_F * sizeof(T) + 3 * 256 * sizeof(double))));
    }
    return 0;
}

template <typename T> int beta_pack_dict(const BetaCtx<T>& c, const T* A, int lda, hipStream_t s) {
    if (c.n_tiles == 0) return 0;
    const BetaArgs<T>& a = c.a;
    hipLaunchKernelGGL(k_beta_pack_dict<T>, dim3(blocks_of((long)a.NP * a.MP)), dim3(256), 0, s, A, lda, c.fm,
                       a.M, a.N, a.NP, a.MP, c.w.Ap1, c.w.Ap3);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T> int beta_sweep(const BetaCtx<T>& c, hipStream_t s) {
    if (c.n_tiles == 0) return 0;
    hipLaunchKernelGGL(k_beta_sweep<T>, dim3(c.n_tiles), dim3(BT_THREADS), (size_t)2 * c.a.MP * BT_F * sizeof(T), s, c.a);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T> int beta_sweep_change(const BetaCtx<T>& c, int it, double tol, hipStream_t s) {
    if (c.n_tiles == 0) return 0;
    hipLaunchKernelGGL((k_beta_sweep<T, true>), dim3(c.n_tiles), dim3(BT_THREADS),
                       (size_t)2 * c.a.MP * BT_F * sizeof(T) + BETA_CHG_LDS, s, c.a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_beta_change_check, dim3(c.n_utt), dim3(256), 0, s, c.a.chg, c.w.utt_tile0, c.utt0, c.w.stop,
                       c.w.trace, c.n_slots, it, tol);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T> int beta_restart(const BetaCtx<T>& c, bool fill, hipStream_t s) {
    if (c.n_tiles == 0) return 0;
    hipLaunchKernelGGL(k_beta_stop_reset, dim3(blocks_of(c.n_utt)), dim3(256), 0, s, c.w.stop, c.utt0, c.n_utt);
    HIP_TRY(hipGetLastError());
    if (!fill) return 0;
    hipLaunchKernelGGL(k_beta_fill<T>, dim3(blocks_of((long)c.n_tiles * BT_F * c.a.N)), dim3(256), 0, s, c.a.H, c.a.hs_t,
                       c.a.hs_n, c.a.N, c.w.tiles + c.a.tile0, c.n_tiles, c.w.h0, 0.0);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T> int beta_h0(const BetaCtx<T>& c, hipStream_t s) {
    if (c.n_tiles == 0) return 0;
    hipLaunchKernelGGL(k_beta_h0<T>, dim3(c.n_utt), dim3(256), 0, s, c.w.Xp, c.w.utt_tile0, c.w.utt_frames, c.a.M, c.a.MP,
                       c.a.N, c.w.h0);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T> int beta_flush(const BetaCtx<T>& c, double thr, hipStream_t s) {
    if (c.n_tiles == 0) return 0;
    hipLaunchKernelGGL(k_beta_flush<T>, dim3(blocks_of((long)c.n_tiles * BT_F * c.a.N)), dim3(256), 0, s, c.a.H, c.a.hs_t,
                       c.a.hs_n, c.a.N, c.w.tiles + c.a.tile0, c.n_tiles, (T)thr);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T> int beta_start(const BetaCtx<T>& c, int init_mode, double init_value, hipStream_t s) {
    if (c.n_tiles == 0 || init_mode == EVC_INIT_GIVEN) return 0;
    const BetaWs<T>& w = c.w;
    const bool sk = init_mode == EVC_INIT_SKLEARN;
    if (sk) HIP_TRY(beta_h0<T>(c, s));
    hipLaunchKernelGGL(k_beta_fill<T>, dim3(blocks_of((long)c.n_tiles * BT_F * c.a.N)), dim3(256), 0, s, c.a.H, c.a.hs_t,
                       c.a.hs_n, c.a.N, w.tiles, c.n_tiles, sk ? w.h0 : nullptr, init_value);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T> int beta_err(const BetaCtx<T>& c, hipStream_t s) {
    if (c.n_tiles == 0) return 0;
    const size_t lds_err = (size_t)c.a.MP * BT_F * sizeof(T) + 3 * 256 * sizeof(double);
    hipLaunchKernelGGL(k_beta_err<T>, dim3(c.n_tiles), dim3(BT_THREADS), lds_err, s, c.a);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int beta_check(const BetaCtx<T>& c, int chk, int check_every, int stop_rule, double tol, hipStream_t s) {
    if (c.n_tiles == 0) return 0;
    HIP_TRY(beta_err<T>(c, s));
    hipLaunchKernelGGL(k_beta_check, dim3(c.n_utt), dim3(256), 0, s, c.w.errf, c.w.utt_tile0, c.w.stop, c.w.einit, c.w.eprev,
                       c.w.trace, c.n_slots, chk, check_every, stop_rule, tol);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename T>
int beta_report(const BetaCtx<T>& c, int iters, int* n_iter_out, double* trace_out, int slots, hipStream_t s) {
    if (!n_iter_out && !trace_out) return 0;
    int* ni_h = static_cast<int*>(malloc(sizeof(int) * c.n_utt));
    if (!ni_h) return (int)hipErrorOutOfMemory;
    hipError_t e = hipMemcpyAsync(ni_h, c.w.stop, sizeof(int) * c.n_utt, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && trace_out && slots > 0)
        e = hipMemcpyAsync(trace_out, c.w.trace, sizeof(double) * c.n_utt * slots, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    for (int u = 0; e == hipSuccess && n_iter_out && u < c.n_utt; ++u) n_iter_out[u] = ni_h[u] ? ni_h[u] : iters;
    free(ni_h);
    HIP_TRY(e);
    return 0;
}

#define BETA_INSTANTIATE(T)                                                                                              \
    template int beta_begin<T>(BetaCtx<T>&, const T*, int, T*, int, int, int, int, const int*, int, int, double, double, \
                               double, double, int, void*, size_t, hipStream_t);                                        \
    template int beta_pack_dict<T>(const BetaCtx<T>&, const T*, int, hipStream_t);                                       \
    template int beta_sweep<T>(const BetaCtx<T>&, hipStream_t);                                                          \
    template int beta_err<T>(const BetaCtx<T>&, hipStream_t);                                                            \
    template int beta_start<T>(const BetaCtx<T>&, int, double, hipStream_t);                                            \
    template int beta_sweep_change<T>(const BetaCtx<T>&, int, double, hipStream_t);                                     \
    template int beta_h0<T>(const BetaCtx<T>&, hipStream_t);                                                             \
    template int beta_restart<T>(const BetaCtx<T>&, bool, hipStream_t);                                                      \
    template int beta_flush<T>(const BetaCtx<T>&, double, hipStream_t);                                                  \
    template int beta_check<T>(const BetaCtx<T>&, int, int, int, double, hipStream_t);                                  \
    template int beta_report<T>(const BetaCtx<T>&, int, int*, double*, int, hipStream_t);
BETA_INSTANTIATE(double)
BETA_INSTANTIATE(float)

namespace {

// arguments already validated by evc_beta_solve; returns 0, -2 or a hipError_t
template <typename T>
int beta_solve(const T* A, int lda, const T* X, int ldx, T* H, int ldh, int M, int N, int T_, const int* utt_offsets,
               int n_utt, const evc_beta_opts& o, void* ws, size_t ws_bytes, int* n_iter_out, double* err_out,
               hipStream_t s) {
    const int n_slots = 1 + (o.check_every > 0 ? o.iters / o.check_every : 0);
    BetaCtx<T> c;
    int st = beta_begin<T>(c, X, ldx, H, ldh, M, N, T_, utt_offsets, n_utt, o.layout, o.beta, o.l1, o.l2, 0.0, n_slots, ws,
                           ws_bytes, s);
    if (st != 0) return st;
    if ((st = beta_pack_dict<T>(c, A, lda, s)) != 0) return st;
    const int n_tiles = c.n_tiles;
    if ((st = beta_start<T>(c, o.init_mode, o.init_value, s)) != 0) return st;
    const bool checks = o.check_every > 0;
    if (checks && (st = beta_check<T>(c, 0, o.check_every, o.stop_rule, o.tol, s)) != 0) return st;
    if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
    for (int it = 1; n_tiles > 0 && it <= o.iters; ++it) {
        if ((st = beta_sweep<T>(c, s)) != 0) return st;
        if (checks && it % o.check_every == 0 && (st = beta_check<T>(c, it / o.check_every, o.check_every, o.stop_rule, o.tol, s)) != 0)
            return st;
    }
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    return beta_report<T>(c, o.iters, n_iter_out, err_out, n_slots, s);
}

}  // namespace

}  // namespace evc

extern "C" {

size_t evc_beta_workspace_bytes(int M, int N, int T, int n_utt, int dtype) {
    return evc::beta_workspace_bytes(M, N, T, n_utt, dtype);
}

int evc_beta_solve(const void* A, int lda, const void* X, int ldx, void* H, int ldh, int M, int N, int T,
                   const int* utt_offsets, int n_utt, const evc_beta_opts* opts, void* workspace, size_t workspace_bytes,
                   int* n_iter_out, double* err_out, evc_stream_t stream) {
    using namespace evc;
    if (!opts || opts->struct_bytes != (int)sizeof(evc_beta_opts)) return ST_BADARG;
    const evc_beta_opts& o = *opts;
    HIP_TRY(solve_args_ok(M, N, T, n_utt, o.dtype, o.layout, A, workspace, lda, ldx, ldh, utt_offsets));
    if (o.iters < 0 || o.check_every < 0 || o.reserved != 0) return ST_BADARG;
    if (o.init_mode != EVC_INIT_GIVEN && o.init_mode != EVC_INIT_SKLEARN && o.init_mode != EVC_INIT_CONST) return ST_BADARG;
    if (o.stop_rule != EVC_STOP_NONE && o.stop_rule != EVC_STOP_SKLEARN) return ST_BADARG;
    if (!(o.beta - o.beta == 0.0)) return ST_BADARG;                      // NaN or infinite
    if (!(o.tol >= 0.0) || !(o.l1 >= 0.0) || !(o.l2 >= 0.0) || !(o.init_value - o.init_value == 0.0)) return ST_BADARG;
    if (T > 0 && (!X || !H)) return ST_BADARG;                             // no frames: X and H are never touched
    if (o.check_every > 0 && o.iters / o.check_every + 1 > BETA_MAX_SLOTS) return ST_BADARG;
    if (M > BETA_MAX_M) return ST_UNSUPPORTED;
    if (workspace_bytes < beta_workspace_bytes(M, N, T, n_utt, o.dtype)) return ST_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (o.dtype == EVC_F64)
        return beta_solve<double>(static_cast<const double*>(A), lda, static_cast<const double*>(X), ldx,
                                  static_cast<double*>(H), ldh, M, N, T, utt_offsets, n_utt, o, workspace, workspace_bytes,
                                  n_iter_out, err_out, s);
    return beta_solve<float>(static_cast<const float*>(A), lda, static_cast<const float*>(X), ldx, static_cast<float*>(H),
                             ldh, M, N, T, utt_offsets, n_utt, o, workspace, workspace_bytes, n_iter_out, err_out, s);
}

}  // extern "C"
