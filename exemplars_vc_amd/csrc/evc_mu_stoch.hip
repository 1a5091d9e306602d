// evc_mu_stoch.hip - evc_mu_stoch_learn: deComP's mini-batch NMF, nmf.solve(minibatch=bs, method='asg-mu' | 'gsg-mu' |
// 'asag-mu' | 'gsag-mu' | 'svrmu' | 'svrmu-acc') (decomp/nmf.py, nmf_methods/serizel.py, nmf_methods/kasai.py), mirrored and
// not corrected.  DESIGN.md §5.23; the arithmetic is stated in include/evc.h.
//
// A step is tiny (M R bs elements), so it is a short chain of launches and nothing else; the host never waits inside an epoch:
//   k_mus_gather     X, mask and H read THROUGH the epoch's order row: the batch as k_mum_sweep's tile images (mask . X | mask),
//                    as frames-as-rows copies Xt | Mt for the dictionary half, and H_F as a contiguous frames-as-rows buffer
//   k_mum_sweep      evc_mu_masked_solve's kernel, unchanged, with the batch as one utterance and H_F as its activations (W's
//                    two packed images are rebuilt before it, as evc_mu_masked_learn does)
//   k_mus_scatter    H_F back to the caller's H
//   k_mus_dict_grad  the fused, masked dictionary gradient, k_beta_dict_grad's geometry (evc_beta_learn.hip): a workgroup owns
//                    one 16-bin tile x BDG_RB component tiles x one of S frame ranges of the batch; W's tile rows sit in LDS
//                    with the bank-shifting row length; per 16 frames a wavefront forms V^T = H_F^T W^T on the matrix cores,
//                    turns the accumulator into Q1 | Q2 (mask and loss) in registers and feeds both back as the left operands
//                    of the g+ | g- MFMAs.  The four wavefronts take a quarter of the range each and are added through LDS in
//                    wavefront order.  V, Q1, Q2 never reach memory.  R <= 256; beyond, and on the unfused route,
//                    evc_mu_masked_learn's kernels (copy2d, gemm_nt, k_mum_dict_q, k_dict_grad) form the same slabs.
//   k_mus_apply      one workgroup per atom: the slabs summed in the order 0 .. S-1, the method's combination (a+-, or prev+- and
//                    full+-), the CANDIDATE atom normalised, the atom's share of max |W - W_new|.  svrmu's prev+-[b] <- g+- is
//                    written here, by the thread that has just read its element: nothing reads it again before the commit.
//   k_mus_commit     the maximum of the shares in a fixed order (a NaN passes) into the trace; stat < tol sets the stop word
//                    and leaves W, else the candidate becomes W.  Every workgroup recomputes the maximum and copies 16 atoms.
// Every kernel here returns at once when the stop word is set, k_mum_sweep through MumArgs::stop.  No float atomics, no
// exchange between workgroups inside a launch, no residency assumption: the same call gives the same bits every time.
#include "evc_mu_masked_common.h"
#include "evc_mu_stoch_plan.h"

// deComP's products and sums stay products and sums (the statement in include/evc.h: "none contracted")
#pragma clang fp contract(off)

namespace evc {

static_assert(MUS_FUSED_MAX_R == BDG_MAX_R && MUS_ROUTE_R <= MUS_FUSED_MAX_R, "evc_mu_stoch_plan.h restates evc_beta_common.h");

namespace {

constexpr int MDG_LD = 20;            // LDS row length of W's tile image: 4 x 20 elements shift the four lane groups by 16 banks
constexpr int MDG_RB = 2;             // component tiles of 16 per workgroup of k_mus_dict_grad
constexpr int MDG_WAVES = 4;          // wavefronts per workgroup: each takes a quarter of the frame range
constexpr int MSA_PER = (MUM_MAX_M + 255) / 256;      // bins per thread of k_mus_apply
constexpr int MSC_ATOMS = 16;         // atoms a workgroup of k_mus_commit copies
enum { MUS_NORM = 0, MUS_ACC = 1, MUS_UPDATE = 2 };

template <typename T> struct MusGatherArgs {
    const T* X; const T* mask; T* H;
    int ldx, ldm, fm;
    long hs_t, hs_n;        // H(n, t) = H[t * hs_t + n * hs_n]
    const int* ord;         // the epoch's order row (NULL: the frames as they lie)
    int t0, bs;             // the step's frames are ord[t0 .. t0 + bs)
    int M, MP, Mk, R, Np, n_tiles;
    T *XMp, *Mp;            // [n_tiles][MP][16]
    T *Xt, *Mt;             // [>= bs][Mk] (Mt NULL without a mask)
    T* HF;                  // [>= bs][Np]
    const int* stop;
};

// the three images of the batch; zero in every padding that is read
template <typename T> __global__ __launch_bounds__(256) void k_mus_gather(MusGatherArgs<T> a) {
    if (*a.stop != 0) return;
    const long nA = (long)a.n_tiles * a.MP * BT_F, nB = (long)a.bs * a.Mk, nC = (long)a.bs * a.R;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < nA) {
        const int m = (int)((i / BT_F) % a.MP), f = (int)(i / ((long)a.MP * BT_F)) * BT_F + (int)(i % BT_F);
        T w = T(0), xm = T(0);
        if (m < a.M && f < a.bs) {
            const long fr = a.ord ? a.ord[a.t0 + f] : a.t0 + f;
            const T x = a.fm ? a.X[fr * a.ldx + m] : a.X[(long)m * a.ldx + fr];
            w = !a.mask ? T(1) : a.fm ? a.mask[fr * a.ldm + m] : a.mask[(long)m * a.ldm + fr];
            xm = x * w;
        }
        a.XMp[i] = xm;
        a.Mp[i] = w;
        return;
    }
    i -= nA;
    if (i < nB) {
        const int f = (int)(i / a.Mk), m = (int)(i % a.Mk);
        const long fr = a.ord ? a.ord[a.t0 + f] : a.t0 + f;
        T x = T(0), w = T(0);
        if (m < a.M) {
            x = a.fm ? a.X[fr * a.ldx + m] : a.X[(long)m * a.ldx + fr];
            if (a.mask) w = a.fm ? a.mask[fr * a.ldm + m] : a.mask[(long)m * a.ldm + fr];
        }
        a.Xt[i] = x;
        if (a.Mt) a.Mt[i] = w;
        return;
    }
    i -= nB;
    if (i < nC) {
        const int f = (int)(i / a.R), n = (int)(i % a.R);
        const long fr = a.ord ? a.ord[a.t0 + f] : a.t0 + f;
        a.HF[(long)f * a.Np + n] = a.H[fr * a.hs_t + n * a.hs_n];
    }
}

// H(:, F) <- H_F
template <typename T> __global__ __launch_bounds__(256) void k_mus_scatter(MusGatherArgs<T> a) {
    if (*a.stop != 0) return;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)a.bs * a.R) return;
    const int f = (int)(i / a.R), n = (int)(i % a.R);
    const long fr = a.ord ? a.ord[a.t0 + f] : a.t0 + f;
    a.H[fr * a.hs_t + n * a.hs_n] = a.HF[(long)f * a.Np + n];
}

template <typename T> struct MusDictArgs {
    const T* Xt;            // [>= T_][ldx] the batch's frames as rows, zero from M on
    const T* Mt;            // the mask likewise, or NULL (1)
    const T* Ht;            // [>= T_][ldh] H_F, frames as rows, zero from R on, ldh a multiple of 128
    const T* W;             // the caller's dictionary: W(m, k) = W[m * ws_m + k * ws_r]
    long ws_m, ws_r;
    T* part;                // [S][2][MTp * 16][ldh]
    int ldx, ldh;
    int M, R, RP16, MTp, T_, S;
    const int* stop;
};

// grid (component groups of MDG_RB tiles, bin tiles, frame ranges); the four wavefronts split the frame range
template <typename T, int LOSS>
__global__ __launch_bounds__(64 * MDG_WAVES) void k_mus_dict_grad(MusDictArgs<T> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mdg_lds[];
    typedef typename Mma<T>::acc_t acc_t;
    typedef typename Vec4<T>::type vec_t;
    if (*a.stop != 0) return;
    T* Ws = reinterpret_cast<T*>(mdg_lds);         // [RP16][MDG_LD]: Ws[k][b] = W[bin b of the tile][component k]
    T* red = Ws + a.RP16 * MDG_LD;                 // [MDG_WAVES - 1][2 MDG_RB x 4][64]: the other wavefronts' partial sums
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b16 = lane & 15, g = lane >> 4;
    const int r0 = blockIdx.x * MDG_RB * 16;
    const int m0 = blockIdx.y * 16;
    const int sp = blockIdx.z;
    const int rb = (int)((long)sp * a.T_ / a.S), re = (int)((long)(sp + 1) * a.T_ / a.S);
    // this wavefront's quarter of the range (short ranges leave some wavefronts without frames)
    const int tb = rb + (int)((long)(re - rb) * wave / MDG_WAVES), te = rb + (int)((long)(re - rb) * (wave + 1) / MDG_WAVES);
    for (int e = threadIdx.x; e < a.RP16 * 16; e += 64 * MDG_WAVES) {
        const int k = e % a.RP16, m = m0 + e / a.RP16;
        const T v = a.W[(long)(m < a.M ? m : a.M - 1) * a.ws_m + (long)(k < a.R ? k : a.R - 1) * a.ws_r];
        Ws[k * MDG_LD + e / a.RP16] = (m < a.M && k < a.R) ? v : T(0);
    }
    __syncthreads();
    const int moff = m0 + b16;
    const bool mlive = moff < a.M;
    acc_t num[MDG_RB], den[MDG_RB];
#pragma unroll
    for (int j = 0; j < MDG_RB; ++j) num[j] = den[j] = acc_t{0, 0, 0, 0};
    const int hoff = r0 + b16;
    const int NC = a.RP16 / 16;
    const T jit = (T)MUM_J;
#pragma unroll 1
    for (int t0 = tb; t0 < te; t0 += 16) {
        // the frame this lane supplies to V's MFMAs (left operand row b16) and the four its accumulator registers hold;
        // a ragged range: clamped addresses, then a select
        const bool vlive = t0 + b16 < te;
        const T* __restrict__ hv_row = a.Ht + (long)(vlive ? t0 + b16 : te - 1) * a.ldh + 4 * g;
        bool live[4];
        T hb[4][MDG_RB], x[4], wgt[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int fr = t0 + Mma<T>::row(lane, r);
            live[r] = fr < te;
            const long frow = live[r] ? fr : te - 1;
#pragma unroll
            for (int j = 0; j < MDG_RB; ++j) {
                const T h = a.Ht[frow * a.ldh + hoff + 16 * j];
                hb[r][j] = live[r] ? h : T(0);
            }
            x[r] = a.Xt[frow * a.ldx + moff];
            wgt[r] = a.Mt ? a.Mt[frow * a.ldx + moff] : T(1);
        }
        acc_t v = acc_t{0, 0, 0, 0};
#pragma unroll 1
        for (int c = 0; c < NC; ++c) {
            vec_t hv = *reinterpret_cast<const vec_t*>(hv_row + 16 * c);
            const T* __restrict__ wr = Ws + (16 * c + 4 * g) * MDG_LD + b16;
#pragma unroll
            for (int s = 0; s < 4; ++s) v = Mma<T>::mma(vlive ? hv[s] : T(0), wr[s * MDG_LD], v);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool on = live[r] && mlive;
            const T xw = x[r] * wgt[r];
            T q1, q2;
            if (LOSS == EVC_LOSS_KL) {
                q1 = xw / (v[r] + jit);
                q2 = wgt[r];
            } else {
                q1 = xw;
                q2 = wgt[r] * v[r];
            }
            q1 = on ? q1 : T(0);
            q2 = on ? q2 : T(0);
#pragma unroll
            for (int j = 0; j < MDG_RB; ++j) {
                num[j] = Mma<T>::mma(q1, hb[r][j], num[j]);
                den[j] = Mma<T>::mma(q2, hb[r][j], den[j]);
            }
        }
    }
    // the four quarters, added in wavefront order
    if (wave > 0) {
        T* mine = red + (wave - 1) * (2 * MDG_RB * 4 * 64) + lane;
#pragma unroll
        for (int j = 0; j < MDG_RB; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                mine[(j * 8 + r) * 64] = num[j][r];
                mine[(j * 8 + 4 + r) * 64] = den[j][r];
            }
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll 1
    for (int w = 1; w < MDG_WAVES; ++w) {
        const T* theirs = red + (w - 1) * (2 * MDG_RB * 4 * 64) + lane;
#pragma unroll
        for (int j = 0; j < MDG_RB; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                num[j][r] += theirs[(j * 8 + r) * 64];
                den[j][r] += theirs[(j * 8 + 4 + r) * 64];
            }
    }
    const long slab = (long)a.MTp * 16 * a.ldh;
    T* __restrict__ out = a.part + (long)sp * 2 * slab;
#pragma unroll
    for (int j = 0; j < MDG_RB; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long o = (long)(m0 + Mma<T>::row(lane, r)) * a.ldh + hoff + 16 * j;
            out[o] = num[j][r];
            out[slab + o] = den[j][r];
        }
}

template <typename T> size_t mdg_lds_bytes(int RP16) {
    return ((size_t)RP16 * MDG_LD + (size_t)(MDG_WAVES - 1) * 2 * MDG_RB * 4 * 64) * sizeof(T);
}

template <typename T> struct MusApplyArgs {
    const T* part;          // [S][2][slab], element (m, r) at m * ldp + r
    long slab;
    int S, ldp;
    const T* W;             // W(m, r) = W[m * ws_m + r * ws_r]
    long ws_m, ws_r;
    T* dst;                 // the normalised atom: the candidate [R][M], or (MUS_NORM) W itself
    long ds_m, ds_r;
    T* acc;                 // [2][R][M]: a+- | full+-
    T* prev;                // [2][R][M]: svrmu's prev+-[b]
    double* astat;          // [R]
    const int* stop;
    int M, R, mode, first, last;
    T omr, rho;             // (1 - rho) and rho; svrmu: (1 - alpha) and alpha
    T n_loop;
};

// One workgroup per atom r; the reductions as k_mum_dict_apply's (evc_mu_masked.hip): the squares summed per thread over its
// bins in ascending order, then a tree over the threads.
template <typename T, int METHOD> __global__ __launch_bounds__(256) void k_mus_apply(MusApplyArgs<T> a) {
    __shared__ double red[256];
    if (*a.stop != 0) return;
    const int r = blockIdx.x;
    const long RM = (long)a.R * a.M;
    const T jit = (T)MUM_J;
    T wo[MSA_PER], wn[MSA_PER];
    T ss = T(0);
#pragma unroll
    for (int i = 0; i < MSA_PER; ++i) {
        const int m = threadIdx.x + 256 * i;
        wo[i] = wn[i] = T(0);
        if (m < a.M) {
            const T w = a.W[(long)m * a.ws_m + (long)r * a.ws_r];
            T v = w;
            if (a.mode != MUS_NORM) {
                const T* __restrict__ p = a.part + (long)m * a.ldp + r;
                T gp = T(0), gn = T(0);
                for (int s = 0; s < a.S; ++s) {
                    gp += p[(long)s * 2 * a.slab];
                    gn += p[((long)s * 2 + 1) * a.slab];
                }
                const long e = (long)r * a.M + m;
                if (METHOD == EVC_STOCH_SVRMU) {
                    if (a.mode == MUS_ACC) {
                        T fp = (a.first ? T(0) : a.acc[e]) + gp, fn = (a.first ? T(0) : a.acc[RM + e]) + gn;
                        if (a.last) {
                            fp = fp / a.n_loop;
                            fn = fn / a.n_loop;
                        }
                        a.acc[e] = fp;
                        a.acc[RM + e] = fn;
                    } else {
                        const T P = (gp + a.prev[RM + e]) + a.acc[e], Q = (gn + a.prev[e]) + a.acc[RM + e];
                        const T aP = a.rho * P;
                        v = w * (a.omr + aP / max_nan(Q, jit));
                        v = max_nan(v, T(0));
                        a.prev[e] = gp;
                        a.prev[RM + e] = gn;
                    }
                } else {
                    T num = gp, den = gn;
                    if (METHOD != EVC_STOCH_ASG) {
                        const T ap = a.first ? T(0) : a.acc[e], an = a.first ? T(0) : a.acc[RM + e];
                        num = a.omr * ap + a.rho * gp;
                        den = a.omr * an + a.rho * gn;
                        a.acc[e] = num;
                        a.acc[RM + e] = den;
                    }
                    if (a.mode == MUS_UPDATE) {
                        const T wp = w * max_nan(num, T(0));
                        v = wp / max_nan(den, jit);
                    }
                }
            }
            wo[i] = w;
            wn[i] = v;
            ss += v * v;
        }
    }
    if (a.mode == MUS_ACC) return;          // uniform
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
    for (int i = 0; i < MSA_PER; ++i) {
        const int m = threadIdx.x + 256 * i;
        if (m < a.M) {
            const T v = wn[i] / norm;
            a.dst[(long)m * a.ds_m + (long)r * a.ds_r] = v;
            d = max_pass_nan(d, fabs((double)(wo[i] - v)));
        }
    }
    red[threadIdx.x] = d;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] = max_pass_nan(red[threadIdx.x], red[threadIdx.x + k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) a.astat[r] = red[0];
}

// stat = max_r astat[r] in a fixed order (every workgroup forms it: no exchange); workgroup 0 records it and, if stat < tol,
// sets the stop word to the step; else workgroup j copies the candidate's atoms [16 j, 16 j + 16) into W
template <typename T>
__global__ __launch_bounds__(256) void k_mus_commit(const T* __restrict__ cand, T* __restrict__ W, long ws_m, long ws_r,
                                                    const double* __restrict__ astat, int M, int R, double* trace_slot, double tol,
                                                    int step_no, int* stop) {
    __shared__ double red[256];
    __shared__ int stopped;
    // one read per workgroup: workgroup 0 of this very launch may be setting the word
    if (threadIdx.x == 0) stopped = *stop;
    __syncthreads();
    if (stopped != 0) return;
    double d = 0.0;
    for (int r = threadIdx.x; r < R; r += 256) d = max_pass_nan(d, astat[r]);
    red[threadIdx.x] = d;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] = max_pass_nan(red[threadIdx.x], red[threadIdx.x + k]);
        __syncthreads();
    }
    const double stat = red[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *trace_slot = stat;
        if (stat < tol) *stop = step_no;
    }
    if (stat < tol) return;
    const int r0 = blockIdx.x * MSC_ATOMS, r1 = r0 + MSC_ATOMS < R ? r0 + MSC_ATOMS : R;
    for (int r = r0; r < r1; ++r)
        for (int m = threadIdx.x; m < M; m += 256) W[(long)m * ws_m + (long)r * ws_r] = cand[(long)r * M + m];
}

unsigned mus_blocks(long n) { return (unsigned)((n + 255) / 256); }

// arguments already validated by evc_mu_stoch_learn; returns ST_OK, ST_WORKSPACE or a hipError_t
template <typename T>
int mus_learn(const void* X_, int ldx, const void* mask_, int ldm, void* W_, int ldw, void* H_, int ldh, const int* order, int M,
              int R, int T_, const evc_mu_stoch_opts& o, bool fused, int S, void* ws, size_t ws_bytes, int* n_epochs_out,
              int* n_steps_out, double* trace_out, hipStream_t s) {
    const int bs = o.batch_size, n_loop = mus_n_loop(T_, bs), method = o.method;
    const MusWs w = carve_mus(ws, M, R, T_, bs, method, o.dtype);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const Dims d = make_dims((int)sizeof(T), M, R, bs, 1);
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    const T* X = static_cast<const T*>(X_);
    const T* mask = static_cast<const T*>(mask_);
    T* W = static_cast<T*>(W_);
    T* H = static_cast<T*>(H_);
    T *HF = reinterpret_cast<T*>(w.HF), *Xt = reinterpret_cast<T*>(w.Xt), *Mt = mask ? reinterpret_cast<T*>(w.Mt) : nullptr;
    T *Am = reinterpret_cast<T*>(w.Am), *Vt = reinterpret_cast<T*>(w.Vt), *Q1t = reinterpret_cast<T*>(w.Q1t);
    T *Q2t = reinterpret_cast<T*>(w.Q2t), *part = reinterpret_cast<T*>(w.part), *acc = reinterpret_cast<T*>(w.acc);
    T *prev = reinterpret_cast<T*>(w.prev), *cand = reinterpret_cast<T*>(w.cand);
    const int MTp = learn_bin_tiles(M);
    const long slab = (long)MTp * 16 * d.Np, RM = (long)R * M;
    const long ws_m = fm ? 1 : ldw, ws_r = fm ? ldw : 1;
    const int per_epoch = method == EVC_STOCH_GSAG ? 1 : n_loop;        // trace slots

    // the activation half: k_mum_sweep over the batch as one utterance, on H_F
    MumCtx<T> c;
    c.w = carve_mum(w.solve_ws, M, R, bs, 1, o.dtype);
    if (c.w.bytes > w.solve_bytes) return ST_WORKSPACE;
    c.n_utt = 1; c.n_slots = 1; c.fm = fm ? 1 : 0;
    HIP_TRY(frame_tiles_stage(BT_F, nullptr, 1, bs, c.w.tiles, c.w.utt_tile0, nullptr, s, &c.n_tiles));
    MumArgs<T>& a = c.a;
    a.Ap1 = reinterpret_cast<T*>(c.w.Ap1); a.Ap3 = reinterpret_cast<T*>(c.w.Ap3);
    a.Xp = reinterpret_cast<T*>(c.w.Xp); a.XMp = reinterpret_cast<T*>(c.w.XMp); a.Mp = reinterpret_cast<T*>(c.w.Mp);
    a.H = HF; a.hs_t = d.Np; a.hs_n = 1;
    a.tiles = c.w.tiles; a.stop = w.stop; a.errf = c.w.errf;
    a.M = M; a.MP = d.Mk; a.N = R; a.NP = round_up(R, 16);
    HIP_TRY(mum_sweep_prepare<T>());
    if (fused) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mus_dict_grad<T, EVC_LOSS_FROBENIUS>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)mdg_lds_bytes<T>(MUS_FUSED_MAX_R)));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mus_dict_grad<T, EVC_LOSS_KL>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)mdg_lds_bytes<T>(MUS_FUSED_MAX_R)));
    }
    HIP_TRY(hipMemsetAsync(w.stop, 0, sizeof(int), s));
    HIP_TRY(hipMemsetAsync(HF, 0, (size_t)d.Tp * d.Np * sizeof(T), s));
    HIP_TRY(hipMemsetAsync(Xt, 0, (size_t)d.Tp * d.Mk * sizeof(T), s));
    if (Mt) HIP_TRY(hipMemsetAsync(Mt, 0, (size_t)d.Tp * d.Mk * sizeof(T), s));

    MusGatherArgs<T> ga;
    ga.X = X; ga.mask = mask; ga.H = H; ga.ldx = ldx; ga.ldm = ldm; ga.fm = fm ? 1 : 0;
    ga.hs_t = fm ? ldh : 1; ga.hs_n = fm ? 1 : ldh;
    ga.ord = order ? w.ord : nullptr; ga.t0 = 0; ga.bs = bs;
    ga.M = M; ga.MP = d.Mk; ga.Mk = d.Mk; ga.R = R; ga.Np = d.Np; ga.n_tiles = c.n_tiles;
    ga.XMp = reinterpret_cast<T*>(c.w.XMp); ga.Mp = reinterpret_cast<T*>(c.w.Mp);
    ga.Xt = Xt; ga.Mt = Mt; ga.HF = HF; ga.stop = w.stop;
    const long n_gather = (long)c.n_tiles * d.Mk * BT_F + (long)bs * d.Mk + (long)bs * R;
    auto gather = [&](int b) -> int {
        ga.t0 = b * bs;
        hipLaunchKernelGGL(k_mus_gather<T>, dim3(mus_blocks(n_gather)), dim3(256), 0, s, ga);
        return (int)hipGetLastError();
    };
    auto scatter = [&]() -> int {
        hipLaunchKernelGGL(k_mus_scatter<T>, dim3(mus_blocks((long)bs * R)), dim3(256), 0, s, ga);
        return (int)hipGetLastError();
    };

    // [g+ | g-] of the gathered batch into S slabs
    MusDictArgs<T> da;
    da.Xt = Xt; da.Mt = Mt; da.Ht = HF; da.W = W; da.ws_m = ws_m; da.ws_r = ws_r; da.part = part;
    da.ldx = d.Mk; da.ldh = d.Np; da.M = M; da.R = R; da.RP16 = round_up(R, 16); da.MTp = MTp; da.T_ = bs; da.S = S;
    da.stop = w.stop;
    auto grads = [&]() -> int {
        if (fused) {
            const dim3 grid(round_up(R, MDG_RB * 16) / (MDG_RB * 16), d.Mk / 16, S);
            if (o.loss == EVC_LOSS_KL)
                hipLaunchKernelGGL((k_mus_dict_grad<T, EVC_LOSS_KL>), grid, dim3(64 * MDG_WAVES), mdg_lds_bytes<T>(da.RP16), s, da);
            else
                hipLaunchKernelGGL((k_mus_dict_grad<T, EVC_LOSS_FROBENIUS>), grid, dim3(64 * MDG_WAVES), mdg_lds_bytes<T>(da.RP16),
                                   s, da);
            return (int)hipGetLastError();
        }
        // evc_mu_masked_learn's route on the gathered copies (H_F is a frames-as-rows operand already)
        HIP_TRY(copy2d<T>(W, ldw, M, R, fm ? 1 : 0, Am, d.Np, d.Mj, d.Np, 0, s));
        HIP_TRY(gemm_nt<T>(HF, d.Np, Am, d.Np, Vt, d.Mj, d.Tp, d.Mj, d.Np, s, nullptr, 0, nullptr, d.Mk));
        HIP_TRY(mum_dict_q<T>(o.loss, Xt, d.Mk, Mt, d.Mk, 1, Vt, Q1t, Q2t, d.Mj, M, bs, (long)d.Tp, s));
        return (int)dict_grad<T>(Q1t, d.Mj, Q2t, d.Mj, HF, d.Np, M, bs, S, part, s);
    };

    MusApplyArgs<T> aa;
    aa.part = part; aa.slab = slab; aa.S = S; aa.ldp = d.Np; aa.W = W; aa.ws_m = ws_m; aa.ws_r = ws_r;
    aa.acc = acc; aa.prev = prev; aa.astat = w.astat; aa.stop = w.stop; aa.M = M; aa.R = R;
    aa.n_loop = (T)n_loop;
    if (method == EVC_STOCH_SVRMU) { aa.omr = (T)(1.0 - o.alpha); aa.rho = (T)o.alpha; }
    else { aa.omr = (T)(1.0 - o.forget_rate); aa.rho = (T)o.forget_rate; }
    auto apply = [&](int mode, int first, int last, int b) -> int {
        aa.mode = mode; aa.first = first; aa.last = last;
        aa.dst = mode == MUS_NORM ? W : cand;
        aa.ds_m = mode == MUS_NORM ? ws_m : 1; aa.ds_r = mode == MUS_NORM ? ws_r : M;
        aa.prev = method == EVC_STOCH_SVRMU ? prev + (long)b * 2 * RM : nullptr;
        switch (method) {
            case EVC_STOCH_ASG: hipLaunchKernelGGL((k_mus_apply<T, EVC_STOCH_ASG>), dim3(R), dim3(256), 0, s, aa); break;
            case EVC_STOCH_SVRMU: hipLaunchKernelGGL((k_mus_apply<T, EVC_STOCH_SVRMU>), dim3(R), dim3(256), 0, s, aa); break;
            default: hipLaunchKernelGGL((k_mus_apply<T, EVC_STOCH_ASAG>), dim3(R), dim3(256), 0, s, aa); break;
        }
        return (int)hipGetLastError();
    };
    auto commit = [&](int slot, int step_no) -> int {
        hipLaunchKernelGGL(k_mus_commit<T>, dim3((R + MSC_ATOMS - 1) / MSC_ATOMS), dim3(256), 0, s, (const T*)cand, W, ws_m, ws_r,
                           (const double*)w.astat, M, R, w.trace + slot, o.tol, step_no, w.stop);
        return (int)hipGetLastError();
    };

    const long total = mus_updates(method, o.epochs, n_loop);
    if (trace_out) for (long i = 0; i < total; ++i) trace_out[i] = __builtin_nan("");
    if (method == EVC_STOCH_SVRMU && o.epochs > 0) HIP_TRY(hipMemsetAsync(prev, 0, (size_t)n_loop * 2 * RM * sizeof(T), s));
    HIP_TRY(apply(MUS_NORM, 0, 0, 0));                                   // nmf.solve normalises the start dictionary
    if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
    int h_stop = 0;
    for (int e = 0; e < o.epochs && h_stop == 0; ++e) {
        if (order && (e == 0 || o.order_rows > 1))
            HIP_TRY(hipMemcpyAsync(w.ord, order + (size_t)e * T_, sizeof(int) * (size_t)T_, hipMemcpyHostToDevice, s));
        if (trace_out) HIP_TRY(hipMemsetAsync(w.trace, 0xff, sizeof(double) * (size_t)per_epoch, s));      // NaN: not evaluated
        if (method == EVC_STOCH_SVRMU)
            for (int b = 0; b < n_loop; ++b) {                          // the full gradient of the current factors
                HIP_TRY(gather(b));
                HIP_TRY(grads());
                HIP_TRY(apply(MUS_ACC, b == 0, b == n_loop - 1, b));
            }
        for (int b = 0; b < n_loop; ++b) {
            const int step_no = e * n_loop + b + 1;
            const bool last = b == n_loop - 1;
            HIP_TRY(gather(b));
            HIP_TRY(mum_pack_dict<T>(c, W, ldw, s));
            for (int k = 0; k < o.inner_iters; ++k) HIP_TRY(mum_sweep<T>(c.a, o.loss, c.n_tiles, s));
            HIP_TRY(scatter());
            HIP_TRY(grads());
            if (method == EVC_STOCH_GSAG) {
                HIP_TRY(apply(last ? MUS_UPDATE : MUS_ACC, b == 0, 0, b));
                if (last) HIP_TRY(commit(0, step_no));
            } else {
                HIP_TRY(apply(MUS_UPDATE, b == 0, 0, b));
                HIP_TRY(commit(b, step_no));
            }
        }
        // once per epoch: the epoch's statistics, and - only where a stop is possible - the stop word
        if (trace_out)
            HIP_TRY(hipMemcpyAsync(trace_out + (long)e * per_epoch, w.trace, sizeof(double) * (size_t)per_epoch,
                                   hipMemcpyDeviceToHost, s));
        if (o.tol > 0.0) {
            HIP_TRY(hipMemcpyAsync(&h_stop, w.stop, sizeof(int), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    if (trace_out) {
        HIP_TRY(hipStreamSynchronize(s));
        const long done = h_stop == 0 ? total : method == EVC_STOCH_GSAG ? (h_stop + n_loop - 1) / n_loop : h_stop;
        for (long i = done; i < total; ++i) trace_out[i] = __builtin_nan("");
    }
    if (n_steps_out) *n_steps_out = h_stop ? h_stop : o.epochs * n_loop;
    if (n_epochs_out) *n_epochs_out = h_stop ? (h_stop + n_loop - 1) / n_loop : o.epochs;
    return ST_OK;
}

}  // namespace

}  // namespace evc

extern "C" {

size_t evc_mu_stoch_learn_workspace_bytes(int M, int R, int T, int batch_size, int method, int dtype) {
    return evc::mus_workspace_bytes(M, R, T, batch_size, method, dtype);
}

int evc_mu_stoch_learn_route(int R, int route) {
    if (R < 1 || R > evc::MUS_MAX_R || route < 0 || route > 2 || (route == 1 && R > evc::MUS_FUSED_MAX_R)) return 0;
    return evc::mus_route(route, R);
}

int evc_mu_stoch_learn_splits(int M, int R, int batch_size, int route) {
    const int rt = evc_mu_stoch_learn_route(R, route);
    if (!rt || M < 1 || M > evc::MUM_MAX_M || batch_size < 1) return 0;
    if (rt == 2) return evc::learn_splits(M, R, batch_size);
    // fused: ranges of at least 64 frames, 16 for each wavefront
    const int S = batch_size / 64;
    return S < 1 ? 1 : S > evc::LEARN_MAX_SPLITS ? evc::LEARN_MAX_SPLITS : S;
}

int evc_mu_stoch_learn(const void* X, int ldx, const void* mask, int ldm, void* W, int ldw, void* H, int ldh, const int* order,
                       int M, int R, int T, const evc_mu_stoch_opts* opts, void* workspace, size_t workspace_bytes,
                       int* n_epochs_out, int* n_steps_out, double* trace_out, evc_stream_t stream) {
    using namespace evc;
    HIP_TRY(mus_args_check(X, ldx, mask, ldm, W, ldw, H, ldh, order, M, R, T, opts, workspace, workspace_bytes));
    const evc_mu_stoch_opts& o = *opts;
    const bool fused = mus_route(o.route, R) == 1;
    const int S = evc_mu_stoch_learn_splits(M, R, o.batch_size, o.route);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return (o.dtype == EVC_F64 ? mus_learn<double> : mus_learn<float>)(X, ldx, mask, ldm, W, ldw, H, ldh, order, M, R, T, o, fused, S,
                                                                        workspace, workspace_bytes, n_epochs_out, n_steps_out,
                                                                        trace_out, s);
}

}  // extern "C"
