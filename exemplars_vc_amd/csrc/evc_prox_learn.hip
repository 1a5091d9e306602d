// evc_prox_learn.hip - evc_prox_learn: sparse dictionary learning, Mairal et al.'s online method as deComP runs it
// (dictionary_learning.py:114-168, method='block_cd').  DESIGN.md §5.19.
//
// One step on a batch F of bs frames:
//   lasso       k_plearn_gather copies the batch's columns of H and X into Z (the caller's layout, contiguous), evc_prox_solve
//               runs on Z as one utterance with nothing asked back (it then never waits for the stream), k_plearn_scatter
//               puts the activations back
//   statistics  k_plearn_stats: C = [S | Q] <- beta C + H_F [H_F; X_F]^T in one launch.  A workgroup of 4 wavefronts owns
//               64 rows x 64 columns of C and streams the batch's frames ascending in slabs of 16, double-buffered in LDS as
//               k_prox_sweep stages its slabs; a wavefront owns 16 rows x 64 columns in 4 accumulators of 16x16x4 MFMAs.  The
//               decay is the epilogue.  Every output is one frame-ascending chain: no split over frames, no atomics.
//   sweep       blocked and right-looking, nb = plearn_block(M, dtype) atoms per block.  Rm = Q - S D^T (the strided
//               contraction into Rm, k_plearn_resid subtracts and keeps the old atoms in Dw); then per block K one launch of
//               k_plearn_block.  Every workgroup first redoes the block's sequential updates - for atom i of the block
//                   r = Rm[k] - sum_{j < i} S[k, k0 + j] dD_j;  u = r / (S_kk + 1e-15) + d_k;  d_k' = u / sqrt(max(|u|^2, 1))
//               a thread owning the bins tid, tid + 256, ..., |u|^2 by registers, wave shuffle and LDS in one fixed tree: the same
//               instructions in the same order in every workgroup, hence the same bits - and then takes S[rows, K] dD off its own
//               PLEARN_ROWS rows of Rm behind the block.  Workgroup 0 alone stores the new atoms to the caller's D and the
//               block's share of max |dD|.  The launch boundary is the only dependency between blocks.
//   stop        k_plearn_stat takes the maximum of the shares in index order; the host reads that one double.
// Nothing here exchanges data between workgroups inside a launch, uses float atomics or assumes residency.
#include "evc_prox_learn_kernels.h"

namespace evc {

namespace {

constexpr int PLS_KS = 16;                 // frames per slab
constexpr int PLS_B = 64;                  // rows and columns of C per workgroup
constexpr int PLS_LD = PLS_B + 16;

// C[i][j] <- beta C[i][j] + sum_t Z(t, i) Z(t, j), i < N, j < N + M, t ascending over the batch
template <typename T>
__global__ __launch_bounds__(256) void k_plearn_stats(const T* __restrict__ Z, long zs_t, long zs_r, int bs, int N, int M,
                                                      T beta, T* __restrict__ C, long ldc) {
    typedef typename Mma<T>::acc_t acc_t;
    __shared__ T As[2][PLS_KS * PLS_LD];
    __shared__ T Bs[2][PLS_KS * PLS_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, q = lane >> 4;
    const int R = N + M;
    const int i0 = blockIdx.y * PLS_B, j0 = blockIdx.x * PLS_B;

    acc_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = acc_t{0, 0, 0, 0};

    // what a thread stages of a slab: 4 elements of each operand, along whichever direction is contiguous in Z
    int sk[4], sr[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (zs_r == 1) { sr[e] = tid & 63; sk[e] = (tid >> 6) + 4 * e; } else { sk[e] = tid & 15; sr[e] = (tid >> 4) + 16 * e; }
    }
    T pa[4], pb[4];
    auto fetch = [&](int t0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long t = t0 + sk[e];
            const int ri = i0 + sr[e], rj = j0 + sr[e];
            pa[e] = (t < bs && ri < N) ? Z[t * zs_t + ri * zs_r] : T(0);
            pb[e] = (t < bs && rj < R) ? Z[t * zs_t + rj * zs_r] : T(0);
        }
    };
    auto stage = [&](int b) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            As[b][sk[e] * PLS_LD + sr[e]] = pa[e];
            Bs[b][sk[e] * PLS_LD + sr[e]] = pb[e];
        }
    };

    const int NS = (bs + PLS_KS - 1) / PLS_KS;
    fetch(0);
    stage(0);
    __syncthreads();
#pragma unroll 1
    for (int sl = 0; sl < NS; ++sl) {
        const int b = sl & 1;
        if (sl + 1 < NS) fetch((sl + 1) * PLS_KS);
        const T* as = &As[b][q * PLS_LD + wave * 16 + i16];
        const T* bs_ = &Bs[b][q * PLS_LD + i16];
#pragma unroll
        for (int st = 0; st < PLS_KS / 4; ++st) {
            const T a = as[st * 4 * PLS_LD];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = Mma<T>::mma(a, bs_[st * 4 * PLS_LD + j * 16], acc[j]);
        }
        if (sl + 1 < NS) stage(b ^ 1);         // last read two barriers ago
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = j0 + j * 16 + i16;
        if (col >= R) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = i0 + wave * 16 + Mma<T>::row(lane, r);
            if (row >= N) continue;
            T* pc = C + (long)row * ldc + col;
            *pc = beta * *pc + acc[j][r];
        }
    }
}

// Rm[k][m] = Q[k][m] - Rm[k][m] (Rm holds S D^T on entry);  Dw[k][m] = D(m, k): the step's old atoms
template <typename T>
__global__ __launch_bounds__(256) void k_plearn_resid(const T* __restrict__ C, long ldc, const T* __restrict__ D, long ds_n,
                                                      long ds_m, T* __restrict__ Rm, T* __restrict__ Dw, int N, int M, int m_fast) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)N * M) return;
    const int k = m_fast ? (int)(i / M) : (int)(i % N);
    const int m = m_fast ? (int)(i % M) : (int)(i / N);
    const long at = (long)k * M + m;
    Rm[at] = C[(long)k * ldc + N + m] - Rm[at];
    Dw[at] = D[k * ds_n + m * ds_m];
}

// One block K = [k0, k0 + nbk) of the sweep; NB: the block width this M runs (nbk <= NB: the last block may be short).
// Dynamic LDS: dD[NB][M], Sb[NB][NB] (the block's corner of S), St[PLEARN_ROWS][NB] (this workgroup's rows of S[:, K]).
template <typename T>
__global__ __launch_bounds__(PLEARN_THREADS) void k_plearn_block(const T* __restrict__ C, long ldc, T* __restrict__ Rm,
                                                                  const T* __restrict__ Dw, T* __restrict__ D, long ds_n, long ds_m,
                                                                  int N, int M, int NB, int k0, int nbk, T jitter,
                                                                  double* __restrict__ share) {
    extern __shared__ __attribute__((aligned(16))) unsigned char plearn_lds[];
    __shared__ T red[2][PLEARN_THREADS / 64];
    __shared__ double redm[PLEARN_THREADS / 64];
    T* dD = reinterpret_cast<T*>(plearn_lds);
    T* Sb = dD + (long)NB * M;
    T* St = Sb + NB * NB;
    const int tid = threadIdx.x;
    const bool first = blockIdx.x == 0;
    const int r0 = k0 + nbk + blockIdx.x * PLEARN_ROWS;        // this workgroup's rows of Rm: [r0, r1)
    const int r1 = r0 + PLEARN_ROWS < N ? r0 + PLEARN_ROWS : N;

    for (int e = tid; e < nbk * nbk; e += PLEARN_THREADS) Sb[(e / nbk) * NB + e % nbk] = C[(long)(k0 + e / nbk) * ldc + k0 + e % nbk];
    for (int e = tid; e < (r1 - r0) * nbk; e += PLEARN_THREADS) St[(e / nbk) * NB + e % nbk] = C[(long)(r0 + e / nbk) * ldc + k0 + e % nbk];
    __syncthreads();

    double worst = -__builtin_inf();
    for (int i = 0; i < nbk; ++i) {
        const int k = k0 + i;
        const T den = Sb[i * NB + i] + jitter;
        T ss = T(0);
        for (int m = tid; m < M; m += PLEARN_THREADS) {        // a thread reads and writes its own bins of dD only
            T r = Rm[(long)k * M + m];
#pragma unroll 4
            for (int j = 0; j < i; ++j) r = r - Sb[i * NB + j] * dD[(long)j * M + m];
            const T u = r / den + Dw[(long)k * M + m];
            dD[(long)i * M + m] = u;
            ss += u * u;
        }
        ss = plearn_sum(ss, red[i & 1]);
        const T nrm = plsqrt(ss != ss ? ss : (ss > T(1) ? ss : T(1)));
        for (int m = tid; m < M; m += PLEARN_THREADS) {
            const T dk = Dw[(long)k * M + m];
            const T dn = dD[(long)i * M + m] / nrm;
            const T dd = dn - dk;
            dD[(long)i * M + m] = dd;
            if (first) {
                D[k * ds_n + m * ds_m] = dn;
                worst = plmax(worst, (double)plabs(dd));
            }
        }
    }
    __syncthreads();            // the update below reads every bin's dD

    // Rm[row] -= sum_j S[row, k0 + j] dD_j, j ascending, for the rows behind the block (none: the workgroup is done)
    for (int e = tid; e < (r1 - r0) * M; e += PLEARN_THREADS) {
        const int rr = e / M, m = e % M;
        T acc = Rm[(long)(r0 + rr) * M + m];
#pragma unroll 4
        for (int j = 0; j < nbk; ++j) acc = acc - St[rr * NB + j] * dD[(long)j * M + m];
        Rm[(long)(r0 + rr) * M + m] = acc;
    }

    if (!first) return;         // uniform
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) worst = plmax(worst, __shfl_xor(worst, o, 64));
    if ((tid & 63) == 0) redm[tid >> 6] = worst;
    __syncthreads();
    if (tid == 0) {
        double m = redm[0];
        for (int w = 1; w < PLEARN_THREADS / 64; ++w) m = plmax(m, redm[w]);
        share[k0 / NB] = m;
    }
}

// stat = the maximum of the blocks' shares in index order (a NaN wins)
__global__ void k_plearn_stat(const double* __restrict__ share, int n, double* __restrict__ stat) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double m = share[0];
    for (int i = 1; i < n; ++i) m = plmax(m, share[i]);
    *stat = m;
}

// arguments already validated by plearn_args_check; returns ST_OK, ST_WORKSPACE or a hipError_t
template <typename T>
int prox_learn(const T* X, int ldx, T* D, int ldd, T* H, int ldh, T* C, int ldc, long long* count_io, const int* order, int M,
               int N, int T_, const evc_prox_learn_opts& o, void* ws, size_t ws_bytes, int* n_epochs_out, int* n_steps_out,
               double* trace_out, hipStream_t s) {
    const int bs = o.batch_size, nbat = T_ / bs;
    const PLearnWs w = carve_plearn(ws, M, N, T_, bs, o.dtype);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    const long xs_t = fm ? ldx : 1, xs_m = fm ? 1 : ldx, hs_t = fm ? ldh : 1, hs_n = fm ? 1 : ldh;
    const long ds_n = fm ? ldd : 1, ds_m = fm ? 1 : ldd;
    const int R = N + M;
    T* Z = reinterpret_cast<T*>(w.Z);
    T* Rm = reinterpret_cast<T*>(w.Rm);
    T* Dw = reinterpret_cast<T*>(w.Dw);
    const long zs_t = fm ? R : 1, zs_r = fm ? 1 : bs;
    T* Zx = Z + (fm ? (long)N : (long)N * bs);           // the batch's X inside Z
    const int ldz = fm ? R : bs;
    const int NB = plearn_block(M, o.dtype), n_blocks = (N + NB - 1) / NB;
    const size_t lds = ((size_t)NB * M + (size_t)NB * NB + (size_t)PLEARN_ROWS * NB) * sizeof(T);
    const evc_prox_opts po = plearn_lasso_opts<evc_prox_opts>(o);
    const bool lasso = !(o.reserved & PLEARN_NO_LASSO), stats = !(o.reserved & PLEARN_NO_STATS), sweep = !(o.reserved & PLEARN_NO_SWEEP);

    if (!o.resume) {
        hipLaunchKernelGGL(k_plearn_unit<T>, dim3(N), dim3(PLEARN_THREADS), 0, s, D, ds_n, ds_m, M);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemset2DAsync(C, sizeof(T) * (size_t)ldc, 0, sizeof(T) * (size_t)R, (size_t)N, s));
        *count_io = 0;
    }
    auto stage_order = [&](int e) -> int { return plearn_stage_order(order, e, T_, w.ord, s); };
    auto step = [&](const int* ord, int t0, double forget) -> int {
        hipLaunchKernelGGL(k_plearn_gather<T>, dim3(plearn_blocks_of((long)bs * R)), dim3(256), 0, s, X, xs_t, xs_m,
                           (const T*)H, hs_t, hs_n, Z, zs_t, zs_r, ord, t0, bs, N, M, fm ? 1 : 0);
        HIP_TRY(hipGetLastError());
        if (lasso)
            HIP_TRY(evc_prox_solve(D, ldd, Zx, ldz, Z, ldz, M, N, bs, nullptr, 1, &po, w.prox_ws, w.prox_bytes, nullptr,
                                   nullptr, reinterpret_cast<evc_stream_t>(s)));
        hipLaunchKernelGGL(k_plearn_scatter<T>, dim3(plearn_blocks_of((long)bs * N)), dim3(256), 0, s, H, hs_t, hs_n,
                           (const T*)Z, zs_t, zs_r, ord, t0, bs, N, fm ? 1 : 0);
        HIP_TRY(hipGetLastError());

        const T beta = (T)forget;
        if (stats) {
            hipLaunchKernelGGL(k_plearn_stats<T>, dim3((R + PLS_B - 1) / PLS_B, (N + PLS_B - 1) / PLS_B), dim3(256), 0, s,
                               (const T*)Z, zs_t, zs_r, bs, N, M, beta, C, (long)ldc);
            HIP_TRY(hipGetLastError());
        }

        if (sweep) {
            // Rm <- S D^T, then Q - that
            HIP_TRY(gemm_strided<T>(C, ldc, 1, D, ds_m, ds_n, Rm, M, 1, N, M, N, s));
            hipLaunchKernelGGL(k_plearn_resid<T>, dim3(plearn_blocks_of((long)N * M)), dim3(256), 0, s, (const T*)C, (long)ldc,
                               (const T*)D, ds_n, ds_m, Rm, Dw, N, M, fm ? 1 : 0);
            HIP_TRY(hipGetLastError());
            for (int k0 = 0; k0 < N; k0 += NB) {
                const int nbk = N - k0 < NB ? N - k0 : NB;
                const int behind = N - k0 - nbk;
                const int tiles = (behind + PLEARN_ROWS - 1) / PLEARN_ROWS;
                hipLaunchKernelGGL(k_plearn_block<T>, dim3(tiles > 0 ? tiles : 1), dim3(PLEARN_THREADS), lds, s, (const T*)C,
                                   (long)ldc, Rm, (const T*)Dw, D, ds_n, ds_m, N, M, NB, k0, nbk, (T)1e-15, w.shares);
                HIP_TRY(hipGetLastError());
            }
        }
        return ST_OK;
    };
    auto read_stat = [&](double* stat) -> int {
        hipLaunchKernelGGL(k_plearn_stat, dim3(1), dim3(64), 0, s, (const double*)w.shares, n_blocks, w.stat);
        HIP_TRY(hipGetLastError());
        return plearn_fetch_stat(w.stat, stat, s);
    };
    return plearn_loop(o, nbat, sweep, order ? w.ord : nullptr, count_io, n_epochs_out, n_steps_out, trace_out, s, stage_order,
                       step, read_stat);
}

}  // namespace

}  // namespace evc

extern "C" {

size_t evc_prox_learn_workspace_bytes(int M, int N, int T, int batch_size, int dtype) {
    return evc::prox_learn_workspace_bytes(M, N, T, batch_size, dtype);
}

int evc_prox_learn_block(int M, int dtype) {
    if (M < 1 || M > evc::PLEARN_MAX_M || (dtype != EVC_F64 && dtype != EVC_F32)) return 0;
    return evc::plearn_block(M, dtype);
}

int evc_prox_learn(const void* X, int ldx, void* D, int ldd, void* H, int ldh, void* stats, int ld_stats, long long* count_io,
                   const int* order, int M, int N, int T, const evc_prox_learn_opts* opts, void* workspace,
                   size_t workspace_bytes, int* n_epochs_out, int* n_steps_out, double* trace_out, evc_stream_t stream) {
    using namespace evc;
    HIP_TRY(plearn_args_check(X, ldx, D, ldd, H, ldh, stats, ld_stats, count_io, order, M, N, T, opts, workspace,
                              workspace_bytes));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (opts->dtype == EVC_F64)
        return prox_learn<double>(static_cast<const double*>(X), ldx, static_cast<double*>(D), ldd, static_cast<double*>(H), ldh,
                                  static_cast<double*>(stats), ld_stats, count_io, order, M, N, T, *opts, workspace,
                                  workspace_bytes, n_epochs_out, n_steps_out, trace_out, s);
    return prox_learn<float>(static_cast<const float*>(X), ldx, static_cast<float*>(D), ldd, static_cast<float*>(H), ldh,
                             static_cast<float*>(stats), ld_stats, count_io, order, M, N, T, *opts, workspace, workspace_bytes,
                             n_epochs_out, n_steps_out, trace_out, s);
}

}  // extern "C"
