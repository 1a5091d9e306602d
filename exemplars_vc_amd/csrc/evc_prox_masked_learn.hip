// evc_prox_masked_learn.hip - evc_prox_masked_learn: sparse dictionary learning with a weight per bin of every frame, as
// deComP's solve_cd_mask runs it (dictionary_learning.py:171-231).  DESIGN.md §5.20.
//
// One step on a batch F of bs frames:
//   lasso       k_plearn_gather (twice: [H_F | X_F], then the mask's columns) copies the batch into Z (the caller's layout,
//               contiguous), evc_prox_masked_solve runs on Z as one utterance with nothing asked back, k_plearn_scatter puts
//               the activations back
//   statistics  k_pmlearn_stats: for every bin m, S_m <- beta S_m + (H_F diag(w_m)) H_F^T, and in the same pass
//               G[k][m] = sum_j S_m[k][j] D_old[j][m] and the diagonals S_m[k][k].  A workgroup of 4 wavefronts owns one bin and
//               64 rows of its plane and walks the column tiles of 64 in ascending j; per tile the batch's frames ascending in
//               slabs of 16 (float32: 32), double-buffered in LDS as k_plearn_stats stages its slabs, the left operand multiplied by
//               w[t][m] as it is staged; a wavefront owns 16 rows x 64 columns in 4 accumulators of 16x16x4 MFMAs.  The epilogue applies the
//               decay, stores the tile and adds tile . D_old[j][m] to a per-lane running sum of each of its 4 rows; after the
//               last tile one xor-shuffle tree over the 16 lanes of a row gives G.  The tensor is read once and written once.
//               k_pmlearn_q: Q <- beta Q + H_F (w . X_F)^T, one thread per entry, frames ascending (1 / N of the work)
//   atoms       k_pmlearn_atoms, one workgroup per atom, one launch: a_k = sum_m (S_m[k][k] + 1e-15) in ascending m,
//               u = (Q[k] - G[k]) / a_k + d_k, |u|^2 by plearn_sum's fixed tree, d_k' = u / sqrt(max(|u|^2, 1)) stored to the
//               caller's D and to the bin-major copy Dt, and the atom's share of max |dD|.  Every atom reads the OLD dictionary
//               only through G and its own row: a Jacobi step, as deComP's.
//   stop        k_pmlearn_stat takes the maximum of the N shares in one workgroup; the host reads that one double.
// Nothing here exchanges data between workgroups inside a launch, uses float atomics or assumes residency.
#include "evc_prox_learn_kernels.h"
#include "evc_prox_masked_learn_plan.h"

namespace evc {

namespace {

constexpr int PML_B = 64;                  // rows of a panel, columns of a tile
constexpr int PML_LD = PML_B + 16;
// frames per slab: 16 in float64, 32 in float32 - the four slab buffers take 40 KB of LDS either way
template <typename T> constexpr int pml_ks() { return 128 / (int)sizeof(T); }

// Dt[m][k] = D(m, k): the dictionary with a bin per row
template <typename T>
__global__ __launch_bounds__(256) void k_pmlearn_dcopy(const T* __restrict__ D, long ds_n, long ds_m, T* __restrict__ Dt, int N,
                                                       int M, int m_fast) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)N * M) return;
    const int k = m_fast ? (int)(i / M) : (int)(i % N);
    const int m = m_fast ? (int)(i % M) : (int)(i / N);
    Dt[(long)m * N + k] = D[k * ds_n + m * ds_m];
}

// Plane m = blockIdx.y, rows [64 blockIdx.x, + 64):  S_m[i][j] <- beta S_m[i][j] + sum_t (Z(t, i) Z(t, wcol + m)) Z(t, j) for
// every j < N, t ascending over the batch;  G[i][m] = sum_j S_m[i][j] Dt[m][j];  diag[m][i] = S_m[i][i].
// wcol = N + M: where the mask's columns start in Z.
template <typename T>
__global__ __launch_bounds__(256) void k_pmlearn_stats(const T* __restrict__ Z, long zs_t, long zs_r, int bs, int N, int wcol,
                                                       T beta, T* __restrict__ S, long lds_, const T* __restrict__ Dt,
                                                       T* __restrict__ G, int M, T* __restrict__ diag) {
    typedef typename Mma<T>::acc_t acc_t;
    constexpr int PML_KS = pml_ks<T>();
    constexpr int PML_E = PML_KS * PML_B / 256;         // elements of each operand a thread stages per slab
    __shared__ T As[2][PML_KS * PML_LD];
    __shared__ T Bs[2][PML_KS * PML_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, q = lane >> 4;
    const int m = blockIdx.y;
    const int i0 = blockIdx.x * PML_B;
    T* Sp = S + (long)m * N * lds_;
    const T* dt = Dt + (long)m * N;
    const T* Zw = Z + (long)(wcol + m) * zs_r;

    // what a thread stages of a slab: PML_E elements of each operand, along whichever direction is contiguous in Z
    int sk[PML_E], sr[PML_E];
#pragma unroll
    for (int e = 0; e < PML_E; ++e) {
        if (zs_r == 1) { sr[e] = tid & 63; sk[e] = (tid >> 6) + 4 * e; }
        else { sk[e] = tid & (PML_KS - 1); sr[e] = tid / PML_KS + (256 / PML_KS) * e; }
    }
    // Every load is unconditional, from an index clamped into the batch, and what lies outside is zeroed afterwards: a load
    // under a condition would wait for its data inside its branch, one round trip after another.
    T pa[PML_E], pb[PML_E];
    auto fetch = [&](int j0, int t0) {
        T va[PML_E], vw[PML_E];
#pragma unroll
        for (int e = 0; e < PML_E; ++e) {
            const int t = t0 + sk[e], ri = i0 + sr[e], rj = j0 + sr[e];
            const long tc = t < bs ? t : bs - 1;
            va[e] = Z[tc * zs_t + (ri < N ? ri : N - 1) * zs_r];
            vw[e] = Zw[tc * zs_t];
            pb[e] = Z[tc * zs_t + (rj < N ? rj : N - 1) * zs_r];
        }
#pragma unroll
        for (int e = 0; e < PML_E; ++e) {
            const int t = t0 + sk[e];
            pa[e] = (t < bs && i0 + sr[e] < N) ? va[e] * vw[e] : T(0);
            pb[e] = (t < bs && j0 + sr[e] < N) ? pb[e] : T(0);
        }
    };
    auto stage = [&](int b) {
#pragma unroll
        for (int e = 0; e < PML_E; ++e) {
            As[b][sk[e] * PML_LD + sr[e]] = pa[e];
            Bs[b][sk[e] * PML_LD + sr[e]] = pb[e];
        }
    };

    const int NS = (bs + PML_KS - 1) / PML_KS, NT = (N + PML_B - 1) / PML_B;
    const int total = NS * NT;
    T gs[4] = {T(0), T(0), T(0), T(0)};        // this lane's part of G for its 4 rows: the columns i16, i16 + 16, ... so far
    acc_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = acc_t{0, 0, 0, 0};

    fetch(0, 0);
    stage(0);
    __syncthreads();
#pragma unroll 1
    for (int it = 0, jt = 0, sl = 0; it < total; ++it) {
        const int b = it & 1;
        if (it + 1 < total) {                   // the next slab: of this tile, or the first of the next
            if (sl + 1 < NS) fetch(jt * PML_B, (sl + 1) * PML_KS); else fetch((jt + 1) * PML_B, 0);
        }
        const T* as = &As[b][q * PML_LD + wave * 16 + i16];
        const T* bs_ = &Bs[b][q * PML_LD + i16];
#pragma unroll
        for (int st = 0; st < PML_KS / 4; ++st) {
            const T a = as[st * 4 * PML_LD];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = Mma<T>::mma(a, bs_[st * 4 * PML_LD + j * 16], acc[j]);
        }
        if (sl == NS - 1) {                     // the tile's frames are in: decay, store, and the tile's share of G
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = jt * PML_B + j * 16 + i16;
                const T dj = col < N ? dt[col] : T(0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = i0 + wave * 16 + Mma<T>::row(lane, r);
                    if (col < N && row < N) {
                        T* pc = Sp + (long)row * lds_ + col;
                        const T v = beta * *pc + acc[j][r];
                        *pc = v;
                        gs[r] += v * dj;
                        if (row == col) diag[(long)m * N + row] = v;
                    }
                }
                acc[j] = acc_t{0, 0, 0, 0};
            }
        }
        if (it + 1 < total) stage(b ^ 1);       // last read two barriers ago
        __syncthreads();
        if (++sl == NS) { sl = 0; ++jt; }
    }

    // the 16 lanes of a row hold its partial sums: one fixed tree, lane i16 == 0 stores
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        T v = gs[r];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        const int row = i0 + wave * 16 + Mma<T>::row(lane, r);
        if (i16 == 0 && row < N) G[(long)row * M + m] = v;
    }
}

// Q[k][m] <- beta Q[k][m] + sum_t Z(t, k) (Z(t, wcol + m) Z(t, N + m)), t ascending over the batch
template <typename T>
__global__ __launch_bounds__(256) void k_pmlearn_q(const T* __restrict__ Z, long zs_t, long zs_r, int bs, int N, int M, T beta,
                                                   T* __restrict__ Q, long ldq) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)N * M) return;
    const int k = (int)(i / M), m = (int)(i % M);
    const T* zh = Z + (long)k * zs_r;
    const T* zx = Z + (long)(N + m) * zs_r;
    const T* zw = Z + (long)(N + M + m) * zs_r;
    T acc = T(0);
#pragma unroll 16
    for (long t = 0; t < bs; ++t) acc += zh[t * zs_t] * (zw[t * zs_t] * zx[t * zs_t]);      // the loads ahead, one chain
    T* pq = Q + (long)k * ldq + m;
    *pq = beta * *pq + acc;
}

// stat = the maximum of the atoms' shares (a NaN wins), by one workgroup: the maximum does not depend on the order
__global__ __launch_bounds__(PLEARN_THREADS) void k_pmlearn_stat(const double* __restrict__ share, int n, double* __restrict__ stat) {
    __shared__ double redm[PLEARN_THREADS / 64];
    const int tid = threadIdx.x;
    double w = -__builtin_inf();
    for (int i = tid; i < n; i += PLEARN_THREADS) w = plmax(w, share[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w = plmax(w, __shfl_xor(w, o, 64));
    if ((tid & 63) == 0) redm[tid >> 6] = w;
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < PLEARN_THREADS / 64; ++v) w = plmax(w, redm[v]);
        *stat = w;
    }
}

// Atom k = blockIdx.x, a thread owning the bins tid, tid + 256, ...
template <typename T>
__global__ __launch_bounds__(PLEARN_THREADS) void k_pmlearn_atoms(const T* __restrict__ Q, long ldq, const T* __restrict__ G,
                                                                   const T* __restrict__ diag, T* __restrict__ D, long ds_n,
                                                                   long ds_m, T* __restrict__ Dt, int N, int M, T jitter,
                                                                   double* __restrict__ share) {
    __shared__ T red[PLEARN_THREADS / 64];
    __shared__ double redm[PLEARN_THREADS / 64];
    const int tid = threadIdx.x, k = blockIdx.x;
    T a = T(0);                                 // every thread forms it, in the same order
    for (int m = 0; m < M; ++m) a += diag[(long)m * N + k] + jitter;
    T u[PMLEARN_MAX_BINS], dk[PMLEARN_MAX_BINS];
    T ss = T(0);
#pragma unroll
    for (int i = 0; i < PMLEARN_MAX_BINS; ++i) {
        const int m = tid + i * PLEARN_THREADS;
        if (m < M) {
            dk[i] = D[k * ds_n + m * ds_m];
            u[i] = (Q[(long)k * ldq + m] - G[(long)k * M + m]) / a + dk[i];
            ss += u[i] * u[i];
        }
    }
    ss = plearn_sum(ss, red);
    const T nrm = plsqrt(ss != ss ? ss : (ss > T(1) ? ss : T(1)));
    double worst = -__builtin_inf();
#pragma unroll
    for (int i = 0; i < PMLEARN_MAX_BINS; ++i) {
        const int m = tid + i * PLEARN_THREADS;
        if (m < M) {
            const T dn = u[i] / nrm;
            D[k * ds_n + m * ds_m] = dn;
            Dt[(long)m * N + k] = dn;
            worst = plmax(worst, (double)plabs(dn - dk[i]));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) worst = plmax(worst, __shfl_xor(worst, o, 64));
    if ((tid & 63) == 0) redm[tid >> 6] = worst;
    __syncthreads();
    if (tid == 0) {
        double w = redm[0];
        for (int v = 1; v < PLEARN_THREADS / 64; ++v) w = plmax(w, redm[v]);
        share[k] = w;
    }
}

// arguments already validated by pmlearn_args_check; returns ST_OK, ST_WORKSPACE or a hipError_t
template <typename T>
int prox_masked_learn(const T* X, int ldx, const T* W, int ldm, T* D, int ldd, T* H, int ldh, T* S, int ld_s, T* Q, int ld_q,
                      long long* count_io, const int* order, int M, int N, int T_, const evc_prox_masked_learn_opts& o, void* ws,
                      size_t ws_bytes, int* n_epochs_out, int* n_steps_out, double* trace_out, hipStream_t s) {
    const int bs = o.batch_size, nbat = T_ / bs;
    const PMLearnWs w = carve_pmlearn(ws, M, N, T_, bs, o.dtype);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const bool fm = o.layout == EVC_FRAME_MAJOR;
    const long xs_t = fm ? ldx : 1, xs_m = fm ? 1 : ldx, ws_t = fm ? ldm : 1, ws_m = fm ? 1 : ldm;
    const long hs_t = fm ? ldh : 1, hs_n = fm ? 1 : ldh, ds_n = fm ? ldd : 1, ds_m = fm ? 1 : ldd;
    const int R = N + 2 * M;
    T* Z = reinterpret_cast<T*>(w.Z);
    T* G = reinterpret_cast<T*>(w.G);
    T* diag = reinterpret_cast<T*>(w.diag);
    T* Dt = reinterpret_cast<T*>(w.Dt);
    const long zs_t = fm ? R : 1, zs_r = fm ? 1 : bs;
    T* Zx = Z + (long)N * zs_r;                          // the batch's X inside Z
    T* Zw = Z + (long)(N + M) * zs_r;                    // the batch's mask inside Z
    const int ldz = fm ? R : bs;
    const evc_prox_masked_opts po = pmlearn_lasso_opts(o);
    const bool lasso = !(o.reserved & PMLEARN_NO_LASSO), stats = !(o.reserved & PMLEARN_NO_STATS);
    const bool atoms = !(o.reserved & PMLEARN_NO_ATOMS);

    if (!o.resume) {
        hipLaunchKernelGGL(k_plearn_unit<T>, dim3(N), dim3(PLEARN_THREADS), 0, s, D, ds_n, ds_m, M);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemset2DAsync(S, sizeof(T) * (size_t)ld_s, 0, sizeof(T) * (size_t)N, (size_t)M * N, s));
        HIP_TRY(hipMemset2DAsync(Q, sizeof(T) * (size_t)ld_q, 0, sizeof(T) * (size_t)M, (size_t)N, s));
        *count_io = 0;
    }
    if ((long)o.epochs * nbat > 0) {
        hipLaunchKernelGGL(k_pmlearn_dcopy<T>, dim3(plearn_blocks_of((long)N * M)), dim3(256), 0, s, (const T*)D, ds_n, ds_m, Dt, N,
                           M, fm ? 1 : 0);
        HIP_TRY(hipGetLastError());
        // without the statistics (measurement only) G and the diagonals are never written: they read as zero
        if (!stats) HIP_TRY(hipMemsetAsync(w.G, 0, (size_t)(w.Dt - w.G), s));       // G and diag lie next to each other
    }
    auto stage_order = [&](int e) -> int { return plearn_stage_order(order, e, T_, w.ord, s); };
    auto step = [&](const int* ord, int t0, double forget) -> int {
        hipLaunchKernelGGL(k_plearn_gather<T>, dim3(plearn_blocks_of((long)bs * (N + M))), dim3(256), 0, s, X, xs_t, xs_m,
                           (const T*)H, hs_t, hs_n, Z, zs_t, zs_r, ord, t0, bs, N, M, fm ? 1 : 0);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_plearn_gather<T>, dim3(plearn_blocks_of((long)bs * M)), dim3(256), 0, s, W, ws_t, ws_m,
                           (const T*)nullptr, 0L, 0L, Zw, zs_t, zs_r, ord, t0, bs, 0, M, fm ? 1 : 0);
        HIP_TRY(hipGetLastError());
        if (lasso)
            HIP_TRY(evc_prox_masked_solve(D, ldd, Zx, ldz, Zw, ldz, Z, ldz, M, N, bs, nullptr, 1, &po, w.prox_ws, w.prox_bytes,
                                          nullptr, nullptr, reinterpret_cast<evc_stream_t>(s)));
        hipLaunchKernelGGL(k_plearn_scatter<T>, dim3(plearn_blocks_of((long)bs * N)), dim3(256), 0, s, H, hs_t, hs_n,
                           (const T*)Z, zs_t, zs_r, ord, t0, bs, N, fm ? 1 : 0);
        HIP_TRY(hipGetLastError());

        const T beta = (T)forget;
        if (stats) {
            hipLaunchKernelGGL(k_pmlearn_stats<T>, dim3((N + PML_B - 1) / PML_B, M), dim3(256), 0, s, (const T*)Z, zs_t, zs_r,
                               bs, N, N + M, beta, S, (long)ld_s, (const T*)Dt, G, M, diag);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_pmlearn_q<T>, dim3(plearn_blocks_of((long)N * M)), dim3(256), 0, s, (const T*)Z, zs_t, zs_r, bs,
                               N, M, beta, Q, (long)ld_q);
            HIP_TRY(hipGetLastError());
        }
        if (atoms) {
            hipLaunchKernelGGL(k_pmlearn_atoms<T>, dim3(N), dim3(PLEARN_THREADS), 0, s, (const T*)Q, (long)ld_q, (const T*)G,
                               (const T*)diag, D, ds_n, ds_m, Dt, N, M, (T)1e-15, w.shares);
            HIP_TRY(hipGetLastError());
        }
        return ST_OK;
    };
    auto read_stat = [&](double* stat) -> int {
        hipLaunchKernelGGL(k_pmlearn_stat, dim3(1), dim3(PLEARN_THREADS), 0, s, (const double*)w.shares, N, w.stat);
        HIP_TRY(hipGetLastError());
        return plearn_fetch_stat(w.stat, stat, s);
    };
    return plearn_loop(o, nbat, atoms, order ? w.ord : nullptr, count_io, n_epochs_out, n_steps_out, trace_out, s, stage_order,
                       step, read_stat);
}

}  // namespace

}  // namespace evc

extern "C" {

size_t evc_prox_masked_learn_workspace_bytes(int M, int N, int T, int batch_size, int dtype) {
    return evc::prox_masked_learn_workspace_bytes(M, N, T, batch_size, dtype);
}

int evc_prox_masked_learn(const void* X, int ldx, const void* mask, int ldm, void* D, int ldd, void* H, int ldh, void* stats_s,
                          int ld_s, void* stats_q, int ld_q, long long* count_io, const int* order, int M, int N, int T,
                          const evc_prox_masked_learn_opts* opts, void* workspace, size_t workspace_bytes, int* n_epochs_out,
                          int* n_steps_out, double* trace_out, evc_stream_t stream) {
    using namespace evc;
    HIP_TRY(pmlearn_args_check(X, ldx, mask, ldm, D, ldd, H, ldh, stats_s, ld_s, stats_q, ld_q, count_io, order, M, N, T, opts,
                               workspace, workspace_bytes));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (opts->dtype == EVC_F64)
        return prox_masked_learn<double>(static_cast<const double*>(X), ldx, static_cast<const double*>(mask), ldm,
                                         static_cast<double*>(D), ldd, static_cast<double*>(H), ldh, static_cast<double*>(stats_s),
                                         ld_s, static_cast<double*>(stats_q), ld_q, count_io, order, M, N, T, *opts, workspace,
                                         workspace_bytes, n_epochs_out, n_steps_out, trace_out, s);
    return prox_masked_learn<float>(static_cast<const float*>(X), ldx, static_cast<const float*>(mask), ldm,
                                    static_cast<float*>(D), ldd, static_cast<float*>(H), ldh, static_cast<float*>(stats_s), ld_s,
                                    static_cast<float*>(stats_q), ld_q, count_io, order, M, N, T, *opts, workspace,
                                    workspace_bytes, n_epochs_out, n_steps_out, trace_out, s);
}

}  // extern "C"
