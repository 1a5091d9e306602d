// MFCC alignment features (evc_mfcc): librosa.feature.mfcc(y, sr, n_fft, hop_length) as called at
// 01_make_dict_parallel.py:96-104 - the features the DTW of the dictionary build runs on.  librosa is absent here, so
// its published chain is restated (parity with the package is unpinned): STFT power -> Slaney mel filterbank ->
// 10 log10 with the per-utterance top_db clamp -> orthonormal DCT-II.  float64.
//
// A call takes a batch of utterances.  They are laid out as ONE virtual signal, the way a Griffin-Lim batch is
// (evc_gl.hip): utterance u is reflect-padded on its own and placed at sample hop * rv[u], so that the frames of all
// utterances are rows of one strided matrix (row stride hop) and S = frames W_f is one contraction on the fp64 matrix
// cores (gemm_nt, table of k_gl_tables).  rv[u + 1] = round_up(rv[u] + T_u + ceil(F / hop), MFCC_RB): the rows between
// two utterances straddle both signals and nobody reads their results, and because every utterance starts at a multiple
// of MFCC_RB rows a workgroup of the two kernels below (MFCC_RB rows each) never spans two utterances.
//
//   k_mfcc_offsets  frame offsets and virtual rows of the utterances from the caller's sample offsets (one workgroup)
//   k_mfcc_tables   mel filterbank, row-compressed (first bin, bin count, weights per filter), and the DCT basis
//   k_mfcc_pad      the virtual signal
//   per chunk of MFCC_CHUNK rows:  gemm_nt (S = frames W_f, possibly as k-slabs), then
//   k_mfcc_mel      slabs summed in order -> power -> sparse mel sums in ascending bin order -> dB; one partial maximum
//                   per workgroup; optionally re / im to the caller
//   k_mfcc_dct      utterance maximum from that utterance's partial maxima (no atomics, no host read), clamp, DCT with
//                   the basis in LDS
// The number of launches does not depend on the number of utterances, only on the number of row chunks.
#include "evc_internal.h"

namespace evc {

constexpr int MFCC_RB = 32;           // virtual rows per workgroup of k_mfcc_mel / k_mfcc_dct; utterances start at multiples
constexpr int MFCC_QC = 32;           // rows of the DCT basis in LDS at a time
constexpr int MFCC_CHUNK = 8192;      // rows of S per contraction (a multiple of 128)
constexpr int MFCC_MAX_MELS = EVC_MFCC_MAX_MELS;   // (MFCC_QC + MFCC_RB) x (n_mels + 1) doubles of LDS: 128.5 KiB of 160
// (EVC_MFCC_MAX_FFT, checked by mfcc_check: 4 x (fft_size / 2 + 1) doubles of LDS, 128 KiB)

struct MfccDims {
    int F, hop, nb, K1, J1, pad;   // fft size, hop, bins, padded extents of the contraction, reflect padding
    int n_mels, n_mfcc, G;         // G: gap rows ceil(F / hop)
    bool center;
};

static MfccDims mfcc_dims(const evc_mfcc_opts& o) {
    MfccDims d;
    d.F = o.fft_size; d.hop = o.hop; d.nb = o.fft_size / 2 + 1;
    d.K1 = round_up(d.F, 16);
    d.J1 = round_up(2 * d.nb, 64);
    d.center = o.center != 0;
    d.pad = d.center ? d.F / 2 : 0;
    d.n_mels = o.n_mels; d.n_mfcc = o.n_mfcc;
    d.G = (d.F + d.hop - 1) / d.hop;
    return d;
}

__host__ __device__ __forceinline__ long mfcc_frames(long L, int F, int hop, bool center) {
    if (L < 1) return 0;
    if (center) return 1 + L / hop;
    return L < F ? 0 : 1 + (L - F) / hop;
}

// virtual rows of the whole batch; -1: more than the int row indices hold
static long mfcc_rows(const long* soff, int n_utt, const MfccDims& d, long* frames_out) {
    long rv = 0, fr = 0;
    for (int u = 0; u < n_utt; ++u) {
        const long T_ = mfcc_frames(soff[u + 1] - soff[u], d.F, d.hop, d.center);
        fr += T_;
        rv = (rv + T_ + d.G + MFCC_RB - 1) / MFCC_RB * MFCC_RB;
        if (rv > (1L << 30)) return -1;
    }
    if (frames_out) *frames_out = fr;
    return rv;
}

// foff[u] = first output row of utterance u, rv[u] = its first virtual row (n_utt + 1 entries each); one workgroup:
// every thread sums a contiguous range of utterances, thread 0 scans the 256 sums
__global__ __launch_bounds__(256) void k_mfcc_offsets(const long* __restrict__ soff, int n_utt, MfccDims d,
                                                      int* __restrict__ foff, int* __restrict__ rv) {
    __shared__ long sf[256], sr[256];
    const int per = (n_utt + 255) / 256, u0 = threadIdx.x * per, u1 = min(u0 + per, n_utt);
    long f = 0, r = 0;
    for (int u = u0; u < u1; ++u) {
        const long T_ = mfcc_frames(soff[u + 1] - soff[u], d.F, d.hop, d.center);
        f += T_;
        r += (T_ + d.G + MFCC_RB - 1) / MFCC_RB * MFCC_RB;      // r stays a multiple of MFCC_RB
    }
    sf[threadIdx.x] = f;
    sr[threadIdx.x] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        long af = 0, ar = 0;
        for (int i = 0; i < 256; ++i) {
            const long tf = sf[i], tr = sr[i];
            sf[i] = af; sr[i] = ar;
            af += tf; ar += tr;
        }
        foff[n_utt] = (int)af;
        rv[n_utt] = (int)ar;
    }
    __syncthreads();
    f = sf[threadIdx.x];
    r = sr[threadIdx.x];
    for (int u = u0; u < u1; ++u) {
        const long T_ = mfcc_frames(soff[u + 1] - soff[u], d.F, d.hop, d.center);
        foff[u] = (int)f;
        rv[u] = (int)r;
        f += T_;
        r += (T_ + d.G + MFCC_RB - 1) / MFCC_RB * MFCC_RB;
    }
}

// the utterance whose rows start at or before virtual row r (rv ascending, rv[0] = 0)
__device__ __forceinline__ int mfcc_utt_of_row(const int* __restrict__ rv, int n_utt, long r) {
    int lo = 0, hi = n_utt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long)rv[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Slaney scale: linear below 1000 Hz (200/3 Hz per mel), logarithmic above (27 mels per factor 6.4)
__device__ __forceinline__ double mfcc_hz_to_mel(double f) {
    const double f_sp = 200.0 / 3.0;
    return f < 1000.0 ? f / f_sp : 15.0 + log(f / 1000.0) / (log(6.4) / 27.0);
}
__device__ __forceinline__ double mfcc_mel_to_hz(double m) {
    const double f_sp = 200.0 / 3.0, m0 = 15.0;
    return m < m0 ? f_sp * m : 1000.0 * exp(log(6.4) / 27.0 * (m - m0));
}

// np.linspace(lo, hi, n)[i]
__device__ __forceinline__ double mfcc_linspace(double lo, double hi, int n, int i) {
    if (n > 1 && i == n - 1) return hi;
    return n > 1 ? (double)i * ((hi - lo) / (double)(n - 1)) + lo : lo;
}

// weight of bin k in filter i (before the area normalisation)
__device__ __forceinline__ double mfcc_weight(const double* melf, int i, double fk) {
    const double lower = (fk - melf[i]) / (melf[i + 1] - melf[i]);
    const double upper = (melf[i + 2] - fk) / (melf[i + 2] - melf[i + 1]);
    return fmax(0.0, fmin(lower, upper));
}

// One workgroup.  mk0[i] / mcnt[i] / moff[i]: first bin, bin count and first weight of filter i (a filter's non-zero
// weights are the contiguous bins strictly inside (mel_f[i], mel_f[i + 2]); a bin lies inside at most two filters, so
// there are at most 2 nb weights); basis[q][n] = s_q cos(pi q (2 n + 1) / (2 n_mels))
__global__ __launch_bounds__(256) void k_mfcc_tables(MfccDims d, double sr, double fmin_, double fmax_,
                                                     int* __restrict__ mk0, int* __restrict__ mcnt,
                                                     int* __restrict__ moff, double* __restrict__ mw,
                                                     double* __restrict__ basis) {
    __shared__ double melf[MFCC_MAX_MELS + 2];
    __shared__ int s_k0[MFCC_MAX_MELS], s_cnt[MFCC_MAX_MELS], s_off[MFCC_MAX_MELS];
    const int nm = d.n_mels;
    const double mlo = mfcc_hz_to_mel(fmin_), mhi = mfcc_hz_to_mel(fmax_);
    for (int i = threadIdx.x; i < nm + 2; i += 256) melf[i] = mfcc_mel_to_hz(mfcc_linspace(mlo, mhi, nm + 2, i));
    __syncthreads();
    for (int i = threadIdx.x; i < nm; i += 256) {
        int k0 = 0, cnt = 0;
        for (int k = 0; k < d.nb; ++k) {
            if (mfcc_weight(melf, i, mfcc_linspace(0.0, 0.5 * sr, d.nb, k)) > 0.0) {
                if (cnt == 0) k0 = k;
                cnt = k - k0 + 1;
            }
        }
        s_k0[i] = k0;
        s_cnt[i] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int i = 0; i < nm; ++i) {
            // never past the 2 nb weights the workspace holds (not reachable with 0 <= fmin < fmax: see above)
            if (acc + s_cnt[i] > 2 * d.nb) s_cnt[i] = 2 * d.nb - acc;
            s_off[i] = acc;
            acc += s_cnt[i];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nm; i += 256) {
        const double enorm = 2.0 / (melf[i + 2] - melf[i]);
        for (int j = 0; j < s_cnt[i]; ++j)
            mw[s_off[i] + j] = mfcc_weight(melf, i, mfcc_linspace(0.0, 0.5 * sr, d.nb, s_k0[i] + j)) * enorm;
        mk0[i] = s_k0[i];
        mcnt[i] = s_cnt[i];
        moff[i] = s_off[i];
    }
    for (int g = threadIdx.x; g < d.n_mfcc * nm; g += 256) {
        const int q = g / nm, n = g % nm;
        const long a = ((long)q * (2 * n + 1)) % (4L * nm);       // exact argument reduction (period 4 n_mels)
        basis[g] = sqrt((q == 0 ? 1.0 : 2.0) / (double)nm) * cospi((double)a / (double)(2 * nm));
    }
}

// xv[i]: utterance u's reflect-padded signal from sample hop rv[u] on (numpy 'reflect': the edge sample is not
// repeated), zero between the utterances and beyond (the gap rows and the padded rows of the contraction read it)
__global__ __launch_bounds__(256) void k_mfcc_pad(const double* __restrict__ x, const long* __restrict__ soff,
                                                  const int* __restrict__ foff, const int* __restrict__ rv, int n_utt,
                                                  MfccDims d, long Lv, double* __restrict__ xv) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Lv) return;
    const int u = mfcc_utt_of_row(rv, n_utt, i / d.hop);
    const long j = i - (long)rv[u] * d.hop, L = soff[u + 1] - soff[u];
    double v = 0.0;
    if (foff[u + 1] > foff[u] && j < L + 2L * d.pad) {
        long s = j - d.pad;
        if (L == 1) s = 0;
        else {
            const long period = 2 * (L - 1);
            s %= period;
            if (s < 0) s += period;
            if (s >= L) s = period - s;
        }
        v = x[soff[u] + s];
    }
    xv[i] = v;
}

// One workgroup per MFCC_RB virtual rows from row r0 on, one wavefront per row at a time.  S holds the chunk's rows
// ([Re | Im] per row, row stride lds_), possibly as `splits` k-slabs that are summed here in order (as k_stft_split does).
// dynamic LDS: 4 x nb doubles (the power spectrum of each wavefront's row)
__global__ __launch_bounds__(256) void k_mfcc_mel(const double* __restrict__ S, int lds_, long slab, int splits, int r0,
                                                  const int* __restrict__ foff, const int* __restrict__ rv, int n_utt,
                                                  MfccDims d, const int* __restrict__ mk0, const int* __restrict__ mcnt,
                                                  const int* __restrict__ moff, const double* __restrict__ mw,
                                                  double amin, double* __restrict__ dB, double* __restrict__ pmax,
                                                  double* __restrict__ re, long ldre, double* __restrict__ im, long ldim) {
    extern __shared__ __attribute__((aligned(16))) double s_pow[];     // [4][nb]
    __shared__ double s_red[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long rb = (long)r0 + (long)blockIdx.x * MFCC_RB;              // first virtual row of this workgroup
    const int u = mfcc_utt_of_row(rv, n_utt, rb);
    const long T_ = foff[u + 1] - foff[u], t0 = rb - rv[u];             // rows t0 .. of utterance u; valid while < T_
    double* pw = s_pow + (size_t)wave * d.nb;
    double wmax = -INFINITY;
    for (int it = 0; it < MFCC_RB / 4; ++it) {
        const int lr = it * 4 + wave;                                   // row within the workgroup
        const bool valid = t0 + lr < T_;
        if (valid) {
            const double* row = S + ((long)blockIdx.x * MFCC_RB + lr) * lds_;
            const long orow = (long)foff[u] + t0 + lr;
            for (int k = lane; k < d.nb; k += 64) {
                double r = row[k], i = row[d.nb + k];
                for (int z = 1; z < splits; ++z) {
                    r += row[z * slab + k];
                    i += row[z * slab + d.nb + k];
                }
                pw[k] = r * r + i * i;
                if (re) re[orow * ldre + k] = r;
                if (im) im[orow * ldim + k] = i;
            }
        }
        __syncthreads();
        if (valid) {
            for (int f = lane; f < d.n_mels; f += 64) {
                const int k0 = mk0[f], cnt = mcnt[f];
                const double* w = mw + moff[f];
                double acc = 0.0;
                for (int j = 0; j < cnt; ++j) acc += pw[k0 + j] * w[j];
                const double db = 10.0 * log10(fmax(amin, acc));
                dB[(rb + lr) * d.n_mels + f] = db;
                wmax = fmax(wmax, db);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) wmax = fmax(wmax, __shfl_down(wmax, o, 64));
    if (lane == 0) s_red[wave] = wmax;
    __syncthreads();
    if (threadIdx.x == 0) pmax[rb / MFCC_RB] = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
}

// One workgroup per MFCC_RB virtual rows.  dynamic LDS: (MFCC_QC + MFCC_RB) x (n_mels + 1) doubles - MFCC_QC rows of the
// basis at a time (all of them for n_mfcc <= MFCC_QC) and the clamped dB tile; rows padded by one double against bank
// conflicts.  out[foff[u] + t][q] = sum_n max(dB[t][n], max_u - top_db) basis[q][n], summed in ascending n
__global__ __launch_bounds__(256) void k_mfcc_dct(const double* __restrict__ dB, const double* __restrict__ pmax,
                                                  const int* __restrict__ foff, const int* __restrict__ rv, int n_utt,
                                                  MfccDims d, const double* __restrict__ basis, double top_db,
                                                  double* __restrict__ out, long ldc) {
    extern __shared__ __attribute__((aligned(16))) double s_dct[];
    __shared__ double s_red[4];
    const int nm = d.n_mels, ldl = nm + 1;
    const long rb = (long)blockIdx.x * MFCC_RB;
    const int u = mfcc_utt_of_row(rv, n_utt, rb);
    const long T_ = foff[u + 1] - foff[u], t0 = rb - rv[u];
    if (t0 >= T_) return;                                               // gap rows only (uniform: before any barrier)
    const int nvalid = (int)(T_ - t0 < MFCC_RB ? T_ - t0 : MFCC_RB);
    // the utterance's maximum: max is exact, so the order of the partial maxima does not matter
    double m = -INFINITY;
    const long pb0 = rv[u] / MFCC_RB, pb1 = (rv[u] + T_ + MFCC_RB - 1) / MFCC_RB;
    for (long p = pb0 + threadIdx.x; p < pb1; p += 256) m = fmax(m, pmax[p]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_down(m, o, 64));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmax(fmax(s_red[0], s_red[1]), fmax(s_red[2], s_red[3]));
    const double floor_ = top_db >= 0.0 ? m - top_db : -INFINITY;
    double* s_b = s_dct;                                                // [MFCC_QC][ldl]
    double* s_x = s_dct + (size_t)MFCC_QC * ldl;                        // [MFCC_RB][ldl]
    for (int g = threadIdx.x; g < nvalid * nm; g += 256) {
        const int t = g / nm, n = g % nm;
        s_x[t * ldl + n] = fmax(dB[(rb + t) * nm + n], floor_);
    }
    for (int q0 = 0; q0 < d.n_mfcc; q0 += MFCC_QC) {
        const int qc = d.n_mfcc - q0 < MFCC_QC ? d.n_mfcc - q0 : MFCC_QC;
        __syncthreads();                                                // the previous chunk's reads (and s_x) are done
        for (int g = threadIdx.x; g < qc * nm; g += 256) s_b[(g / nm) * ldl + g % nm] = basis[(long)q0 * nm + g];
        __syncthreads();
        for (int g = threadIdx.x; g < nvalid * qc; g += 256) {
            const int t = g / qc, q = g % qc;
            const double* b = s_b + q * ldl;
            const double* xr = s_x + t * ldl;
            double acc = 0.0;
            for (int n = 0; n < nm; ++n) acc += xr[n] * b[n];
            out[((long)foff[u] + t0 + t) * ldc + q0 + q] = acc;
        }
    }
}

// ---- host side ----

struct MfccPlan {
    long R, frames;          // virtual rows (a multiple of MFCC_RB), output frames
    long Rp, Lv;             // rows padded to the contraction's 128, samples of the virtual signal
    int Ic;                  // rows of the largest chunk (padded)
    size_t nsplit;           // elements of the split-K slabs
};

static bool mfcc_plan(const long* soff, int n_utt, const MfccDims& d, MfccPlan* p) {
    p->R = mfcc_rows(soff, n_utt, d, &p->frames);
    if (p->R < 0 || p->frames > (1L << 30)) return false;
    p->Rp = (p->R + 127) / 128 * 128;
    p->Lv = ((long)d.hop * (p->Rp - 1) + d.K1 + 15) & ~15L;
    p->Ic = (int)(p->Rp < MFCC_CHUNK ? p->Rp : MFCC_CHUNK);
    // gemm_nt splits a contraction over k only while it has fewer than 256 blocks of 128 x 64 outputs, into at most
    // 8 slabs: room for 8 slabs of the tallest such chunk, whatever the batch (< 8 * 256 * 128 * 64 doubles = 128 MiB)
    long rs = (long)(255 / (d.J1 / 64)) * 128;
    if (rs > p->Ic) rs = p->Ic;
    p->nsplit = 8 * (size_t)rs * d.J1;
    return true;
}

static size_t al32(size_t n) { return (n + 31) & ~size_t(31); }

static size_t mfcc_workspace_bytes(const long* soff, int n_utt, const evc_mfcc_opts& o) {
    const MfccDims d = mfcc_dims(o);
    MfccPlan p;
    if (!mfcc_plan(soff, n_utt, d, &p)) return 0;
    if (p.frames == 0) return 256;
    const size_t n = al32((size_t)d.J1 * d.K1) + al32((size_t)p.Ic * d.J1) + al32(p.nsplit) + al32((size_t)p.Lv)
                   + al32((size_t)p.R * d.n_mels) + al32((size_t)(p.R / MFCC_RB))
                   + al32(2 * (size_t)d.nb) + al32((size_t)d.n_mfcc * d.n_mels)
                   + al32((size_t)n_utt + 1)                                       // sample offsets (longs)
                   + al32(((size_t)n_utt + 2) / 2) * 2 + al32(((size_t)d.n_mels + 1) / 2) * 3;   // int tables
    return n * sizeof(double) + 256;
}

static bool mfcc_has_frames(const long* soff, int n_utt, const evc_mfcc_opts& o) {
    long frames = 0;
    return mfcc_rows(soff, n_utt, mfcc_dims(o), &frames) > 0 && frames > 0;
}

static hipError_t mfcc_run(const double* x, const long* soff, int n_utt, const evc_mfcc_opts& o, double* out, long ldc,
                           double* re, long ldre, double* im, long ldim, void* ws, hipStream_t s) {
    const MfccDims d = mfcc_dims(o);
    MfccPlan pl;
    if (!mfcc_plan(soff, n_utt, d, &pl)) return hipErrorInvalidValue;
    double* p = reinterpret_cast<double*>(((uintptr_t)ws + 255) & ~uintptr_t(255));
    auto take = [&](size_t n) { double* q = p; p += al32(n); return q; };
    double* Wf = take((size_t)d.J1 * d.K1);
    double* S = take((size_t)pl.Ic * d.J1);
    double* split = take(pl.nsplit);
    double* xv = take((size_t)pl.Lv);
    double* dB = take((size_t)pl.R * d.n_mels);
    double* pmax = take((size_t)(pl.R / MFCC_RB));
    double* mw = take(2 * (size_t)d.nb);
    double* basis = take((size_t)d.n_mfcc * d.n_mels);
    long* dsoff = reinterpret_cast<long*>(take((size_t)n_utt + 1));
    int* foff = reinterpret_cast<int*>(take(((size_t)n_utt + 2) / 2));
    int* rv = reinterpret_cast<int*>(take(((size_t)n_utt + 2) / 2));
    int* mk0 = reinterpret_cast<int*>(take(((size_t)d.n_mels + 1) / 2));
    int* mcnt = reinterpret_cast<int*>(take(((size_t)d.n_mels + 1) / 2));
    int* moff = reinterpret_cast<int*>(take(((size_t)d.n_mels + 1) / 2));

    // the caller keeps sample_offsets valid until the call returns (include/evc.h); HIP stages a pageable source
    // before hipMemcpyAsync returns
    hipError_t e = hipMemcpyAsync(dsoff, soff, sizeof(long) * ((size_t)n_utt + 1), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_mfcc_offsets, dim3(1), dim3(256), 0, s, dsoff, n_utt, d, foff, rv);
    e = stft_forward_table(d.F, d.hop, Wf, s);
    if (e != hipSuccess) return e;
    const double sr = (double)o.sr, fmax_ = o.fmax == 0.0 ? 0.5 * sr : o.fmax;
    hipLaunchKernelGGL(k_mfcc_tables, dim3(1), dim3(256), 0, s, d, sr, o.fmin, fmax_, mk0, mcnt, moff, mw, basis);
    hipLaunchKernelGGL(k_mfcc_pad, dim3((unsigned)((pl.Lv + 255) / 256)), dim3(256), 0, s, x, dsoff, foff, rv, n_utt, d,
                       pl.Lv, xv);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t lds_mel = 4 * (size_t)d.nb * sizeof(double);
    const size_t lds_dct = (size_t)(MFCC_QC + MFCC_RB) * (d.n_mels + 1) * sizeof(double);
    if (lds_mel > 64 * 1024) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mfcc_mel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_mel);
        if (e != hipSuccess) return e;
    }
    if (lds_dct > 64 * 1024) {
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_mfcc_dct), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_dct);
        if (e != hipSuccess) return e;
    }
    for (long r0 = 0; r0 < pl.R; r0 += MFCC_CHUNK) {
        const long rows = pl.R - r0 < MFCC_CHUNK ? pl.R - r0 : MFCC_CHUNK;     // a multiple of MFCC_RB
        const int Ic = (int)((rows + 127) / 128 * 128);
        int sp = 0;
        e = gemm_nt<double>(xv + r0 * d.hop, d.hop, Wf, d.K1, S, d.J1, Ic, d.J1, d.K1, s, pl.nsplit ? split : nullptr,
                            pl.nsplit, &sp);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_mfcc_mel, dim3((unsigned)(rows / MFCC_RB)), dim3(256), lds_mel, s, sp ? split : S, d.J1,
                           (long)Ic * d.J1, sp ? sp : 1, (int)r0, foff, rv, n_utt, d, mk0, mcnt, moff, mw, o.amin, dB,
                           pmax, re, ldre, im, ldim);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_mfcc_dct, dim3((unsigned)(pl.R / MFCC_RB)), dim3(256), lds_dct, s, dB, pmax, foff, rv, n_utt, d,
                       basis, o.top_db, out, ldc);
    return hipGetLastError();
}

}  // namespace evc

using namespace evc;

// ---- the C entries (include/evc.h) ----
// 0, or the status the options / offsets of an evc_mfcc call earn before anything else is looked at
static int mfcc_check(const long* soff, int n_utt, const evc_mfcc_opts* o) {
    if (!o || o->struct_bytes != (int)sizeof(evc_mfcc_opts) || n_utt < 0) return ST_BADARG;
    if (o->sr < 1 || o->fft_size < 2 || (o->fft_size & 1) || o->hop < 1 || o->n_mels < 1) return ST_BADARG;
    if (o->n_mfcc < 1 || o->n_mfcc > o->n_mels) return ST_BADARG;
    const double fmax_ = o->fmax == 0.0 ? 0.5 * o->sr : o->fmax;
    if (!(o->fmin >= 0.0 && o->fmin < fmax_ && fmax_ <= 0.5 * o->sr) || !(o->amin > 0.0) || o->top_db != o->top_db)
        return ST_BADARG;
    if (n_utt > 0) {
        if (!soff || soff[0] < 0) return ST_BADARG;
        for (int u = 0; u < n_utt; ++u)
            if (soff[u + 1] < soff[u]) return ST_BADARG;
    }
    if (o->n_mels > EVC_MFCC_MAX_MELS || o->fft_size > EVC_MFCC_MAX_FFT) return ST_UNSUPPORTED;
    return ST_OK;
}

extern "C" {

size_t evc_mfcc_workspace_bytes(const long* sample_offsets, int n_utt, const evc_mfcc_opts* opts) {
    if (mfcc_check(sample_offsets, n_utt, opts) != ST_OK || n_utt < 1) return 0;
    return mfcc_workspace_bytes(sample_offsets, n_utt, *opts);
}

int evc_mfcc(const void* x, const long* sample_offsets, int n_utt, const evc_mfcc_opts* opts, void* mfcc, int ldc,
             void* re, int ldre, void* im, int ldim, void* workspace, size_t workspace_bytes, evc_stream_t stream) {
    const int st = mfcc_check(sample_offsets, n_utt, opts);
    if (st != ST_OK) return st;
    const int nb = opts->fft_size / 2 + 1;
    if (ldc < opts->n_mfcc || (re && ldre < nb) || (im && ldim < nb)) return ST_BADARG;
    if (n_utt == 0 || !mfcc_has_frames(sample_offsets, n_utt, *opts)) return ST_OK;
    if (!x || !mfcc || !workspace) return ST_BADARG;
    const size_t need = mfcc_workspace_bytes(sample_offsets, n_utt, *opts);
    if (need == 0) return ST_BADARG;                            // more rows than the int indices hold
    if (workspace_bytes < need) return ST_WORKSPACE;
    return (int)mfcc_run(static_cast<const double*>(x), sample_offsets, n_utt, *opts, static_cast<double*>(mfcc), ldc,
                         static_cast<double*>(re), ldre, static_cast<double*>(im), ldim, workspace,
                         reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
