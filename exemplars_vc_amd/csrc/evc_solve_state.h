// evc_solve_state.h - the per-utterance stop state of the solves whose stop rule runs on the device (evc_semi_solve,
// evc_prox_solve, evc_prox_masked_solve): the kernel that resets it, the head that stages the utterance
// offsets and launches that kernel, and the read-back of the stop iterations and the trace.  Each translation unit includes
// this file into an unnamed namespace of its own: all get the same device code from the same text.  The kernel keeps the
// name it had in evc_prox_kernels.h.
#pragma once
#include "evc_internal.h"

namespace evc {

namespace {

// stop = 0, trace = NaN, frame_utt[t] = the utterance of frame t (the largest u with offs[u] <= t)
__global__ void k_prox_state(const int* __restrict__ offs, int n_utt, int T_, int n_slots, int* stop, double* trace,
                             int* frame_utt) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_utt) stop[i] = 0;
    if (i < (long)n_utt * n_slots) trace[i] = __builtin_nan("");
    if (i < T_) {
        int lo = 0, hi = n_utt - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (offs[mid] <= i) lo = mid; else hi = mid - 1;
        }
        frame_utt[i] = lo;
    }
}

// The head of a call: utt_offsets (NULL: one utterance, {0, T_}) staged to `offs`, then k_prox_state over the largest of its
// three ranges.  n_utt is the third only without slots and frames: evc_semi_solve always has a slot (n_slots >= 1), so the
// last clamp never moves its grid.
inline int solve_state_head(const int* utt_offsets, int n_utt, int T_, int n_slots, int* offs, int* stop, double* trace,
                            int* frame_utt, hipStream_t s) {
    const int whole[2] = {0, T_};
    HIP_TRY(hipMemcpyAsync(offs, utt_offsets ? utt_offsets : whole, sizeof(int) * ((size_t)n_utt + 1), hipMemcpyHostToDevice, s));
    long n_state = (long)n_utt * n_slots;
    if (n_state < T_) n_state = T_;
    if (n_state < n_utt) n_state = n_utt;
    hipLaunchKernelGGL(k_prox_state, dim3((unsigned)((n_state + 255) / 256)), dim3(256), 0, s, (const int*)offs, n_utt, T_,
                       n_slots, stop, trace, frame_utt);
    return (int)hipGetLastError();
}

// The tail of a call: n_iter_out[u] = the updates applied when utterance u stopped, or `iters`; trace_out = the
// [n_utt][n_slots] statistics (nothing without slots).  Waits for the stream only if the caller reads either.
inline int solve_read_back(const int* stop, const double* trace, int n_utt, int n_slots, int iters, int* n_iter_out,
                           double* trace_out, hipStream_t s) {
    if (!n_iter_out && !(trace_out && n_slots > 0)) return ST_OK;
    int* ni_h = static_cast<int*>(malloc(sizeof(int) * n_utt));
    if (!ni_h) return (int)hipErrorOutOfMemory;
    hipError_t e = hipMemcpyAsync(ni_h, stop, sizeof(int) * n_utt, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && trace_out && n_slots > 0)
        e = hipMemcpyAsync(trace_out, trace, sizeof(double) * n_utt * n_slots, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    for (int u = 0; e == hipSuccess && n_iter_out && u < n_utt; ++u) n_iter_out[u] = ni_h[u] ? ni_h[u] : iters;
    free(ni_h);
    return (int)e;
}

}  // namespace

}  // namespace evc
