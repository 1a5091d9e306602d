// evc_transform.hip - evc_online_transform: scikit-learn's MiniBatchNMF.transform, that is MiniBatchNMF._solve_W
// (_nmf.py:2046-2071): multiplicative updates of the activations with the dictionary fixed, checked EVERY iteration against
// ||H_new - H_old||_F / ||H_new||_F <= tol, the stopping update kept.  DESIGN.md §5.13.
//
// One utterance is one transform call: its own start sqrt(mean(X_u) / R), its own ratio, its own stop.  Per iteration two
// launches and no host round trip: the change variant of k_beta_sweep (evc_beta.hip), which stores the same h_new as the
// plain sweep and leaves every frame's shares of the two sums of squares, and k_beta_change_check, which sums an utterance's
// shares in a fixed order, records the ratio and sets stop[u] on the device; the sweeps of a stopped utterance return at once.
// With tol = 0 the activations are bitwise those of evc_beta_solve(EVC_INIT_SKLEARN, the same iters, no checks).
// The argument checks and the workspace carving are host-only code in evc_transform_plan.h, which a stand-alone program runs
// under the host sanitizers (tests/transform_host_main.hip).
#include "evc_transform_plan.h"

namespace evc {

namespace {

// arguments already validated by evc_online_transform; returns ST_OK, ST_WORKSPACE or a hipError_t
template <typename T>
int online_transform(const void* W_, int ldw, const void* X_, int ldx, void* H_, int ldh, int M, int R, int T_,
                     const int* utt_offsets, int n_utt, const evc_transform_opts& o, void* ws, size_t ws_bytes,
                     int* n_iter_out, double* change_out, hipStream_t s) {
    const TrWs w = carve_transform(ws, M, R, T_, n_utt, o.dtype);
    if (w.bytes > ws_bytes) return ST_WORKSPACE;
    const int n_slots = transform_slots(o.max_iter);
    BetaCtx<T> c;
    HIP_TRY(beta_begin<T>(c, static_cast<const T*>(X_), ldx, static_cast<T*>(H_), ldh, M, R, T_, utt_offsets, n_utt, o.layout,
                          o.beta, o.l1, o.l2, 0.0, n_slots, w.beta_ws, w.beta_bytes, s));
    c.a.chg = w.chg;
    HIP_TRY(beta_pack_dict<T>(c, static_cast<const T*>(W_), ldw, s));
    HIP_TRY(beta_start<T>(c, o.init_mode, o.init_value, s));
    if (o.ev_loop_start) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_start), s));
    for (int it = 1; it <= o.max_iter; ++it) HIP_TRY(beta_sweep_change<T>(c, it, o.tol, s));
    if (o.ev_loop_stop) HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(o.ev_loop_stop), s));
    return beta_report<T>(c, o.max_iter, n_iter_out, change_out, o.max_iter, s);     // max_iter = 0: no slot, no trace copy
}

}  // namespace

}  // namespace evc

extern "C" {

size_t evc_online_transform_workspace_bytes(int M, int R, int T, int n_utt, int dtype) {
    return evc::transform_workspace_bytes(M, R, T, n_utt, dtype);
}

int evc_online_transform(const void* W, int ldw, const void* X, int ldx, void* H, int ldh, int M, int R, int T,
                         const int* utt_offsets, int n_utt, const evc_transform_opts* opts, void* workspace,
                         size_t workspace_bytes, int* n_iter_out, double* change_out, evc_stream_t stream) {
    using namespace evc;
    HIP_TRY(transform_args_check(W, ldw, X, ldx, H, ldh, M, R, T, utt_offsets, n_utt, opts, workspace, workspace_bytes));
    const evc_transform_opts& o = *opts;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return (o.dtype == EVC_F64 ? online_transform<double> : online_transform<float>)(
        W, ldw, X, ldx, H, ldh, M, R, T, utt_offsets, n_utt, o, workspace, workspace_bytes, n_iter_out, change_out, s);
}

}  // extern "C"
