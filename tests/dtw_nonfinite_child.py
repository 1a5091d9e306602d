"""Child process of test_gpu_dtw_tiles.py::test_nonfinite_features_are_safe: runs evc_dtw_align on the three-pair batch
of dtw_cases.py, once as it is and once per poisoned middle pair, and writes every call's image and wall time to an
.npz.  A process of its own so that the parent can put a time limit on it; plain ctypes on the HIP runtime the library
links (no torch: the start-up stays short).

    python dtw_nonfinite_child.py OUT.npz
"""
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import dtw_cases as K  # noqa: E402
import dtw_restatement as R  # noqa: E402


def main(out):
    from exemplars_vc_amd import _lib
    L = _lib.lib()
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L.hipFree.argtypes = [C.c_void_p]
    H2D, D2H = 1, 2

    def ok(st, what):
        if st != 0:
            raise RuntimeError(f"{what}: status {st}")

    def up(arr):
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        ok(L.hipMalloc(C.byref(p), max(arr.nbytes, 256)), "hipMalloc")
        ok(L.hipMemcpy(p, arr.ctypes.data, arr.nbytes, H2D), "hipMemcpy")
        return p

    def down(p, like):
        got = np.empty_like(like)
        ok(L.hipMemcpy(got.ctypes.data, p, got.nbytes, D2H), "hipMemcpy")
        return got

    def run(batch):
        cap = int(batch.poff[-1])
        h_pa = np.full(K.GUARD + cap + K.GUARD, K.SENTINEL, dtype=np.int32)
        h_plen = np.full(batch.n, K.SENTINEL, dtype=np.int32)
        h_tot = np.full(batch.n, K.TOTAL_SENTINEL)
        h_ws = np.full(R.workspace_bytes(batch.aoff, batch.boff), 0xA5, dtype=np.uint8)
        bufs = [up(batch.packed("a")), up(batch.packed("b")), up(h_pa), up(h_pa), up(h_plen), up(h_tot), up(h_ws)]
        A, B, pa, pb, plen, tot, ws = bufs
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        ok(L.hipDeviceSynchronize(), "sync")
        t0 = time.perf_counter()
        st = L.evc_dtw_align(A, batch.D, ip(batch.aoff), B, batch.D, ip(batch.boff), batch.D, batch.n,
                             C.c_void_p(pa.value + 4 * K.GUARD), C.c_void_p(pb.value + 4 * K.GUARD), plen,
                             tot, ws, h_ws.nbytes, None)
        ok(st, "evc_dtw_align")
        ok(L.hipDeviceSynchronize(), "sync after evc_dtw_align")
        dt = time.perf_counter() - t0
        img = dict(pa=down(pa, h_pa), pb=down(pb, h_pa), plen=down(plen, h_plen), total=down(tot, h_tot), ws=down(ws, h_ws))
        for p in bufs:
            ok(L.hipFree(p), "hipFree")
        return img, dt

    base = K.three_batch()
    run(base)                                        # (the first launch loads the code object)
    res = {}
    img, dt = run(base)
    res.update({f"finite_{k}": v for k, v in img.items()}, finite_seconds=dt)
    for c, (side, frame, value) in enumerate(K.NONFINITE):
        img, dt = run(K.poisoned(base, side, frame, value))
        res.update({f"case{c}_{k}": v for k, v in img.items()})
        res[f"case{c}_seconds"] = dt
        np.savez(out, **res)                         # (what has run so far survives a time limit)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
