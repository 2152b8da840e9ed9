#!/usr/bin/env python3
"""Timing of k-medoids of pangene cluster on the GPU.  Not a test: prints one JSON line per measurement.

    python3 tests/run_cluster_timing.py [--device-only] [--reps N] [--no-checker] [--sizes 2000,10000] [--out FILE]

Shapes: n = 2 000 and n = 10 000 assemblies over 5 000 items, lineage-structured (tests/support/tree_ref.py), jaccard distances in fixed
point, k = 16.  Per shape: the wall time of pga_pan_medoids (the backend entry: upload of the n x n matrix, BUILD, the swap iterations
in chunks, the finish, one download; best of --reps calls after a warm-up call), its iterations (swaps, plus the one that finds no
negative delta) and its host waits -- derived from the iterations, not counted in the entry: one per chunk of iterations and one at
the end --, of capi.pan_medoids in the product (adds the
symmetry and range checks of tree.cpp and the copies into the caller's arrays) and in the checker build (the host loops of tree.cpp, one
core; where an iteration takes long it runs BUILD and CHECKER_ITER iterations and the remaining iterations are scaled from those, and the
line says so).  The bytes the swap kernel reads per iteration -- n x n int32 -- are printed beside the bandwidth the copy kernel reaches
in this process (copy_gbps, read + write), so that its kernel time from rocprofv3 gives its share of that.  --device-only runs the
pga_pan_medoids calls alone (for rocprofv3 --kernel-trace --stats, with --reps 1)."""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import cluster_ref as cr  # noqa: E402
import tree_ref as tr  # noqa: E402

M_ITEMS = 5000
K = 16
BATCH = int(os.environ.get("PANGENE_MEDOIDS_BATCH", "8"))  # iterations the entry queues between two reads of the status
CHECKER_FULL_MAX = 4000
CHECKER_ITER = 2


class pga_medoids_in_t(C.Structure):
    _fields_ = [("q", C.c_void_p), ("n", C.c_int32), ("k", C.c_int32), ("max_iter", C.c_int32)]


class pga_medoids_out_t(C.Structure):
    _fields_ = [("medoid", C.c_void_p), ("label", C.c_void_p), ("dist", C.c_void_p), ("size", C.c_void_p), ("sums", C.c_void_p), ("rec", C.c_void_p),
                ("td", C.c_int64), ("n_rec", C.c_int32), ("n_swap", C.c_int32), ("converged", C.c_int32)]


def best_of(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--no-checker", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="2000,10000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.init()
    hip = capi.load()
    copy_gbps = hip.pg_device_copy_gbps(1 << 30, 5)
    fn = hip.pga_pan_medoids
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(pga_medoids_in_t), C.POINTER(pga_medoids_out_t)]
    res = []
    for n in (int(x) for x in a.sizes.split(",")):
        P = tr.lineage_presence(M_ITEMS, n, 7)
        q = tr.fixed(capi.pan_shared(hip, P), "jaccard")[0].astype(np.int32)
        cin, cout = pga_medoids_in_t(q.ctypes.data, n, K, 1000), pga_medoids_out_t()

        def call():
            if fn(C.byref(cin), C.byref(cout)) != 0:
                raise RuntimeError("pga_pan_medoids failed")
        if a.device_only and a.reps == 1:  # the profiled run: one call a shape, no warm-up
            t = time.perf_counter()
            call()
            wall = time.perf_counter() - t
        else:
            wall = best_of(call, a.reps)
        iters = cout.n_swap + cout.converged
        r = {"n": n, "M": M_ITEMS, "k": K, "swaps": cout.n_swap, "converged": cout.converged, "iterations": iters,
             "host_waits_derived": (iters + BATCH - 1) // BATCH + 1, "swap_bytes_per_iteration": 4 * n * n, "copy_gbps": round(copy_gbps, 1),
             "entry_wall_ms": round(wall * 1e3, 2)}
        if not a.device_only:
            r["product_pan_medoids_ms"] = round(best_of(lambda: capi.pan_medoids(hip, q, K), a.reps) * 1e3, 2)
            if not a.no_checker:
                import oracle_host
                ora = oracle_host.load()
                got = capi.pan_medoids(hip, q, K)
                if n <= CHECKER_FULL_MAX:
                    t = time.perf_counter()
                    want = capi.pan_medoids(ora, q, K)
                    r["checker_host_loops_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                    r["same"] = bool(cr.same(got, want))
                else:  # BUILD + the finish (max_iter = 0), then CHECKER_ITER iterations on top; the other iterations cost as much each
                    t = time.perf_counter()
                    capi.pan_medoids(ora, q, K, max_iter=0)
                    t0 = time.perf_counter() - t
                    t = time.perf_counter()
                    want = capi.pan_medoids(ora, q, K, max_iter=CHECKER_ITER)
                    t1 = time.perf_counter() - t
                    r["checker_host_loops_ms"] = round((t0 + (t1 - t0) / CHECKER_ITER * max(iters, 1)) * 1e3, 1)
                    r["checker_scaled_from_iterations"] = CHECKER_ITER
                    r["same"] = bool(np.array_equal(want["rec"], got["rec"][:len(want["rec"])]))
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
