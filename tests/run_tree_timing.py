#!/usr/bin/env python3
"""Timing of the joins of pangene tree on the GPU.  Not a test: prints one JSON line per measurement.

    python3 tests/run_tree_timing.py [--device-only] [--no-checker] [--sizes 2000,10000] [--out FILE]

Shapes: A = 2 000 and A = 10 000 assemblies over M = 5 000 items, lineage-structured (tests/support/tree_ref.py), jaccard distances in
fixed point; methods nj and upgma.  Per shape and method: the wall time of pga_pan_join (the backend entry: upload of the A x A
matrix, 2 launches per join, download of the records; median of 3 after a warm-up call), of capi.pan_join in the product (adds the
symmetry and range checks of tree.cpp and the copy into the caller's array) and in the checker build (the host loops of tree.cpp, one
core; past A = 4 000 it is stopped after 500 joins and scaled by the pairs searched, and the line says so).  The bytes the search
kernel has to read -- r (r - 1) / 2 int32 per join, summed over the joins -- are printed beside the bandwidth the copy kernel
reaches in this process (copy_gbps, read + write), so that its kernel time from rocprofv3 gives its share of that.  --device-only
runs the pga_pan_join calls alone (for rocprofv3 --kernel-trace --stats)."""
import argparse, ctypes as C, json, os, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import dist_ref as dr  # noqa: E402
import tree_ref as tr  # noqa: E402

M_ITEMS = 5000
CHECKER_FULL_MAX = 4000
CHECKER_JOINS = 500


class pga_join_in_t(C.Structure):
    _fields_ = [("q", C.c_void_p), ("n", C.c_int32), ("method", C.c_int32)]


class pga_join_out_t(C.Structure):
    _fields_ = [("rec", C.c_void_p), ("n_rec", C.c_int32)]


def med(f, reps=3):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts)


def entry_time(lib, q, method):
    cin, cout = pga_join_in_t(q.ctypes.data, q.shape[0], method), pga_join_out_t()
    fn = lib.pga_pan_join
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(pga_join_in_t), C.POINTER(pga_join_out_t)]

    def call():
        if fn(C.byref(cin), C.byref(cout)) != 0:
            raise RuntimeError("pga_pan_join failed")
    return med(call)


def pairs(A, stop_r):
    """live pairs searched by the joins from r = A down to r = stop_r + 1"""
    return sum(r * (r - 1) // 2 for r in range(stop_r + 1, A + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--no-checker", action="store_true")
    ap.add_argument("--sizes", default="2000,10000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.init()
    hip = capi.load()
    copy_gbps = hip.pg_device_copy_gbps(1 << 30, 5)
    res = []
    for A in (int(x) for x in a.sizes.split(",")):
        P = tr.lineage_presence(M_ITEMS, A, 7)
        q = tr.fixed(capi.pan_shared(hip, P), "jaccard")[0].astype(np.int32)
        for mi, method in enumerate(tr.METHODS):
            n_join = A - 3 if method == "nj" else A - 1
            n_pair = pairs(A, A - n_join)
            r = {"A": A, "M": M_ITEMS, "method": method, "joins": n_join, "launches": 1 + 2 * n_join + (method == "nj"),
                 "search_bytes": 4 * n_pair, "copy_gbps": round(copy_gbps, 1), "entry_wall_ms": round(entry_time(hip, q, mi) * 1e3, 2)}
            if not a.device_only:
                r["product_pan_join_ms"] = round(med(lambda: capi.pan_join(hip, q, method)) * 1e3, 2)
                if not a.no_checker:
                    import oracle_host
                    ora = oracle_host.load()
                    if A <= CHECKER_FULL_MAX:
                        t = time.perf_counter()
                        rec = capi.pan_join(ora, q, method)
                        r["checker_host_loops_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                        r["same"] = bool(np.array_equal(capi.pan_join(hip, q, method), rec))
                    else:
                        os.environ["PANGENE_TREE_STOP_AFTER"] = str(CHECKER_JOINS)
                        t = time.perf_counter()
                        try:
                            capi.pan_join(ora, q, method)
                        except RuntimeError:
                            pass
                        t = time.perf_counter() - t
                        del os.environ["PANGENE_TREE_STOP_AFTER"]
                        r["checker_host_loops_ms"] = round(t * 1e3 * n_pair / pairs(A, A - CHECKER_JOINS), 1)
                        r["checker_scaled_from_joins"] = CHECKER_JOINS
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
