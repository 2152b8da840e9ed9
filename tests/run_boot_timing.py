#!/usr/bin/env python3
"""Timing of the bootstrap of pangene tree on the GPU.  Not a test: prints one JSON line per measurement.

    python3 tests/run_boot_timing.py [--device-only] [--no-checker] [--sizes 2000,10000] [--out FILE]

Shapes: A = 2 000 and A = 10 000 assemblies over M = 5 000 items, lineage-structured (tests/support/tree_ref.py), jaccard; methods nj
and upgma; B = pga_boot_batch(A) replicates, one call's worth.  Per shape and method: the wall time of pga_pan_boot (the backend entry:
upload of the bit rows, draws, resampling, counts, distances, the batched joins, download of the records; median of 3 after a warm-up
call) and the same per replicate, beside the wall of pga_pan_join on the reference matrix (join_entry_wall_ms: the single-tree kernels,
whose wall is the sum of their kernel times -- what a loop over them on device-resident q_b would pay per replicate, plus the upload of
one matrix) and the wall of one replicate alone (boot_one_replicate_wall_ms, n_rep = 1: that includes the upload, the draws, the rows,
the counts and the distances, so it is NOT the loop's figure; the batched joins are compared with join_entry_wall_ms, by the kernel
times of k_join_*_b per replicate from rocprofv3).  The bytes the batched search has to read -- B times r (r - 1) / 2 int32 per
join, summed over the joins -- are printed beside the bandwidth the copy kernel reaches in this process (copy_gbps, read + write), so
that the search's kernel time from rocprofv3 gives its share of that.  The checker build (host loops of tree.cpp, one core) is timed on
one replicate, past A = 4 000 on its first 500 joins and scaled by the pairs searched.  --device-only runs the pga_pan_boot calls alone
(for rocprofv3 --kernel-trace --stats)."""
import argparse, ctypes as C, json, os, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import boot_direct as bd  # noqa: E402
import tree_ref as tr  # noqa: E402
from run_tree_timing import entry_time, pairs, M_ITEMS, CHECKER_FULL_MAX, CHECKER_JOINS  # noqa: E402


def med(f, reps=3):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts)


def boot_time(lib, bits, M, A, method, n_rep):
    cin = bd.pga_boot_in_t(bits.ctypes.data, M, A, 0, method, 11, 1, n_rep, None)
    cout = bd.pga_boot_out_t()
    fn = lib.pga_pan_boot
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(bd.pga_boot_in_t), C.POINTER(bd.pga_boot_out_t)]

    def call():
        if fn(C.byref(cin), C.byref(cout)) != 0:
            raise RuntimeError("pga_pan_boot failed")
    return med(call)


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
        bits = bd.bit_rows(P)
        B = bd.batch(hip, A)
        q = None if a.device_only else tr.fixed(capi.pan_shared(hip, P), "jaccard")[0].astype(np.int32)
        for mi, method in enumerate(tr.METHODS):
            n_join = A - 3 if method == "nj" else A - 1
            n_pair = pairs(A, A - n_join)
            wall = boot_time(hip, bits, M_ITEMS, A, mi, B)
            r = {"A": A, "M": M_ITEMS, "method": method, "B": B, "joins": n_join, "launches": 1 + 2 * n_join + (method == "nj"),
                 "search_bytes": 4 * n_pair * B, "copy_gbps": round(copy_gbps, 1), "boot_wall_ms": round(wall * 1e3, 2),
                 "boot_wall_per_replicate_ms": round(wall * 1e3 / B, 3)}
            if not a.device_only:
                r["boot_one_replicate_wall_ms"] = round(boot_time(hip, bits, M_ITEMS, A, mi, 1) * 1e3, 2)
                r["join_entry_wall_ms"] = round(entry_time(hip, q, mi) * 1e3, 2)
                if not a.no_checker:
                    import oracle_host
                    ora = oracle_host.load()
                    if A > CHECKER_FULL_MAX:
                        os.environ["PANGENE_TREE_STOP_AFTER"] = str(CHECKER_JOINS)
                    t = time.perf_counter()
                    try:
                        capi.pan_boot_records(ora, P, "jaccard", method, seed=11, first=1, n=1)
                    except RuntimeError:
                        pass
                    t = time.perf_counter() - t
                    if A > CHECKER_FULL_MAX:
                        del os.environ["PANGENE_TREE_STOP_AFTER"]
                        # (the draws, rows, counts and distances before the joins are not scaled: they are timed in full)
                        r["checker_scaled_from_joins"] = CHECKER_JOINS
                        os.environ["PANGENE_TREE_STOP_AFTER"] = "1"
                        t0 = time.perf_counter()
                        try:
                            capi.pan_boot_records(ora, P, "jaccard", method, seed=11, first=1, n=1)
                        except RuntimeError:
                            pass
                        t0 = time.perf_counter() - t0
                        del os.environ["PANGENE_TREE_STOP_AFTER"]
                        t = t0 + (t - t0) * n_pair / pairs(A, A - CHECKER_JOINS)
                    r["checker_one_replicate_ms"] = round(t * 1e3, 1)
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
