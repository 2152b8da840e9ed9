#!/usr/bin/env python3
"""Timing of the lineage-aware trait test on one MI355X ("Lineage-aware trait test measured").

    python tests/run_pairs_timing.py [--device-only] [--no-checker] [--genes 100000] [--asm 2000,10000] [--out FILE]

Lineage-structured matrices (tree_ref.lineage_presence) of 100 000 genes over A = 2 000 and 10 000 assemblies, one balanced random trait,
nj and upgma.  The tree comes from capi.pan_tree once per shape and method and is timed on its own (tree_ms).  Per shape and method:
the wall time of pga_pan_pairs (the backend entry: packing of the program and the labels, upload, k_pairs, download; median of three
calls after a warm-up) with the program of pairs_ref.program; joins per second = (A - 1) x genes x rows x 2 runs over that wall; the
wall of capi.pan_pairs in the product (adds the tree compiler and the byte-to-bit packing) and in the checker build (the host loops of
trait.cpp on one core, run on a prefix of --checker-genes genes and SCALED, which the output says); tree_share = tree_ms over
tree_ms + the product's capi.pan_pairs wall, the part of `pangene trait -L` the tree itself takes beside the pair counts.
--device-only runs the pga_pan_pairs calls alone (the run to put under rocprofv3 --kernel-trace --stats for the kernel time)."""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import pairs_ref as pr  # noqa: E402
import tree_ref  # noqa: E402
from pairs_direct import bit_rows, pga_pairs_in_t, pga_pairs_out_t  # noqa: E402


def median(f, reps=3, warm=True):
    if warm:
        f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--no-checker", action="store_true")
    ap.add_argument("--genes", type=int, default=100000)
    ap.add_argument("--asm", default="2000,10000")
    ap.add_argument("--checker-genes", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.init()
    hip = capi.load()
    fn = hip.pga_pan_pairs
    fn.restype = C.c_int
    res = []
    for A in [int(x) for x in a.asm.split(",")]:
        G = a.genes
        P = tree_ref.lineage_presence(G, A, 7, founders=8, flip=0.05, dup=0.0)
        y = (np.random.default_rng(5).permutation(A) < A // 2).astype(np.int8)
        for method in ("nj", "upgma"):
            t0 = time.perf_counter()
            rec, _ = capi.pan_tree(hip, P, "jaccard", method)
            t_tree = time.perf_counter() - t0
            kids = pr.tree(rec, A, method)
            op, order, need = pr.program(kids, A)
            bits = np.ascontiguousarray(bit_rows(P)[order])
            lab = np.ascontiguousarray(y[None, order])
            cin, cout = pga_pairs_in_t(op.ctypes.data, bits.ctypes.data, lab.ctypes.data, G, A, 1), pga_pairs_out_t()

            def call():
                if fn(C.byref(cin), C.byref(cout)) != 0:
                    raise RuntimeError("pga_pan_pairs failed")
            t = median(call, a.reps)
            out = np.ctypeslib.as_array(C.cast(cout.out, C.POINTER(C.c_int32)), shape=(G, 3)).copy()
            joins = (A - 1) * G * 2
            r = {"G": G, "A": A, "method": method, "stack_need": need, "tree_ms": round(t_tree * 1e3, 3), "entry_wall_ms": round(t * 1e3, 3),
                 "joins": joins, "joins_per_s": round(joins / t, 0), "sum_pairs": int(out[:, 0].sum())}
            if not a.device_only:
                t_capi = median(lambda: capi.pan_pairs(hip, P, y, rec, method), a.reps, warm=False)
                r["product_capi_pan_pairs_ms"] = round(t_capi * 1e3, 3)
                r["tree_share"] = round(t_tree / (t_tree + t_capi), 3)
                if not a.no_checker:
                    import oracle_host
                    ora = oracle_host.load()
                    g = min(G, a.checker_genes)
                    t0 = time.perf_counter()
                    ref = capi.pan_pairs(ora, P[:g], y, rec, method)
                    t_host = time.perf_counter() - t0
                    r["checker_host_loops_ms"] = round(t_host * 1e3 * (G / g), 1)
                    r["checker_scaled_from_genes"] = g if g != G else None
                    r["same"] = bool(np.array_equal(out[:g, 0], ref["pairs"][0]) and np.array_equal(out[:g, 1], ref["supp"][0]) and np.array_equal(out[:g, 2], ref["opp"][0]))
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
