#!/usr/bin/env python3
"""Timing of pangene gainloss on one MI355X ("Gain and loss measured").

    python tests/run_gainloss_timing.py [--device-only] [--no-checker] [--items 100000] [--asm 2000,10000] [--reps 3] [--out FILE]

Lineage-structured matrices (tree_ref.lineage_presence) of 100 000 items over A = 2 000 and 10 000 assemblies, upgma, g = l = 1.  The tree
comes from capi.pan_tree once per shape and is timed on its own (tree_ms).  Per shape: the wall time of pga_pan_gainloss (the backend
entry: packing of the program, upload, the three kernels chunk by chunk, download; median of --reps calls after a warm-up) with the
program of gainloss_ref.program; node visits per second = items x (2 A - 1) x 2 passes over that wall; the wall of capi.pan_gainloss in
the product (adds the tree compiler, the byte-to-bit packing and the item counts) and in the checker build (the host loops of
pan_gainloss.hpp on one core, run on a prefix of --checker-items items and SCALED, which the output says); tree_share = tree_ms over
tree_ms + the product's capi.pan_gainloss wall, the part of `pangene gainloss` the tree itself takes beside the reconstruction.
--device-only runs the pga_pan_gainloss calls alone (the run to put under rocprofv3 --kernel-trace --stats for the kernels' shares)."""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import gainloss_ref as gr  # noqa: E402
import pairs_ref as pr  # noqa: E402
import tree_ref  # noqa: E402
from gainloss_direct import chunk, pga_gainloss_in_t, pga_gainloss_out_t  # noqa: E402
from pairs_direct import bit_rows  # noqa: E402


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
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--asm", default="2000,10000")
    ap.add_argument("--checker-items", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.init()
    hip = capi.load()
    fn = hip.pga_pan_gainloss
    fn.restype = C.c_int
    res = []
    for A in [int(x) for x in a.asm.split(",")]:
        M = a.items
        P = tree_ref.lineage_presence(M, A, 7, founders=8, flip=0.05, dup=0.0)
        t0 = time.perf_counter()
        rec, _ = capi.pan_tree(hip, P, "jaccard", "upgma")
        t_tree = time.perf_counter() - t0
        kids = pr.tree(rec, A, "upgma")
        op, order, need, node_of, par = gr.program(kids, A)
        bits = np.ascontiguousarray(bit_rows(P)[order])
        cin, cout = pga_gainloss_in_t(op.ctypes.data, bits.ctypes.data, par.ctypes.data, M, A, 1, 1, 0, None), pga_gainloss_out_t()

        def call():
            if fn(C.byref(cin), C.byref(cout)) != 0:
                raise RuntimeError("pga_pan_gainloss failed")
        t = median(call, a.reps, warm=not a.device_only or a.reps > 1)
        gene = np.ctypeslib.as_array(C.cast(cout.gene, C.POINTER(C.c_int32)), shape=(M, 4)).copy()
        visits = M * (2 * A - 1) * 2
        r = {"items": M, "A": A, "stack_need": need, "chunk": chunk(hip, A), "tree_ms": round(t_tree * 1e3, 3), "entry_wall_ms": round(t * 1e3, 3),
             "node_visits": visits, "node_visits_per_s": round(visits / t, 0), "sum_cost": int(gene[:, 0].sum())}
        if not a.device_only:
            t_capi = median(lambda: capi.pan_gainloss(hip, P, rec, "upgma"), a.reps, warm=False)
            r["product_capi_pan_gainloss_ms"] = round(t_capi * 1e3, 3)
            r["tree_share"] = round(t_tree / (t_tree + t_capi), 3)
            if not a.no_checker:
                import oracle_host
                ora = oracle_host.load()
                m = min(M, a.checker_items)
                t0 = time.perf_counter()
                ref = capi.pan_gainloss(ora, P[:m], rec, "upgma")
                t_host = time.perf_counter() - t0
                r["checker_host_loops_ms"] = round(t_host * 1e3 * (M / m), 1)
                r["checker_scaled_from_items"] = m if m != M else None
                r["same"] = bool(np.array_equal(gene[:m, 0], ref["cost"]) and np.array_equal(gene[:m, 1], ref["gains"]) and np.array_equal(gene[:m, 2], ref["losses"])
                                 and np.array_equal(gene[:m, 3], ref["root"]))
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
