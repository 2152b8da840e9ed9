#!/usr/bin/env python3
"""Timing of pangene coevo on one MI355X ("Co-evolution measured").

    python tests/run_coevo_timing.py [--device-only] [--no-checker] [--items 100000] [--asm 2000,10000] [--reps 3] [--out FILE]

A U-shaped presence model, so that the eligible items are few among all: a tenth of the items are accessory and lineage-structured
(tree_ref.lineage_presence, 8 founders, flip 0.02: many events each), the others are core or rare (present everywhere or nowhere but for
flips at a rate of 0.2 / A per cell: most have no event or one and stay below -c 2).  upgma over jaccard, g = l = 1, late, -r 0.8 -c 2.  The
tree comes from capi.pan_tree once per shape.  Per shape: the wall time of pga_pan_coevo (the backend entry: packing of the program,
upload, reconstruction, flags and scan, event rows, pairs, sort and emit, the three waits and the downloads; median of --reps calls after
a warm-up) with the program of gainloss_ref.program; E and the pairs selected; the word pairs of k_ce_pairs, E (E + 1) / 2 x ceil(B / 32)
(for its time per word pair, next to k_assoc_pairs' in profiles/assoc_kernels.txt, divide the kernel's time from the trace by it); the
wall of capi.pan_coevo in the product (adds the tree compiler and the byte-to-bit packing) and in the checker build.  The checker's
coevo_host runs on a prefix of --checker-items items, twice: with -c 2^31 - 1 nothing is eligible and the time is the reconstruction
and the events, linear in the items; the difference to the run with -c 2 is the pair loops, quadratic in the eligible items.  Both parts
are SCALED to the full shape (by items, and by pairs of eligible items), which the output says.
--device-only runs the pga_pan_coevo calls alone (the run to put under rocprofv3 --kernel-trace --stats for the kernels' times:
k_gl_up, k_gl_down, k_ce_flag and the scan, k_ce_gather, k_ce_rows, k_ce_pairs, the radix sort's passes and k_ce_emit)."""
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
from coevo_direct import chunk, pga_coevo_in_t, pga_coevo_out_t  # noqa: E402
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


def u_shaped(M, A, seed):
    """(M, A) bool: every tenth item accessory and lineage-structured, the others core or rare with a few flips"""
    rng = np.random.default_rng(seed)
    P = np.zeros((M, A), dtype=bool)
    acc = np.arange(0, M, 10)
    P[acc] = tree_ref.lineage_presence(len(acc), A, seed, founders=8, flip=0.02, dup=0.0)
    rest = np.setdiff1d(np.arange(M), acc)
    P[rest[::2]] = True
    n_flip = int(0.2 * len(rest))
    P[rng.choice(rest, size=n_flip), rng.integers(0, A, size=n_flip)] ^= True
    return P


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
    fn = hip.pga_pan_coevo
    fn.restype = C.c_int
    res = []
    for A in [int(x) for x in a.asm.split(",")]:
        M = a.items
        P = u_shaped(M, A, 7)
        t0 = time.perf_counter()
        rec, _ = capi.pan_tree(hip, P, "jaccard", "upgma")
        t_tree = time.perf_counter() - t0
        kids = pr.tree(rec, A, "upgma")
        op, order, need, node_of, par = gr.program(kids, A)
        bits = np.ascontiguousarray(bit_rows(P)[order])
        cin, cout = pga_coevo_in_t(op.ctypes.data, bits.ctypes.data, par.ctypes.data, M, A, 1, 1, 0, 2, 800, 0, 1 << 24, None, 0), pga_coevo_out_t()

        def call():
            if fn(C.byref(cin), C.byref(cout)) != 0:
                raise RuntimeError("pga_pan_coevo failed")
        t = median(call, a.reps, warm=not a.device_only or a.reps > 1)
        events = np.ctypeslib.as_array(C.cast(cout.events, C.POINTER(C.c_int32)), shape=(M,)).copy()
        n = cout.n_pair
        pairs = np.ctypeslib.as_array(C.cast(cout.pair, C.POINTER(C.c_int32)), shape=(n, 4)).copy() if n else np.zeros((0, 4), dtype=np.int32)
        E = int((events >= 2).sum())
        WB = (2 * A - 2 + 31) // 32
        r = {"items": M, "A": A, "branches": 2 * A - 2, "row_words": WB, "stack_need": need, "chunk": chunk(hip, A), "tree_ms": round(t_tree * 1e3, 3),
             "entry_wall_ms": round(t * 1e3, 3), "eligible": E, "pairs_selected": int(n), "tiles": ((E + 127) // 128) * ((E + 127) // 128 + 1) // 2,
             "word_pairs": E * (E + 1) // 2 * WB, "sum_events": int(events.sum())}
        if not a.device_only:
            t_capi = median(lambda: capi.pan_coevo(hip, P, rec, "upgma"), a.reps, warm=False)
            r["product_capi_pan_coevo_ms"] = round(t_capi * 1e3, 3)
            if not a.no_checker:
                import oracle_host
                ora = oracle_host.load()
                m = min(M, a.checker_items)
                t0 = time.perf_counter()
                capi.pan_coevo(ora, P[:m], rec, "upgma", min_events=2147483647)
                t_lin = time.perf_counter() - t0
                t0 = time.perf_counter()
                e_ref, p_ref = capi.pan_coevo(ora, P[:m], rec, "upgma")
                t_all = time.perf_counter() - t0
                Em = int((e_ref >= 2).sum())
                t_pair = max(t_all - t_lin, 0.0)
                f_pair = (E * (E - 1) / 2) / max(Em * (Em - 1) / 2, 1)
                r["checker_prefix_items"], r["checker_prefix_eligible"] = m, Em
                r["checker_prefix_linear_ms"], r["checker_prefix_pairs_ms"] = round(t_lin * 1e3, 1), round(t_pair * 1e3, 1)
                r["checker_linear_ms_scaled"], r["checker_pairs_ms_scaled"] = round(t_lin * 1e3 * (M / m), 1), round(t_pair * 1e3 * f_pair, 1)
                r["checker_host_loops_ms_scaled"] = round(t_lin * 1e3 * (M / m) + t_pair * 1e3 * f_pair, 1)
                sel = pairs[pairs[:, 1] < m]
                r["same"] = bool(np.array_equal(events[:m], e_ref) and np.array_equal(sel, p_ref))
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
