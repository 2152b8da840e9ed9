#!/usr/bin/env python3
"""Timing of pangene rates on one MI355X ("Gain and loss rates measured").

    python tests/run_rates_timing.py [--no-checker] [--items 100000] [--asm 2000,10000] [--reps 3] [--checker-items 100] [--out FILE]

Lineage-structured matrices (tree_ref.lineage_presence) of 100 000 items over A = 2 000 and 10 000 assemblies, upgma.  The tree comes from
capi.pan_tree once per shape.  Per shape, with PANGENE_RATES_TIMING=1 so that the backend reports its kernels' device times from events:
  round     one pga_pan_rates call of 25 parameter sets without posteriors, what a round of the fit is: the wall (best of --reps after a
            warm-up), k_rt_up's device time and its fp64 rate -- 6 operations per node for the parent's vector and 2 per join, 14 (A - 1)
            per item and set;
  post      one call of one set with posteriors: the wall, the three kernels' device times, and the bytes k_rt_down asks for -- its own
            row and its sibling's, 32 bytes per item and node -- over its time;
  fit, given  the wall of capi.pan_rates fitted and at given rates (the posterior call and the scan of nine sets; both include the
            byte-to-bit packing, the item counts and the program), best of --reps after a warm-up; fit_only = their difference;
  checker   the checker build's plain loops on one core at given rates over the first --checker-items items, and that figure scaled
            linearly to all items and to the fit's set evaluations: an EXTRAPOLATION, marked as such."""
import argparse, ctypes as C, json, os, re, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import gainloss_ref as gr  # noqa: E402
import pairs_ref as pr  # noqa: E402
import rates_ref as rr  # noqa: E402
import tree_ref  # noqa: E402
from pairs_direct import bit_rows  # noqa: E402
from rates_direct import chunk, raw  # noqa: E402


def best(f, reps=3):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return min(ts)


class Stderr:
    """what the library writes to file descriptor 2 inside the block"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()

    def kernels(self):
        """the smallest up, down and node device times among the backend's lines"""
        rows = [[float(x) for x in m] for m in re.findall(r"up_ms=([0-9.]+) down_ms=([0-9.]+) node_ms=([0-9.]+)", self.text)]
        return [min(r[i] for r in rows) for i in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-checker", action="store_true")
    ap.add_argument("--items", type=int, default=100000)
    ap.add_argument("--asm", default="2000,10000")
    ap.add_argument("--checker-items", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.init()
    os.environ["PANGENE_RATES_TIMING"] = "1"
    hip = capi.load()
    res = []
    for A in [int(x) for x in a.asm.split(",")]:
        M = a.items
        P = tree_ref.lineage_presence(M, A, 7, founders=8, flip=0.05, dup=0.0)
        P = P[P.any(axis=1)]
        M = len(P)
        rec, _ = capi.pan_tree(hip, P, "jaccard", "upgma")
        kids, ln = rr.lengths(rec, A, "upgma")
        t, _ = rr.normalise(ln)
        op, order, need, node_of, par = gr.program(kids, A)
        bits = np.ascontiguousarray(bit_rows(P)[order])
        n_op = 2 * A - 1

        def tables(pairs):
            sets = [rr.tables(lam, mu, t) for lam, mu in pairs]
            return np.ascontiguousarray(np.stack([s[0] for s in sets])[:, node_of]), np.ascontiguousarray(np.stack([s[1] for s in sets]))
        tab25, pi25 = tables([(2.0 ** (i - 2), 2.0 ** (j - 2)) for i in range(5) for j in range(5)])
        tab1, pi1 = tables([(1.0, 1.0)])

        def call(tab, pi, post):
            if raw(hip, op, bits, par, M, A, tab, pi, post=post)[0] != 0:
                raise RuntimeError("pga_pan_rates failed")
        with Stderr() as e25:
            t_round = best(lambda: call(tab25, pi25, 0), a.reps)
        with Stderr() as e1:
            t_post = best(lambda: call(tab1, pi1, 1), a.reps)
        up25 = e25.kernels()[0]
        up1, down1, node1 = e1.kernels()
        flops = 25.0 * M * 14 * (A - 1)
        down_bytes = 32.0 * M * n_op
        r = {"items": M, "A": A, "stack_need": need, "chunk": chunk(hip, A), "round_wall_ms": round(t_round * 1e3, 3), "round_k_rt_up_ms": up25,
             "k_rt_up_fp64_gflops": round(flops / (up25 * 1e-3) / 1e9, 1), "post_wall_ms": round(t_post * 1e3, 3), "post_k_rt_up_ms": up1, "post_k_rt_down_ms": down1,
             "post_k_rt_node_ms": node1, "k_rt_down_bytes": down_bytes, "k_rt_down_tb_per_s": round(down_bytes / (down1 * 1e-3) / 1e12, 3)}
        with Stderr():
            fit = capi.pan_rates(hip, P, rec, "upgma")
            t_fit = best(lambda: capi.pan_rates(hip, P, rec, "upgma"), a.reps)
            t_given = best(lambda: capi.pan_rates(hip, P, rec, "upgma", fit["gain"], fit["loss"]), a.reps)
        r.update({"rounds": fit["rounds"], "converged": fit["converged"], "gain": fit["gain"], "loss": fit["loss"], "lnL": fit["lnL"],
                  "fit_wall_ms": round(t_fit * 1e3, 1), "given_wall_ms": round(t_given * 1e3, 1), "fit_only_wall_ms": round((t_fit - t_given) * 1e3, 1)})
        if not a.no_checker:
            import oracle_host
            ora = oracle_host.load()
            m = min(M, a.checker_items)
            t0 = time.perf_counter()
            capi.pan_rates(ora, P[:m], rec, "upgma", fit["gain"], fit["loss"])
            t_host = time.perf_counter() - t0
            r["checker_given_ms_measured_on_items"] = [m, round(t_host * 1e3, 1)]
            r["checker_given_ms_EXTRAPOLATED"] = round(t_host * 1e3 * M / m, 0)
            r["checker_fit_ms_EXTRAPOLATED"] = round(t_host * 1e3 * M / m * (25.0 * fit["rounds"] / 10.0), 0)  # ten set evaluations against 25 a round
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
