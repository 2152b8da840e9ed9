#!/usr/bin/env python3
"""Timing of pangene permanova on one MI355X ("PERMANOVA measured").  A script, not a test.

    python tests/run_permanova_timing.py [--device-only] [--no-checker] [--sizes 2000,10000] [--perms 10000] [--reps 3] [--out FILE]

Lineage-structured presence matrices (tree_ref.lineage_presence, 5 000 items) at N = 2 000 and 10 000 assemblies, their jaccard
distances, one balanced trait, n = 10^4 permutations.  Per size: the wall time of pga_pan_permanova (the backend entry: upload of the
N x N matrix, k_perma_prep, the observed row, the batches of k_trait_perm + k_perma_quad + k_perma_stat, one wait; best of three after a
warm-up call), of capi.pan_permanova in the product (adds the matrix checks and the compaction) and of capi.pan_permanova in the checker
build (the host loops of tree.cpp on one core, run with a prefix of the permutations and SCALED, which the output says).
macs = D x n x N^2 with D the digit planes, the figure the issue of this command counts k_perma_quad by (the kernel itself does about
half of it: the symmetry); its rate is that over the kernel's time from rocprofv3 --kernel-trace --stats on a --device-only --reps 1 run
of its own, and the yardstick is the rate k_qtrait_count reaches in tests/run_qtrait_timing.py in the same session.  --device-only runs
the pga_pan_permanova calls alone."""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import permanova_ref as pr  # noqa: E402
import trait_ref as tr  # noqa: E402
import tree_ref  # noqa: E402
from permanova_direct import pga_permanova_in_t, pga_permanova_out_t  # noqa: E402

ITEMS = 5000
CHECKER_PREFIX = 20


def best(f, reps=3, warm=True):
    if warm:
        f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return min(ts)


def entry_time(lib, q, y, s, n, reps):
    N = len(y)
    label = np.ascontiguousarray(tr.pack(y[None, :])[0])
    cin = pga_permanova_in_t(q.ctypes.data, label.ctypes.data, N, s, int(q.max()), int(y.sum()), n, 11, None, None, None)
    cout = pga_permanova_out_t()
    fn = lib.pga_pan_permanova
    fn.restype = C.c_int

    def call():
        if fn(C.byref(cin), C.byref(cout)) != 0:
            raise RuntimeError("pga_pan_permanova failed")
    t = best(call, reps)
    return t, (cout.t, cout.a, cout.b, cout.k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--no-checker", action="store_true")
    ap.add_argument("--sizes", default="2000,10000")
    ap.add_argument("--perms", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.init()
    hip = capi.load()
    res = []
    n = a.perms
    for N in [int(x) for x in a.sizes.split(",")]:
        P = tree_ref.lineage_presence(ITEMS, N, 7)
        S = (P.astype(np.float32).T @ P.astype(np.float32)).astype(np.int64)  # exact: counts below 2^24
        q = np.ascontiguousarray(tree_ref.fixed(S, "jaccard")[0], dtype=np.int32)
        y = pr.balanced(N, 5)
        s = pr.shift_of(int(q.max()), N)
        D = pr.planes_of((int(q.max()) >> s) ** 2)
        t, out = entry_time(hip, q, y, s, n, a.reps)
        r = {"N": N, "items": ITEMS, "n_perm": n, "shift": s, "planes": D, "macs": D * n * N * N, "entry_wall_ms": round(t * 1e3, 3), "k": int(out[3])}
        if not a.device_only:
            yl = y.astype(np.int8)
            r["product_capi_pan_permanova_ms"] = round(best(lambda: capi.pan_permanova(hip, q, yl, n_perm=n), a.reps, warm=False) * 1e3, 3)
            if not a.no_checker:
                import oracle_host
                ora = oracle_host.load()
                n_host = min(n, CHECKER_PREFIX)
                capi.pan_permanova(ora, q, yl, n_perm=0)
                t0 = time.perf_counter()
                base = capi.pan_permanova(ora, q, yl, n_perm=0)
                t_base = time.perf_counter() - t0
                t0 = time.perf_counter()
                ref = capi.pan_permanova(ora, q, yl, n_perm=n_host)
                t_host = time.perf_counter() - t0
                r["checker_host_loops_ms"] = round((t_base + (t_host - t_base) * (n / n_host)) * 1e3, 1)  # the part that does not grow with n is not scaled
                r["checker_scaled_from_n"] = n_host if n_host != n else None
                r["same_on_prefix"] = bool(pr.same(capi.pan_permanova(hip, q, yl, n_perm=n_host), {k: np.asarray(v) for k, v in ref.items()}) and
                                           int(base["A"][0]) == out[1])
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
