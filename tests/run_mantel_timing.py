#!/usr/bin/env python3
"""Timing of pangene mantel on one MI355X ("Mantel measured").  A script, not a test.

    python tests/run_mantel_timing.py [--device-only] [--no-checker] [--sizes 2000] [--perms 10000] [--reps 3] [--out FILE]

A lineage-structured presence matrix (tree_ref.lineage_presence, 5 000 items) at N = 2 000 assemblies: X is its gene:jaccard distances, Y
the same with symmetric noise added (adj-like: a second matrix that tells much the same story), n = 10^4 permutations.  Per size: the wall
time of pga_pan_mantel (the backend entry: upload of the two N x N matrices, the identity order, the batches of k_mantel_order +
k_mantel_z + k_mantel_stat, one wait; best of three after a warm-up call), of capi.pan_mantel in the product (adds the matrix checks, the
shifts and the sums) and of capi.pan_mantel in the checker build (the host loops of tree.cpp on one core, run with a prefix of the
permutations and SCALED, which the output says).  gathers = n x N (N - 1) / 2, the multiply-adds k_mantel_z does; its rate is that over
the kernel's time from rocprofv3 --kernel-trace --stats on a --device-only --reps 1 run of its own.  --device-only runs the
pga_pan_mantel calls alone."""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import mantel_ref as mr  # noqa: E402
import tree_ref  # noqa: E402
from mantel_direct import pga_mantel_in_t, pga_mantel_out_t  # noqa: E402

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


def entry_time(lib, a, b, n, reps):
    cin = pga_mantel_in_t(a.ctypes.data, b.ctypes.data, a.shape[0], int(a.max()), int(b.max()), n, 11, None, None)
    cout = pga_mantel_out_t()
    fn = lib.pga_pan_mantel
    fn.restype = C.c_int

    def call():
        if fn(C.byref(cin), C.byref(cout)) != 0:
            raise RuntimeError("pga_pan_mantel failed")
    t = best(call, reps)
    return t, (cout.z, cout.n_ge, cout.n_le)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--no-checker", action="store_true")
    ap.add_argument("--sizes", default="2000")
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
        qx = tree_ref.fixed(S, "jaccard")[0]
        qy = mr.noisy_copy(qx, 9, 1 << 16)
        sx, sy = mr.shift_of(int(qx.max()), N), mr.shift_of(int(qy.max()), N)
        da, db = np.ascontiguousarray(qx >> sx, dtype=np.int32), np.ascontiguousarray(qy >> sy, dtype=np.int32)
        t, out = entry_time(hip, da, db, n, a.reps)
        r = {"N": N, "items": ITEMS, "n_perm": n, "sx": sx, "sy": sy, "gathers": n * N * (N - 1) // 2, "entry_wall_ms": round(t * 1e3, 3), "n_ge": int(out[1]), "n_le": int(out[2])}
        if not a.device_only:
            r["product_capi_pan_mantel_ms"] = round(best(lambda: capi.pan_mantel(hip, qx, qy, n_perm=n), a.reps, warm=False) * 1e3, 3)
            if not a.no_checker:
                import oracle_host
                ora = oracle_host.load()
                n_host = min(n, CHECKER_PREFIX)
                capi.pan_mantel(ora, qx, qy, n_perm=0)
                t0 = time.perf_counter()
                base = capi.pan_mantel(ora, qx, qy, n_perm=0)
                t_base = time.perf_counter() - t0
                t0 = time.perf_counter()
                ref = capi.pan_mantel(ora, qx, qy, n_perm=n_host)
                t_host = time.perf_counter() - t0
                r["checker_host_loops_ms"] = round((t_base + (t_host - t_base) * (n / n_host)) * 1e3, 1)  # the part that does not grow with n is not scaled
                r["checker_scaled_from_n"] = n_host if n_host != n else None
                r["same_on_prefix"] = bool(mr.same(capi.pan_mantel(hip, qx, qy, n_perm=n_host), ref) and base["Z"] == out[0])
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
