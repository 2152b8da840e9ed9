#!/usr/bin/env python3
"""Timing of pangene trait on one MI355X ("Trait measured").

    python tests/run_trait_timing.py [--device-only] [--no-checker] [--perms 10000,1000000] [--out FILE]

Shapes 5 000 x 10 000 and 60 000 x 200 (assoc_ref.planted), one balanced random trait, n = 10^4 and 10^6 permutations.  Per shape and
n: the wall time of pga_pan_trait (the backend entry: upload, obs, the batches of k_trait_perm + k_trait_count, download of a, s, k;
best of three after a warm-up call), of capi.pan_trait in the product (adds the compaction and the byte-to-bit packing) and of
capi.pan_trait in the checker build (the host loops of trait.cpp on one core; at n = 10^6 it is run with 10^4 permutations and the
figure is SCALED by 100, which the output says).  valu_ops = G x n x ceil(N / 32) x 2, the operation count of k_trait_count; its
share of VALU peak is that over the kernel's time (from rocprofv3 --kernel-trace --stats on a --device-only run) over 78.6 Tops/s.
--device-only runs the pga_pan_trait calls alone."""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import assoc_ref as ar  # noqa: E402
import trait_ref as tr  # noqa: E402
from trait_direct import pga_trait_in_t, pga_trait_out_t  # noqa: E402

SHAPES = [(5000, 10000), (60000, 200)]
PEAK_OPS = 256 * 128 * 2.4e9


def best(f, reps=3, warm=True):
    if warm:
        f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return min(ts)


def entry_time(lib, P, y, n, reps):
    G, N = P.shape
    bits = np.ascontiguousarray(tr.pack(P))
    lab = np.ascontiguousarray(tr.pack(y[None, :])[0])
    cin, cout = pga_trait_in_t(bits.ctypes.data, lab.ctypes.data, G, N, 1, n, 11, None), pga_trait_out_t()
    fn = lib.pga_pan_trait
    fn.restype = C.c_int

    def call():
        if fn(C.byref(cin), C.byref(cout)) != 0:
            raise RuntimeError("pga_pan_trait failed")
    t = best(call, reps)
    return t, np.ctypeslib.as_array(cout.k, shape=(G,)).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--no-checker", action="store_true")
    ap.add_argument("--perms", default="10000,1000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.init()
    hip = capi.load()
    res = []
    for G, N in SHAPES:
        P = ar.planted(G, N, 7, n_module=50)
        y = (np.random.default_rng(5).permutation(N) < N // 2).astype(np.uint8)
        W = (N + 31) // 32
        for n in [int(x) for x in a.perms.split(",")]:
            ops = G * n * W * 2
            t, k = entry_time(hip, P, y, n, a.reps)
            r = {"G": G, "N": N, "n_perm": n, "valu_ops": ops, "ops_at_peak_ms": round(ops / PEAK_OPS * 1e3, 3), "entry_wall_ms": round(t * 1e3, 3), "sum_k": int(k.sum())}
            if not a.device_only:
                r["product_capi_pan_trait_ms"] = round(best(lambda: capi.pan_trait(hip, P, y, n_perm=n), a.reps, warm=False) * 1e3, 3)
                if not a.no_checker:
                    import oracle_host
                    ora = oracle_host.load()
                    n_host = min(n, 10000)
                    t0 = time.perf_counter()
                    ref = capi.pan_trait(ora, P, y, n_perm=n_host)
                    t_host = time.perf_counter() - t0
                    r["checker_host_loops_ms"] = round(t_host * 1e3 * (n / n_host), 1)
                    r["checker_scaled_from_n"] = n_host if n_host != n else None
                    if n_host == n:
                        r["same"] = bool(np.array_equal(capi.pan_trait(hip, P, y, n_perm=n)["k"], ref["k"]))
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
