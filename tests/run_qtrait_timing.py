#!/usr/bin/env python3
"""Timing of pangene qtrait on one MI355X ("Quantitative traits measured").  A script, not a test.

    python tests/run_qtrait_timing.py [--device-only] [--no-checker] [--perms 10000] [--reps 3] [--out FILE]

Shapes 5 000 x 10 000 and 60 000 x 200 (assoc_ref.planted), one continuous trait without ties, n = 10^4 permutations.  Per shape: the
wall time of pga_pan_qtrait (the backend entry: upload, obs, the batches of k_qtrait_perm + k_qtrait_count, download of a, D, k; best
of three after a warm-up call), of capi.pan_qtrait in the product (adds the ranks, the compaction and the byte-to-bit packing) and of
capi.pan_qtrait in the checker build (the host loops of trait.cpp on one core, run with a prefix of the permutations and SCALED, which
the output says).  mfma_ops = planes x 2 x G x K x n with K = N rounded up to 128 and planes = 2 (1 when N <= 128), the operation count
of k_qtrait_count; its share of the i8 MFMA peak is that over the kernel's time (from rocprofv3 --kernel-trace --stats on a
--device-only --reps 1 run of its own) over the peak.  The yardstick for k_qtrait_count is 16 x the k_trait_count time of
tests/run_trait_timing.py at the same shape and n in the same session.  --device-only runs the pga_pan_qtrait calls alone."""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import assoc_ref as ar  # noqa: E402
import trait_ref as tr  # noqa: E402
from qtrait_direct import pga_qtrait_in_t, pga_qtrait_out_t  # noqa: E402

SHAPES = [(5000, 10000), (60000, 200)]
PEAK_I8_OPS = 256 * 4 * 2048 * 2.4e9  # 256 CUs x 4 SIMDs x 2 048 int8 operations a clock (twice the bf16 rate: 5.0 Pops/s) at 2.4 GHz
CHECKER_PREFIX = 200


def best(f, reps=3, warm=True):
    if warm:
        f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return min(ts)


def centred_ranks(v):
    """c2 of distinct values: 2 rank - (N + 1) with ranks from 1"""
    r = np.empty(len(v), dtype=np.int64)
    r[np.argsort(v, kind="stable")] = np.arange(1, len(v) + 1)
    return (2 * r - (len(v) + 1)).astype(np.int16)


def entry_time(lib, P, c2, n, reps):
    G, N = P.shape
    bits = np.ascontiguousarray(tr.pack(P))
    c2 = np.ascontiguousarray(c2, dtype=np.int16)
    cin, cout = pga_qtrait_in_t(bits.ctypes.data, c2.ctypes.data, G, N, 1, n, 11, None, None), pga_qtrait_out_t()
    fn = lib.pga_pan_qtrait
    fn.restype = C.c_int

    def call():
        if fn(C.byref(cin), C.byref(cout)) != 0:
            raise RuntimeError("pga_pan_qtrait failed")
    t = best(call, reps)
    return t, np.ctypeslib.as_array(cout.k, shape=(G,)).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--no-checker", action="store_true")
    ap.add_argument("--perms", default="10000")
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
        v = np.random.default_rng(5).normal(size=N)
        c2 = centred_ranks(v)
        K, planes = (N + 127) // 128 * 128, 2 if N > 128 else 1
        for n in [int(x) for x in a.perms.split(",")]:
            ops = planes * 2 * G * K * n
            t, k = entry_time(hip, P, c2, n, a.reps)
            r = {"G": G, "N": N, "n_perm": n, "mfma_ops": ops, "ops_at_i8_peak_ms": round(ops / PEAK_I8_OPS * 1e3, 3), "entry_wall_ms": round(t * 1e3, 3), "sum_k": int(k.sum())}
            if not a.device_only:
                r["product_capi_pan_qtrait_ms"] = round(best(lambda: capi.pan_qtrait(hip, P, v, n_perm=n), a.reps, warm=False) * 1e3, 3)
                if not a.no_checker:
                    import oracle_host
                    ora = oracle_host.load()
                    n_host = min(n, CHECKER_PREFIX)
                    t0 = time.perf_counter()
                    ref = capi.pan_qtrait(ora, P, v, n_perm=n_host)
                    t_host = time.perf_counter() - t0
                    r["checker_host_loops_ms"] = round(t_host * 1e3 * (n / n_host), 1)
                    r["checker_scaled_from_n"] = n_host if n_host != n else None
                    r["same_on_prefix"] = bool(np.array_equal(capi.pan_qtrait(hip, P, v, n_perm=n_host)["k"], ref["k"]))
            print(json.dumps(r), flush=True)
            res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
