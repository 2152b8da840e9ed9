#!/usr/bin/env python3
"""Timing of the pairwise shared-item counts (pangene dist) on the GPU.  Not a test: prints one JSON line per measurement.

    python3 tests/run_dist_timing.py [--device-only] [--no-checker] [--out FILE]

Shapes (A assemblies, M items): (10 000, 5 000) and (200, 60 000), every assembly with a density of its own.  Per shape: the wall time
of pga_pan_shared (the backend entry: upload, kernel, download of the A x A result; median of 5 after a warm-up call), of pg_pan_shared
in the product (adds the bit packing and the copy into the caller's array) and of pg_pan_shared in the checker build (the host loops
of dist.cpp, one core, one call).  The kernel's share of VALU peak: A (A + 1) / 2 * ceil(M / 32) word pairs * 2 ops over the kernel
time of rocprofv3 and 78.6 Tops/s (256 CUs x 128 lanes x 2.4 GHz); the operation count is printed here.  --device-only runs the
pga_pan_shared calls alone (for rocprofv3 --kernel-trace --stats)."""
import argparse, ctypes as C, json, os, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import dist_direct  # noqa: E402

SHAPES = [(10000, 5000), (200, 60000)]
PEAK_OPS = 256 * 128 * 2.4e9


class pga_shared_in_t(C.Structure):
    _fields_ = [("bits", C.c_void_p), ("n_item", C.c_int32), ("n_asm", C.c_int32)]


class pga_shared_out_t(C.Structure):
    _fields_ = [("shared", C.c_void_p)]


def med(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts)


def entry_time(lib, P):
    M, A = P.shape
    W = (M + 31) // 32
    b = np.zeros((A, W * 4), dtype=np.uint8)
    b[:, :(M + 7) // 8] = np.packbits(P.T, axis=1, bitorder="little")
    bits = np.ascontiguousarray(b).view("<u4")
    cin, cout = pga_shared_in_t(bits.ctypes.data, M, A), pga_shared_out_t()
    fn = lib.pga_pan_shared
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(pga_shared_in_t), C.POINTER(pga_shared_out_t)]

    def call():
        if fn(C.byref(cin), C.byref(cout)) != 0:
            raise RuntimeError("pga_pan_shared failed")
    return med(call)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--no-checker", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.init()
    hip = capi.load()
    res = []
    for A, M in SHAPES:
        P = dist_direct.presence(M, A, 7)
        ops = A * (A + 1) // 2 * ((M + 31) // 32) * 2
        r = {"A": A, "M": M, "valu_ops": ops, "ops_at_peak_us": round(ops / PEAK_OPS * 1e6, 2),
             "entry_wall_ms": round(entry_time(hip, P) * 1e3, 3)}
        if not a.device_only:
            r["product_pg_pan_shared_ms"] = round(med(lambda: capi.pan_shared(hip, P)) * 1e3, 3)
            if not a.no_checker:
                import oracle_host
                ora = oracle_host.load()
                t = time.perf_counter()
                S_ora = capi.pan_shared(ora, P)
                r["checker_host_loops_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                r["same"] = bool(np.array_equal(capi.pan_shared(hip, P), S_ora))
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
