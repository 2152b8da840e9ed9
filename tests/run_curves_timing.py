#!/usr/bin/env python3
"""Timing of the accumulation curves on the GPU.  Not a test: prints one JSON line per measurement.

    python3 tests/run_curves_timing.py [--device-only] [--out FILE]

Shapes (A assemblies, G genes, n orders): (10 000, 5 000, 100) and (200, 60 000, 100), U-shaped gene frequencies (core plus cloud).
Per shape: the wall time of pga_pan_curves (the backend entry: upload, kernels, download; median of 5 after a warm-up call), of
pg_pan_curves in the product (adds the bit packing and the orders) and of pg_pan_curves in the checker build (the host loops of
curves.cpp, one core).  Then BASELINE configs[1] (100 x 5 000 bacterial) through the build route: `pangene --curves=100` against
`pangene --matrix`, with the step's own split from PANGENE_CURVES_TIMING=1.  --device-only runs the pga_pan_curves calls alone (for
rocprofv3 --kernel-trace --stats)."""
import argparse, ctypes as C, json, os, re, statistics, subprocess, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi, synth  # noqa: E402
import curves_ref as cr  # noqa: E402

HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
SHAPES = [(10000, 5000, 100), (200, 60000, 100)]


class pga_curves_in_t(C.Structure):
    _fields_ = [("bits", C.c_void_p), ("order", C.c_void_p), ("n_gene", C.c_int32), ("n_asm", C.c_int32), ("n_perm", C.c_int32)]


class pga_curves_out_t(C.Structure):
    _fields_ = [("count", C.c_void_p)]


def med(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts)


def entry_time(lib, P, n):
    G, A = P.shape
    W = (A + 31) // 32
    b = np.zeros((G, W * 4), dtype=np.uint8)
    b[:, :(A + 7) // 8] = np.packbits(P, axis=1, bitorder="little")
    bits = np.ascontiguousarray(b).view("<u4")
    rng = np.random.default_rng(1)
    order = np.ascontiguousarray(np.stack([np.arange(A)] + [rng.permutation(A) for _ in range(n - 1)]).astype(np.int32))
    cin = pga_curves_in_t(bits.ctypes.data, order.ctypes.data, G, A, n)
    cout = pga_curves_out_t()
    fn = lib.pga_pan_curves
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(pga_curves_in_t), C.POINTER(pga_curves_out_t)]

    def call():
        if fn(C.byref(cin), C.byref(cout)) != 0:
            raise RuntimeError("pga_pan_curves failed")
    return med(call)


def timed_cli(argv, reps=3):
    e = dict(os.environ, PANGENE_CURVES_TIMING="1")
    best, line = None, ""
    for _ in range(reps):
        t = time.perf_counter()
        r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=1800)
        dt = time.perf_counter() - t
        if r.returncode != 0:
            raise RuntimeError("%s: exit %d\n%s" % (" ".join(argv[:3]), r.returncode, r.stderr.decode()[-2000:]))
        m = [l for l in r.stderr.decode().split("\n") if l.startswith("[curves-timing]")]
        if best is None or dt < best:
            best, line = dt, (m[-1] if m else "")
    return best, dict(re.findall(r"(\w+)=(\S+)", line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.init()
    hip = capi.load()
    res = []

    def emit(r):
        print(json.dumps(r), flush=True)
        res.append(r)
    for A, G, n in SHAPES:
        P = cr.u_shaped(G, A, 7)
        r = {"A": A, "G": G, "n": n, "entry_wall_ms": round(entry_time(hip, P, n) * 1e3, 3)}
        if not a.device_only:
            r["product_pg_pan_curves_ms"] = round(med(lambda: capi.pan_curves(hip, P, n)) * 1e3, 3)
            import oracle_host
            ora = oracle_host.load()
            r["checker_host_loops_ms"] = round(med(lambda: capi.pan_curves(ora, P, n), reps=1) * 1e3, 3)
            r["same"] = bool(np.array_equal(capi.pan_curves(hip, P, n), capi.pan_curves(ora, P, n)))
        emit(r)
    if not a.device_only:
        with tempfile.TemporaryDirectory() as td:
            files = synth.write_files(synth.bact(100, 5000, seed=1), os.path.join(td, "c1"))
            t_curves, kv = timed_cli([HIP, "--curves=100"] + files)
            t_matrix, _ = timed_cli([HIP, "--matrix"] + files)
            emit({"input": "configs1", "curves_wall_s": round(t_curves, 4), "matrix_wall_s": round(t_matrix, 4),
                  "genes": int(kv.get("genes", -1)), "assemblies": int(kv.get("assemblies", -1)),
                  "prep_ms": float(kv.get("prep_ms", "nan")), "count_ms": float(kv.get("count_ms", "nan")),
                  "write_ms": float(kv.get("write_ms", "nan"))})
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
