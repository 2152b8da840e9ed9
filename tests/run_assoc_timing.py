#!/usr/bin/env python3
"""Timing of the gene associations (pangene assoc) on the GPU.  Not a test: prints one JSON line per measurement.

    python3 tests/run_assoc_timing.py [--device-only] [--no-checker] [--out FILE]

Shapes (G genes, A assemblies): (5 000, 10 000) and (60 000, 200), U-shaped frequency spectrum with planted modules
(assoc_ref.planted).  Per shape: E (eligible rows) and the selected pairs, the wall time of pga_pan_assoc (the backend entry: upload,
prepare, pairs, sort, download of the sparse list; median of 5 after a warm-up call), of pg_pan_assoc from Python in the product (adds
the bit packing and the copy into the caller's array) and in the checker build (the host loops of assoc.cpp, one core, one call).
The yardstick is the only route the library had before: pan_shared on the transposed matrix (G x G int32 on the host) and a numpy
filter of that square; beyond 65 535 genes pan_shared refuses, which is recorded.  The pairs kernel's share of VALU peak:
E (E + 1) / 2 * ceil(A / 32) word pairs * 2 ops over the kernel time of rocprofv3 and 78.6 Tops/s (256 CUs x 128 lanes x 2.4 GHz); the
operation count is printed here.  --device-only runs the pga_pan_assoc calls alone (for rocprofv3 --kernel-trace --stats)."""
import argparse, ctypes as C, json, os, statistics, sys, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import assoc_ref as ar  # noqa: E402

SHAPES = [(5000, 10000), (60000, 200)]
PEAK_OPS = 256 * 128 * 2.4e9


class pga_assoc_in_t(C.Structure):
    _fields_ = [("bits", C.c_void_p), ("n_gene", C.c_int32), ("n_asm", C.c_int32), ("min_count", C.c_int32), ("r_permille", C.c_int32),
                ("sign", C.c_int32), ("max_pair", C.c_int64)]


class pga_assoc_out_t(C.Structure):
    _fields_ = [("n_pair", C.c_int64), ("pair", C.c_void_p), ("count", C.c_void_p)]


def med(f, reps=5):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts)


def entry_time(lib, P):
    G, A = P.shape
    W = (A + 31) // 32
    b = np.zeros((G, W * 4), dtype=np.uint8)
    b[:, :(A + 7) // 8] = np.packbits(P, axis=1, bitorder="little")
    bits = np.ascontiguousarray(b).view("<u4")
    cin, cout = pga_assoc_in_t(bits.ctypes.data, G, A, 2, 800, 0, 16777216), pga_assoc_out_t()
    fn = lib.pga_pan_assoc
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(pga_assoc_in_t), C.POINTER(pga_assoc_out_t)]

    def call():
        if fn(C.byref(cin), C.byref(cout)) != 0:
            raise RuntimeError("pga_pan_assoc failed")
    return med(call), int(cout.n_pair)


def old_route(lib, P):
    """pan_shared over the genes as if they were assemblies, then the selection on the host: (seconds, pairs) or (None, reason)"""
    G, A = P.shape
    cnt = P.sum(axis=1, dtype=np.int64)
    PT = np.ascontiguousarray(P.T)

    def go():
        S = capi.pan_shared(lib, PT).astype(np.int64)
        el = np.minimum(cnt, A - cnt) >= 2
        D = S * A - cnt[:, None] * cnt[None, :]
        V = cnt * (A - cnt)
        ok = (10 ** 6 * D.astype(np.float64) ** 2 >= 640000.0 * V[:, None].astype(np.float64) * V[None, :]) & el[:, None] & el[None, :]
        return int(np.triu(ok, 1).sum())  # (float64 here: the yardstick's time, not its last bit, is what is measured)
    try:
        n = go()
    except RuntimeError as e:
        return None, str(e)
    return med(go, 3), n


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
    for G, A in SHAPES:
        P = ar.planted(G, A, 7, n_module=50)
        cnt = P.sum(axis=1, dtype=np.int64)
        E = int((np.minimum(cnt, A - cnt) >= 2).sum())
        W = (A + 31) // 32
        ops = E * (E + 1) // 2 * W * 2
        t, n = entry_time(hip, P)
        r = {"G": G, "A": A, "E": E, "pairs": n, "pair_tests": E * (E - 1) // 2, "valu_ops": ops, "ops_at_peak_us": round(ops / PEAK_OPS * 1e6, 2),
             "entry_wall_ms": round(t * 1e3, 3)}
        if not a.device_only:
            r["product_pg_pan_assoc_ms"] = round(med(lambda: capi.pan_assoc(hip, P)) * 1e3, 3)
            t_old, n_old = old_route(hip, P)
            r["transposed_pan_shared_route_ms"] = None if t_old is None else round(t_old * 1e3, 1)
            r["transposed_pan_shared_route_result"] = n_old
            if not a.no_checker:
                import oracle_host
                ora = oracle_host.load()
                t0 = time.perf_counter()
                ref = capi.pan_assoc(ora, P)
                r["checker_host_loops_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                got = capi.pan_assoc(hip, P)
                r["same"] = bool(np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]))
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
