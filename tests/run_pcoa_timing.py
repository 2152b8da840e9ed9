#!/usr/bin/env python3
"""Timing of pangene pcoa on one MI355X ("Principal coordinates measured").  A script, not a test.

    python tests/run_pcoa_timing.py [--sizes 2048,10000] [--axes 3] [--reps 3] [--eigh-max 2048] [--out FILE]

A lineage-structured presence matrix (tree_ref.lineage_presence, 5 000 items) at N assemblies and its gene:jaccard distances in fixed
point.  Per size: the wall time of pga_pan_pcoa (the backend entry: upload of the N x N matrix, the chunks of steps, the Ritz vectors;
best of `reps` after a warm-up call), the steps it took, and the device time of k_pcoa_mult per product from the events the entry records
under PANGENE_PCOA_TIMING (its [pcoa-kernels] line on stderr), with the bytes N^2 x 4 over that time; the README's copy-kernel figure
(6.0-6.2 TB/s) is the ceiling to read it against.  Up to --eigh-max assemblies numpy.linalg.eigh of the dense B on ONE host core stands beside it, and
the entry's eigenvalues are checked against it within 1e-9 l_1."""
import os
os.environ.setdefault("OMP_NUM_THREADS", "1")  # numpy's eigh on one core (before numpy loads its BLAS)
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
os.environ.setdefault("MKL_NUM_THREADS", "1")
import argparse, json, re, sys, tempfile, time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402
import pcoa_ref as pc  # noqa: E402
import tree_ref  # noqa: E402
from pcoa_direct import direct  # noqa: E402

ITEMS = 5000


def with_stderr(f):
    """f() with the process's stderr (the library writes there) captured: (result, text)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            r = f()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return r, tmp.read().decode(errors="replace")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,10000")
    ap.add_argument("--axes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--eigh-max", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.init()
    hip = capi.load()
    res = []
    for N in [int(x) for x in a.sizes.split(",")]:
        P = tree_ref.lineage_presence(ITEMS, N, 7)
        S = (P.astype(np.float32).T @ P.astype(np.float32)).astype(np.int64)  # exact: counts below 2^24
        q = np.ascontiguousarray(tree_ref.fixed(S, "jaccard")[0], dtype=np.int32)
        direct(hip, q, 20, a.axes)  # warm-up: the buffers, the code object
        walls = []
        for _ in range(a.reps):
            t = time.perf_counter()
            got = direct(hip, q, 20, a.axes)
            walls.append(time.perf_counter() - t)
        os.environ["PANGENE_PCOA_TIMING"] = "1"
        _, err = with_stderr(lambda: direct(hip, q, 20, a.axes))
        del os.environ["PANGENE_PCOA_TIMING"]
        m = re.search(r"\[pcoa-kernels\].*mult_ms_per_step=([0-9.]+)", err)
        mult_ms = float(m.group(1)) if m else None
        r = {"N": N, "items": ITEMS, "axes": int(got["axes"]), "steps": int(got["steps"]), "restarts": int(got["restarts"]), "converged": int(got["converged"]),
             "entry_wall_ms": round(min(walls) * 1e3, 3), "mult_ms": mult_ms, "mult_tb_per_s": round(N * N * 4 / (mult_ms * 1e-3) / 1e12, 3) if mult_ms else None,
             "eig": [float(x) for x in got["eig"]]}
        if N <= a.eigh_max:
            B = pc.matrix_b(q, 20)
            t = time.perf_counter()
            w = np.linalg.eigh(B)[0][::-1]
            r["numpy_eigh_one_core_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            w = w[np.argsort(-w)]
            top = [x for x in w if abs(x) > 1e-12 * w[0]][:a.axes]  # (the zero of the constant vector is no axis)
            r["eig_within_1e-9"] = bool(np.all(np.abs(np.array(top) - got["eig"][:len(top)]) <= 1e-9 * w[0]))
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
