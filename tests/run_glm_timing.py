#!/usr/bin/env python3
"""Timing of pangene glm's product on one MI355X ("Structure-adjusted association measured").  A script, not a test.

    python tests/run_glm_timing.py [--sizes 50000x10000x4] [--cov 3] [--reps 3] [--host-genes 2000] [--out FILE]

A random presence matrix of G genes x A assemblies at density 0.3, T quantitative traits with a tenth of their values missing and k
random covariates through pg_pan_glm, so that the null fits, the columns and the Cholesky factors are the library's own.  Per size: the
wall time of pg_pan_glm in the product (packing the matrix, the null fits, upload, the two kernels, download; best of `reps` after a
warm-up call); the device time of k_glm_sums and k_glm_stat from the events pga_pan_glm records under PANGENE_GLM_TIMING (its
[glm-kernels] line on stderr); the fp64 rate 2 x G x A_pad x 16 x T / time of the sums kernel, A_pad = A rounded up to 128, beside the
78.6 TFLOP/s of the fp64 matrix cores; and the bytes the kernel must move at least -- the bit matrix once, the partial sums once -- over
that time, beside the README's copy-kernel figure (6.0-6.2 TB/s).  The checker build's host loop (the set bits walked in fp64 on ONE
core; its [glm-timing] stat_ms) runs on the first --host-genes genes of the same matrix and is scaled to G: it is linear in the genes."""
import os
os.environ.setdefault("OMP_NUM_THREADS", "1")
import argparse, json, re, sys, tempfile, time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
from pangene_amd import capi  # noqa: E402


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
    ap.add_argument("--sizes", default="50000x10000x4")
    ap.add_argument("--cov", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-genes", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.init()
    import oracle_host
    hip, ora = capi.load(), oracle_host.load()
    res = []
    for size in a.sizes.split(","):
        G, A, T = (int(x) for x in size.split("x"))
        rng = np.random.default_rng(G + A + T)
        P = rng.random((G, A), dtype=np.float32) < 0.3
        cov = rng.standard_normal((A, a.cov))
        y = rng.standard_normal((T, A)) + (cov[:, 0] if a.cov else 0.0)
        y[rng.random((T, A)) < 0.1] = np.nan
        capi.pan_glm(hip, P, y, cov, "quant")  # warm-up: the buffers, the code object
        walls = []
        for _ in range(a.reps):
            t = time.perf_counter()
            got = capi.pan_glm(hip, P, y, cov, "quant")
            walls.append(time.perf_counter() - t)
        os.environ["PANGENE_GLM_TIMING"] = "1"
        _, err = with_stderr(lambda: capi.pan_glm(hip, P, y, cov, "quant"))
        m = re.search(r"\[glm-kernels\].*segments=(\d+) .*sums_ms=([0-9.]+) stat_ms=([0-9.]+)", err)
        segs, sums_ms, stat_ms = (int(m.group(1)), float(m.group(2)), float(m.group(3))) if m else (None, None, None)
        Gh = min(G, a.host_genes)
        host, err = with_stderr(lambda: capi.pan_glm(ora, P[:Gh], y, cov, "quant"))
        del os.environ["PANGENE_GLM_TIMING"]
        mh = re.search(r"\[glm-timing\] route=array .*stat_ms=([0-9.]+)", err)
        host_ms = float(mh.group(1)) * G / Gh if mh else None
        a_pad = (A + 127) // 128 * 128
        flop = 2.0 * G * a_pad * 16 * T
        byts = G * ((A + 31) // 32) * 4 + (segs or 1) * T * G * 16 * 8
        same = bool(np.array_equal(got["a"][:, :Gh], host["a"]) and np.allclose(got["U"][:, :Gh], host["U"], rtol=0, atol=4 * A * 2.0 ** -53 * np.abs(host["U"]).max() * A))
        r = {"genes": G, "assemblies": A, "traits": T, "cov": a.cov, "segments": segs, "entry_wall_ms": round(min(walls) * 1e3, 2), "sums_ms": sums_ms, "stat_ms": stat_ms,
             "sums_tflops_fp64": round(flop / (sums_ms * 1e-3) / 1e12, 2) if sums_ms else None, "sums_min_tb_per_s": round(byts / (sums_ms * 1e-3) / 1e12, 3) if sums_ms else None,
             "host_loop_one_core_ms": round(host_ms, 1) if host_ms else None, "host_genes_run": Gh, "host_agrees": same}
        print(json.dumps(r), flush=True)
        res.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
