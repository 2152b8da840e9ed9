"""TEST INFRASTRUCTURE: direct pg_pan_curves cases for tests/test_curves_gpu.py, run in a child process of their own so that the test can
bound them with a timeout.  The product library (HIP kernels) and the checker build (host loops) run the same matrices in one process; the
numpy restatement checks a few orders of each.  Prints one line per case and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/curves_direct.py {large|sizes}"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import curves_ref as cr  # noqa: E402


def check(hip, ora, P, n, seed, perms, label):
    from pangene_amd import capi
    got = capi.pan_curves(hip, P, n_perm=n, seed=seed)
    want = capi.pan_curves(ora, P, n_perm=n, seed=seed)
    ok = np.array_equal(got, want)
    for p in perms:
        if p < n:
            ok = ok and np.array_equal(got[:, p, :], cr.curves_one(P, cr.order(P.shape[1], p, seed)))
    G, A = P.shape
    if ok and A:
        pan, core, new, uniq = got.astype(np.int64)
        ok = bool((np.diff(pan, axis=1) >= 0).all() and (np.diff(core, axis=1) <= 0).all() and (new.sum(1) == pan[:, -1]).all()
                  and (uniq <= pan).all() and (pan <= G).all())
    print("%s G=%d A=%d n=%d: %s" % (label, G, A, n, "ok" if ok else "DIFFERENT"), flush=True)
    if not ok:
        sys.exit(1)


def main():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    from pangene_amd import capi
    import oracle_host
    hip, ora = capi.load(), oracle_host.load()
    which = sys.argv[1]
    if which == "large":
        # past the LDS histogram form (ranks >= 4 095 go to the global histograms), U-shaped: core plus cloud
        check(hip, ora, cr.u_shaped(3000, 20000, 1), 100, 11, [0, 57], "u-shaped")
        check(hip, ora, cr.u_shaped(60000, 200, 2), 100, 11, [0, 1, 99], "many genes")
        check(hip, ora, np.random.default_rng(3).random((100, 1)) < 0.5, 5, 11, [0, 4], "one column")
        P = cr.u_shaped(400, 70, 4)
        t = torch.from_numpy(P).cuda()
        assert np.array_equal(capi.pan_curves(hip, t, n_perm=3), capi.pan_curves(ora, P, n_perm=3))
        print("torch cuda tensor: ok", flush=True)
    else:
        # the cached device buffers: growing, shrinking and growing again in one process
        rng = np.random.default_rng(5)
        for G, A, n in [(50, 40, 3), (3000, 5000, 20), (20, 10, 2), (60000, 200, 10), (1, 1, 1), (0, 5, 2), (7, 0, 2), (500, 300, 7),
                        (3000, 5000, 20), (2, 33, 4), (800, 4095, 3), (800, 4096, 3), (10, 64, 1)]:
            P = cr.u_shaped(G, A, int(rng.integers(1 << 30))) if G and A else np.zeros((G, A), dtype=bool)
            check(hip, ora, P, n, int(rng.integers(1 << 32)), [0, n - 1], "sizes")
        hip.pg_trim_host_cache(0)  # gives the buffers back; the next call allocates again
        check(hip, ora, cr.u_shaped(300, 100, 9), 4, 1, [0, 3], "after trim")
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
