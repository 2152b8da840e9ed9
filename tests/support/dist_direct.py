"""TEST INFRASTRUCTURE: direct pg_pan_shared cases for tests/test_dist_gpu.py, run in a child process of their own so that the test can
bound them with a timeout.  The product library (HIP kernel) runs matrices no GFA fixture reaches; the checker build (host loops) and
the numpy restatement check them where that is affordable, invariants and 64 sampled rows where it is not.  Prints one line per case
and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/dist_direct.py {large|sizes|edges}"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import assoc_ref as ar  # noqa: E402
import dist_ref as dr  # noqa: E402


def presence(M, A, seed):
    """(M, A) bool, every assembly with a density of its own (0 .. 0.6)"""
    rng = np.random.default_rng(seed)
    dens = rng.random(A).astype(np.float32) * 0.6
    P = np.empty((M, A), dtype=bool)
    for m0 in range(0, M, 4096):  # in slabs: a float matrix of the whole shape would not fit
        P[m0:m0 + 4096] = rng.random((min(4096, M - m0), A), dtype=np.float32) < dens
    return P


def check_sampled(S, P, label):
    """symmetry, the diagonal = column counts, S <= min(n_i, n_j), and 64 rows exactly as float32 B[r] @ B.T (counts < 2^24)"""
    M, A = P.shape
    n = P.sum(0, dtype=np.int64)
    ok = S.shape == (A, A) and np.array_equal(S, S.T) and np.array_equal(np.diag(S), n)
    ok = ok and bool((S <= np.minimum(n[:, None], n[None, :])).all()) and bool((S >= 0).all())
    rows = np.random.default_rng(A).choice(A, size=min(64, A), replace=False)
    R = P[:, rows].T.astype(np.float32)  # (64, M)
    for a0 in range(0, A, 1024):
        blk = P[:, a0:a0 + 1024].astype(np.float32)  # (M, <= 1024)
        ok = ok and np.array_equal((R @ blk).astype(np.int64), S[rows, a0:a0 + 1024].astype(np.int64))
    print("%s M=%d A=%d: %s" % (label, M, A, "ok" if ok else "DIFFERENT"), flush=True)
    if not ok:
        sys.exit(1)


def check_exact(hip, ora, P, label):
    from pangene_amd import capi
    got = capi.pan_shared(hip, P)
    ok = np.array_equal(got, dr.shared(P)) and np.array_equal(got, capi.pan_shared(ora, P))
    for m in dr.METRICS:
        ok = ok and np.array_equal(capi.pan_dist(hip, P, m), dr.metric(dr.shared(P), m))
    print("%s M=%d A=%d: %s" % (label, P.shape[0], P.shape[1], "ok" if ok else "DIFFERENT"), flush=True)
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
        P = presence(70001, 12003, 1)  # 94 x 94 tiles, 69 K chunks, the last one partial
        check_sampled(capi.pan_shared(hip, P), P, "large")
        del P
        P = presence(60013, 200, 2)  # 3 tiles: the K chunks are split over workgroups that add into S
        check_exact(hip, ora, P, "split K")
        P = presence(5000, 1500, 3)
        check_sampled(capi.pan_shared(hip, torch.from_numpy(P).cuda()), P, "torch cuda tensor")
    elif which == "edges":
        # the shapes at which the tile body can go wrong: every row count against every row length, rows of every density in each; at
        # A <= 128 there is one tile, so the rows of 33 and 65 words run split K in 2 and 3 slices that add into a zeroed S
        for A in ar.EDGE_ROWS:
            for M in ar.EDGE_COLS + (33 * 32, 65 * 32):
                check_exact(hip, ora, ar.edge_rows(A, M, A + M).T, "edges")
    else:
        # the cached device buffers: growing, shrinking and growing again in one process
        for i, (M, A) in enumerate([(40, 50), (3000, 700), (10, 2), (0, 9), (7, 0), (0, 0), (1, 1), (33, 129), (4097, 257),
                                    (3000, 700), (64, 1), (100000, 3), (31, 1000)]):
            check_exact(hip, ora, presence(M, A, 10 + i), "sizes")
        hip.pg_trim_host_cache(0)  # gives the buffers back; the next call allocates again
        check_exact(hip, ora, presence(500, 300, 99), "after trim")
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
