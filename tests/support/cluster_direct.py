"""TEST INFRASTRUCTURE: direct pg_pan_medoids / pg_pan_cluster cases for tests/test_cluster_gpu.py, run in a child process of their own so
that the test can bound them with a timeout.  The product library (HIP kernels of k_medoids.hpp) clusters matrices no GFA fixture
reaches; the numpy restatement (tests/support/cluster_ref.py) checks them where that is affordable, the checker build (host loops of
tree.cpp) where it is not.  Prints one line per case and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/cluster_direct.py {sizes|large|uneven|ties|chunks|cached|magnitude}"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cluster_ref as cr  # noqa: E402
import dist_ref as dr  # noqa: E402
import tree_ref as tr  # noqa: E402


def report(label, n, k, ok, note=""):
    print("%s n=%d k=%d%s: %s" % (label, n, k, note, "ok" if ok else "DIFFERENT"), flush=True)
    if not ok:
        sys.exit(1)


def uneven(n, seed):
    """about nine tenths of the columns in one tight cluster, the others far from it and from each other"""
    rng = np.random.default_rng(seed)
    n_big = n * 9 // 10
    pts = np.concatenate([rng.integers(0, 50, size=(n_big, 2)), 1000 + 400 * np.arange(n - n_big)[:, None] + rng.integers(0, 30, size=(n - n_big, 2))])
    pts = pts[rng.permutation(n)]
    return (np.abs(pts[:, None, :] - pts[None, :, :]).sum(axis=2) << 10).astype(np.int32)


def main():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    from pangene_amd import capi
    import oracle_host
    hip, ora = capi.load(), oracle_host.load()
    which = sys.argv[1]
    if which == "sizes":  # across a wave (64), a tile of candidates (256) and two of them, against the restatement
        swaps = 0
        for n in (3, 63, 64, 65, 255, 256, 257, 513):
            for k in sorted({2, 3, 17} | ({n - 1} if n <= 65 else set())):
                if not 2 <= k <= n - 1:
                    continue
                q = cr.planted(n, 5, n + k) if k == 3 else cr.random_matrix(n, n + k, hi=1 << 12)
                want = cr.medoids(q, k)
                swaps += want["n_swap"]
                report("sizes", n, k, want["converged"] == 1 and cr.same(capi.pan_medoids(hip, q, k), want), " swaps=%d" % want["n_swap"])
        report("sizes: some input swapped", 0, 0, swaps >= 8)
    elif which == "large":  # past 1 024 columns, and k at its limit (the acc buffer at 1 024 x n): against the checker build only
        for n, k in ((1025, 16), (1100, 1024)):
            q = cr.random_matrix(n, n, hi=1 << 16)
            want = capi.pan_medoids(ora, q, k)
            report("large", n, k, want["converged"] == 1 and cr.same(capi.pan_medoids(hip, q, k), want), " swaps=%d" % want["n_swap"])
        try:
            capi.pan_medoids(hip, np.zeros((1100, 1100), dtype=np.int32), 1025)
            report("k = 1 025 accepted", 1100, 1025, False)
        except RuntimeError as e:
            report("k = 1 025 refused", 1100, 1025, "status -2" in str(e))
    elif which == "uneven":  # one row a chunk: chunks cross cluster boundaries, and hundreds of workgroups add into the big cluster's sums
        os.environ["PANGENE_MEDOIDS_ROWS"] = "1"
        q = uneven(600, 3)
        for k in (8, 61):
            want = cr.medoids(q, k)
            got = capi.pan_medoids(hip, q, k)
            report("uneven", 600, k, cr.same(got, want) and (k != 8 or int(got["size"].max()) >= 500), " largest=%d swaps=%d" % (got["size"].max(), got["n_swap"]))
        os.environ["PANGENE_MEDOIDS_ROWS"] = "7"
        report("uneven rows=7", 600, 8, cr.same(capi.pan_medoids(hip, q, 8), cr.medoids(q, 8)))
    elif which == "ties":  # all-equal distances (every tie rule decides), and copies of columns (zero distances, medoids that are copies)
        for n, k in ((5, 2), (200, 7), (300, 299)):
            q = np.full((n, n), 3 << 18, dtype=np.int32)
            np.fill_diagonal(q, 0)
            got = capi.pan_medoids(hip, q, k)
            report("equal", n, k, cr.same(got, cr.medoids(q, k)) and got["medoid"].tolist() == list(range(k)))
        base = cr.planted(40, 3, 9)
        idx = np.random.default_rng(4).integers(0, 40, size=300)
        q = base[np.ix_(idx, idx)].astype(np.int32)
        for k in (2, 30, 60):  # (60: more medoids than distinct rows)
            got = capi.pan_medoids(hip, q, k)
            report("copies", 300, k, cr.same(got, cr.medoids(q, k)) and bool((got["size"] >= 1).all()) and got["label"][got["medoid"]].tolist() == list(range(k)))
        P = tr.lineage_presence(2000, 130, 7, dup=0.4)
        for metric in tr.METRICS:
            qq, F = tr.fixed(dr.shared(P), metric)
            got, F2 = capi.pan_cluster(hip, P, 6, metric)
            report("presence " + metric, 130, 6, F2 == F and cr.same(got, cr.medoids(qq, 6)))
    elif which == "chunks":  # iterations queued one by one and eight at a time: the same records; a limit inside a chunk
        q = cr.random_matrix(300, 1)
        want = cr.medoids(q, 8)
        report("chunks: the input swaps", 300, 8, want["n_swap"] >= 3, " swaps=%d" % want["n_swap"])
        for batch in ("1", "8", "3"):
            os.environ["PANGENE_MEDOIDS_BATCH"] = batch
            report("chunks batch=" + batch, 300, 8, cr.same(capi.pan_medoids(hip, q, 8), want))
            for it in (0, 1, 2, 4):
                report("chunks batch=%s max_iter=%d" % (batch, it), 300, 8, cr.same(capi.pan_medoids(hip, q, 8, max_iter=it), cr.medoids(q, 8, it)))
    elif which == "magnitude":  # entries in the upper half of the range: gain, removal, acc, plus, td and sums are far beyond 32 bits
        for label, q, k, swaps in cr.magnitude_inputs():
            want = cr.medoids(q, k)
            big = max(int(want["td"]), int(want["sums"].max()), int(np.abs(want["rec"][:, 2]).max())) > 1 << 35
            report("magnitude, " + label, q.shape[0], k, big and want["converged"] == 1 and (swaps is None or want["n_swap"] >= swaps) and
                   cr.same(capi.pan_medoids(hip, q, k), want), " swaps=%d td=%d" % (want["n_swap"], want["td"]))
        n, k = cr.MAGNITUDE_CHECKER
        q = cr.full_random(n, n + k)
        want = capi.pan_medoids(ora, q, k)
        report("magnitude, uniform, checker build", n, k, want["converged"] == 1 and want["td"] > 1 << 37 and cr.same(capi.pan_medoids(hip, q, k), want),
               " swaps=%d td=%d" % (want["n_swap"], want["td"]))
    elif which == "cached":  # the cached device buffers: growing, shrinking and growing again in one process
        for i, (n, k) in enumerate(((40, 3), (700, 20), (3, 2), (257, 200), (1030, 5), (64, 63), (700, 2))):
            q = cr.random_matrix(n, 20 + i, hi=1 << 14)
            report("cached", n, k, cr.same(capi.pan_medoids(hip, q, k), capi.pan_medoids(ora, q, k)))
        hip.pg_trim_host_cache(0)  # gives the buffers back; the next call allocates again
        q = cr.random_matrix(300, 99)
        report("after trim", 300, 9, cr.same(capi.pan_medoids(hip, q, 9), capi.pan_medoids(ora, q, 9)))
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
