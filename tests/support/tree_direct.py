"""TEST INFRASTRUCTURE: direct pg_pan_join / pg_pan_tree cases for tests/test_tree_gpu.py, run in a child process of their own so that
the test can bound them with a timeout.  The product library (HIP kernels of k_join.hpp) joins matrices no GFA fixture reaches; the
numpy restatement (tests/support/tree_ref.py) checks them where that is affordable, the checker build (host loops of tree.cpp) where it
is not.  Prints one line per case and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/tree_direct.py {sizes|large|cached|equal|presence|parts}"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dist_ref as dr  # noqa: E402
import tree_ref as tr  # noqa: E402

# (A, method) -> (items, seed, share of exact copies): inputs for which the restatement meets a tied minimum.  The sizes cross a wave
# (64), a tile's rows (16), the update kernel's workgroup (256) and, from 513 on, several row blocks per column chunk.
SIZES = {
    (3, "nj"): (40, 1, 0.5), (3, "upgma"): (40, 2, 0.5), (4, "nj"): (40, 1, 0.5), (4, "upgma"): (40, 2, 0.5),
    (5, "nj"): (40, 1, 0.5), (5, "upgma"): (40, 2, 0.5), (63, "nj"): (500, 1, 0.15), (63, "upgma"): (500, 1, 0.15),
    (64, "nj"): (500, 1, 0.15), (64, "upgma"): (500, 1, 0.15), (65, "nj"): (500, 1, 0.15), (65, "upgma"): (500, 1, 0.15),
    (127, "nj"): (800, 1, 0.15), (127, "upgma"): (800, 1, 0.15), (128, "nj"): (800, 1, 0.15), (128, "upgma"): (800, 1, 0.15),
    (129, "nj"): (800, 1, 0.15), (129, "upgma"): (800, 1, 0.15), (257, "nj"): (1000, 1, 0.15), (257, "upgma"): (1000, 1, 0.15),
    (513, "nj"): (1500, 1, 0.15), (513, "upgma"): (1500, 1, 0.15), (600, "nj"): (1500, 1, 0.15), (600, "upgma"): (1500, 1, 0.15),
}


def matrix(M, A, seed, dup=0.15, metric=None):
    P = tr.lineage_presence(M, A, seed, dup=dup)
    q, _ = tr.fixed(dr.shared(P), metric or ("jaccard" if A % 2 else "diff"))
    return q.astype(np.int32)


def report(label, A, method, ok):
    print("%s A=%d %s: %s" % (label, A, method, "ok" if ok else "DIFFERENT"), flush=True)
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
    if which == "sizes":
        for (A, method), (M, seed, dup) in sorted(SIZES.items()):
            q = matrix(M, A, seed, dup)
            stats = {}
            want = tr.joins(q, method, stats)
            if not (A == 3 and method == "nj") and stats["n_tied"] < 1:
                report("no tied minimum in the input", A, method, False)
            report("sizes", A, method, np.array_equal(capi.pan_join(hip, q, method), want))
    elif which == "large":  # past one column chunk of 1 024, and 2 049: against the checker build only
        for A in (1025, 2049):
            q = matrix(600, A, A)
            for method in tr.METHODS:
                report("large", A, method, np.array_equal(capi.pan_join(hip, q, method), capi.pan_join(ora, q, method)))
    elif which == "cached":  # the cached device buffers: growing, shrinking and growing again in one process
        for i, A in enumerate((40, 700, 3, 257, 1030, 64)):
            q = matrix(300, A, 20 + i)
            for method in tr.METHODS:
                report("cached", A, method, np.array_equal(capi.pan_join(hip, q, method), capi.pan_join(ora, q, method)))
        hip.pg_trim_host_cache(0)  # gives the buffers back; the next call allocates again
        q = matrix(300, 300, 99)
        report("after trim", 300, "nj", np.array_equal(capi.pan_join(hip, q, "nj"), capi.pan_join(ora, q, "nj")))
    elif which == "equal":  # every distance the same: every criterion ties at every join and the label rule alone decides the tree
        for A in (5, 200):
            q = np.full((A, A), 3 << 18, dtype=np.int32)
            np.fill_diagonal(q, 0)
            for method in tr.METHODS:
                stats = {}
                want = tr.joins(q, method, stats)
                report("equal", A, method, stats["n_tied"] >= A - 3 and np.array_equal(capi.pan_join(hip, q, method), want))
    elif which == "presence":  # pg_pan_tree: presence bytes -> pan_shared -> fixed point -> joins, all in the product
        P = tr.lineage_presence(2000, 130, 7)
        for metric in tr.METRICS:
            q, F = tr.fixed(dr.shared(P), metric)
            for method in tr.METHODS:
                rec, F2 = capi.pan_tree(hip, P, metric, method)
                report("presence " + metric, 130, method, F2 == F and np.array_equal(rec, tr.joins(q, method)))
        rec, _ = capi.pan_tree(hip, torch.from_numpy(P).cuda(), "jaccard", "nj")
        report("torch cuda tensor", 130, "nj", np.array_equal(rec, tr.joins(tr.fixed(dr.shared(P), "jaccard")[0], "nj")))
    elif which == "parts":  # few workgroups in the search: each strides over several tiles, some of them below the diagonal
        os.environ["PANGENE_JOIN_PARTS"] = "7"
        q = matrix(1500, 600, 1)
        for method in tr.METHODS:
            report("parts", 600, method, np.array_equal(capi.pan_join(hip, q, method), capi.pan_join(ora, q, method)))
        q = matrix(600, 1025, 5)
        report("parts", 1025, "nj", np.array_equal(capi.pan_join(hip, q, "nj"), capi.pan_join(ora, q, "nj")))
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
