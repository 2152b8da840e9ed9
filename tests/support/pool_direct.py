"""TEST INFRASTRUCTURE: the device buffer pools of the seven context-free pga_pan_* entries (pga_host_pan.hpp) for
tests/test_pan_pool_gpu.py, run in a child process of its own so that the test can bound it with a timeout.  Every entry is called
through capi at a tiny shape, pg_trim_host_cache(0) gives every pool back, and the same calls follow at a larger and then a smaller
shape: every result must equal the restatement's.  That a release reaches every pool, that a released pool allocates again, and that a
pool grows and is then reused at a smaller size all show here.  Prints one line per call and "ALL OK" at the end; exits 1 at the first
difference.

    python tests/support/pool_direct.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import assoc_ref as ar  # noqa: E402
import boot_ref as br  # noqa: E402
import curves_ref as cr  # noqa: E402
import dist_ref as dr  # noqa: E402
import pairs_ref as pr  # noqa: E402
import trait_ref as tr  # noqa: E402
import tree_ref as tref  # noqa: E402


def same(got, want):
    return all(np.array_equal(got[key], want[key]) for key in want)


def all_entries(lib, G, A, seed):
    """one call of each entry on a (G, A) gene x assembly matrix (its transpose where the assemblies are the rows); A >= 3"""
    from pangene_amd import capi
    rng = np.random.default_rng(seed)
    P = ar.planted(G, A, seed)
    y = rng.integers(0, 2, size=A).astype(np.int8)
    y[:2] = (0, 1)
    S = dr.shared(P)
    q = tref.fixed(S, "jaccard")[0]
    rec = tref.joins(q, "nj")
    want_pairs, cnt = ar.select(P, 0.5, 1)
    got_pairs, got_phi = capi.pan_assoc(lib, P, min_phi=0.5, min_count=1)
    results = {
        "curves": np.array_equal(capi.pan_curves(lib, P, n_perm=3, seed=2), cr.curves(P, n_perm=3, seed=2)),
        "shared": np.array_equal(capi.pan_shared(lib, P), S),
        "assoc": np.array_equal(got_pairs, want_pairs) and np.array_equal(got_phi, ar.phi(want_pairs, cnt, A)),
        "trait": same(capi.pan_trait(lib, P, y, n_perm=70, seed=3), tr.pan_trait(P, y, n_perm=70, seed=3)),
        "join": np.array_equal(capi.pan_join(lib, q, "nj"), rec),
        "boot": np.array_equal(capi.pan_boot_records(lib, P, "jaccard", "upgma", seed=4, first=1, n=2), br.records(P, "jaccard", "upgma", 4, 1, 2)),
        "pairs": same(capi.pan_pairs(lib, P, y, rec, "nj"), pr.counts(P, y[None, :], rec, "nj")),
    }
    for name, ok in results.items():
        print("%s G=%d A=%d: %s" % (name, G, A, "ok" if ok else "DIFFERENT"), flush=True)
        if not ok:
            sys.exit(1)


def main():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    from pangene_amd import capi
    hip = capi.load()
    all_entries(hip, 9, 5, 1)
    hip.pg_trim_host_cache(0)
    all_entries(hip, 300, 140, 2)  # every pool allocates again, larger than before
    all_entries(hip, 20, 7, 3)     # and is reused at a smaller size
    hip.pg_trim_host_cache(0)
    all_entries(hip, 20, 7, 3)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
