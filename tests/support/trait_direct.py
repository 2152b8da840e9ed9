"""TEST INFRASTRUCTURE: direct pg_pan_trait / pga_pan_trait cases for tests/test_trait_gpu.py, run in a child process of their own so that
the test can bound them with a timeout.  The product library (HIP kernels) runs matrices no GFA fixture reaches, and the numpy
restatement (tests/support/trait_ref.py) checks a, s and k of every gene and trait completely, never a sample.  Prints one line per
case and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/trait_direct.py {large|batches|sizes|rows|edges|wide} [--cpu-only]

--cpu-only runs the checker build against the restatement instead (to see that the cases stay affordable without a GPU)."""
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import assoc_ref as ar  # noqa: E402
import trait_ref as tr  # noqa: E402


class pga_trait_in_t(C.Structure):
    _fields_ = [("bits", C.c_void_p), ("label", C.c_void_p), ("n_gene", C.c_int32), ("n_col", C.c_int32), ("min_count", C.c_int32), ("n_perm", C.c_int32),
                ("seed", C.c_uint32), ("perm_rows", C.c_void_p)]


class pga_trait_out_t(C.Structure):
    _fields_ = [("a", C.POINTER(C.c_int32)), ("s", C.POINTER(C.c_int32)), ("k", C.POINTER(C.c_int32))]


def check(lib, P, L, label, given=None, **kw):
    from pangene_amd import capi
    t0 = time.perf_counter()
    want = tr.pan_trait(P, L, **kw)
    t_ref = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = capi.pan_trait(lib, P if given is None else given[0], L if given is None else given[1], **kw)
    t_lib = time.perf_counter() - t0
    ok = all(got[key].shape == want[key].shape and np.array_equal(got[key], want[key]) for key in want)
    print("%s G=%d A=%d T=%d %s: sum k = %d, restatement %.1f s, library %.2f s: %s" % (
        label, P.shape[0], P.shape[1], np.atleast_2d(L).shape[0], kw, int(want["k"].sum()), t_ref, t_lib, "ok" if ok else "DIFFERENT"), flush=True)
    if not ok:
        for key in want:
            bad = np.argwhere(got[key] != want[key]) if got[key].shape == want[key].shape else []
            if len(bad):
                print("  %s: %d differ, first at %s: got %d, want %d" % (key, len(bad), bad[0].tolist(), got[key][tuple(bad[0])], want[key][tuple(bad[0])]))
        sys.exit(1)
    return want


def labels(P, seed, planted_rows=()):
    """(T, A) int8: the presence rows asked for and their complements, a random trait, and one with missing values"""
    rng = np.random.default_rng(seed)
    A = P.shape[1]
    rows = []
    for g in planted_rows:
        rows += [P[g].astype(np.int8), (~P[g]).astype(np.int8)]
    rows.append(rng.integers(0, 2, size=A).astype(np.int8))
    gaps = rng.integers(0, 2, size=A).astype(np.int8)
    gaps[rng.random(A) < 0.2] = -1
    rows.append(gaps)
    return np.stack(rows)


def perm_rows(lib, y, n, seed):
    """the label rows of the first batch as the device made them: (n, W) uint32"""
    N = len(y)
    W = (N + 31) // 32
    lab = np.ascontiguousarray(tr.pack(np.asarray(y, dtype=np.uint8)[None, :])[0])
    rows = np.zeros((n, W), dtype=np.uint32)
    a = pga_trait_in_t(None, lab.ctypes.data, 0, N, 1, n, seed, rows.ctypes.data)
    out = pga_trait_out_t()
    lib.pga_pan_trait.restype = C.c_int
    rc = lib.pga_pan_trait(C.byref(a), C.byref(out))
    assert rc == 0, rc
    return rows


def main():
    which = sys.argv[1]
    cpu_only = "--cpu-only" in sys.argv[2:]
    from pangene_amd import capi
    if cpu_only:
        import oracle_host
        lib, batch = oracle_host.load(), 65536
    else:
        import torch
        assert torch.cuda.is_available()
        torch.cuda.init()
        lib = capi.load()
        lib.pga_trait_batch.restype = C.c_int32
        batch = int(lib.pga_trait_batch())  # read from the library, PANGENE_TRAIT_BATCH included
    if which == "large":
        P = ar.planted(20003, 1001, 1, n_module=40)  # 32 words a row, the last partial; 157 gene tiles, the last partial
        cnt = P.sum(axis=1)
        g = int(np.argmin(np.abs(cnt - 500)))
        L = labels(P, 2, planted_rows=(g,))
        want = check(lib, P, L, "large", n_perm=2000)
        assert want["k"][0, g] == 0 and want["k"][1, g] == 0 and int(want["k"].sum()) > 0
    elif which == "batches":
        P = ar.planted(300, 40, 3)
        L = labels(P, 4)[:1]
        for n in (batch - 1, batch, batch + 1, 3 * batch + 5):
            check(lib, P, L, "batches (batch = %d)" % batch, n_perm=n, min_count=2)
    elif which == "sizes":
        # N past the LDS form of k_trait_perm (W > 128 words): the rows live in global memory
        P = ar.planted(700, 4200, 5)
        check(lib, P, labels(P, 6)[:1], "global-memory rows", n_perm=200)
        # the cached device buffers: growing, shrinking and growing again in one process
        for i, (G, A) in enumerate([(40, 50), (3000, 700), (10, 2), (0, 9), (7, 0), (1, 1), (2, 4), (129, 33), (257, 4097), (3000, 700), (1, 64), (50000, 9), (1000, 31)]):
            P = ar.planted(G, A, 10 + i)
            check(lib, P, labels(P, 20 + i), "sizes", n_perm=130 if A < 4000 else 70, seed=7)
        if not cpu_only:
            import torch
            Q = ar.planted(3000, 500, 3)
            LQ = labels(Q, 8)
            check(lib, Q, LQ, "torch cuda tensors", given=(torch.from_numpy(Q).cuda(), torch.from_numpy(LQ).cuda()), n_perm=300)
            lib.pg_trim_host_cache(0)  # gives the buffers back; the next call allocates again
        P = ar.planted(500, 300, 99)
        check(lib, P, labels(P, 9), "after trim", n_perm=100, min_count=3)
    elif which == "edges":
        # the shapes at which the tile body can go wrong: every gene count against every row length, 129 permutations in batches of 128,
        # so that the second batch is one row of a second permutation tile; product and checker build against the restatement
        import oracle_host
        ora = oracle_host.load()
        os.environ["PANGENE_TRAIT_BATCH"] = "128"
        for A in ar.EDGE_COLS:
            y = (np.random.default_rng(A).random(A) < 0.4).astype(np.int8)
            if A > 1:
                y[0], y[-1] = 1, 0  # both values occur
            for G in ar.EDGE_ROWS:
                P = ar.edge_rows(G, A, G + A)
                want = check(lib, P, y, "edges", n_perm=129, seed=5)
                got = capi.pan_trait(ora, P, y, n_perm=129, seed=5)
                assert all(np.array_equal(got[key], want[key]) for key in want), "checker build differs"
        del os.environ["PANGENE_TRAIT_BATCH"]
    elif which == "wide":
        # thresholds whose 64-bit products pass 2^31, equality on either side, D = 0 and the largest |D| (trait_ref.wide_inputs); 70 000
        # dependent swaps a lane in the global-memory form of the permutation kernel, whose rows are compared as well
        import oracle_host
        ora = oracle_host.load()
        for label, P, y, must in tr.wide_inputs():
            want = check(lib, P, y, label, n_perm=tr.WIDE_PERM)
            assert all(int(want["k"][0, g]) == k for g, k in must.items()), "the restatement misses a count the input was built for"
            if not cpu_only:
                got = capi.pan_trait(ora, P, y, n_perm=tr.WIDE_PERM)
                assert all(np.array_equal(got[key], want[key]) for key in want), "checker build differs"
                t0 = time.perf_counter()
                rows = perm_rows(lib, (y != 0).astype(np.uint8), tr.WIDE_PERM, 11)
                ok = np.array_equal(rows, tr.pack(tr.perm_labels(y, tr.WIDE_PERM, 11)))
                print("%s: %d permuted rows, library %.2f s: %s" % (label, tr.WIDE_PERM, time.perf_counter() - t0, "ok" if ok else "DIFFERENT"), flush=True)
                if not ok:
                    sys.exit(1)
    elif which == "rows":
        # the permuted label rows themselves: pins the device's 64-bit %
        assert not cpu_only
        for N in (31, 64, 1000, 4200):
            y = (np.random.default_rng(N).random(N) < 0.4).astype(np.uint8)
            for seed in (11, 0xFFFFFFFF):
                got = perm_rows(lib, y, 64, seed)
                want = tr.pack(tr.perm_labels(y, 64, seed))
                ok = np.array_equal(got, want)
                print("rows N=%d seed=%d: %s" % (N, seed, "ok" if ok else "DIFFERENT"), flush=True)
                if not ok:
                    sys.exit(1)
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
