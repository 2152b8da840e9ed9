"""TEST INFRASTRUCTURE: direct pga_pan_permanova / pg_pan_permanova cases for tests/test_permanova_gpu.py, run in a child process of their
own so that the test can bound them with a timeout.  The product library (HIP kernels, the int8 MFMA kernel k_perma_quad among them) runs
matrices no GFA fixture reaches, and the numpy / Python-int restatement (tests/support/permanova_ref.py) checks T, A, B and k and, through
the tests-only a_rows / b_rows / perm_rows pointers of pga_permanova_in_t, A_p, B_p and the label row of EVERY permutation of the first
batch, never a sample.  Prints one line per case and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/permanova_direct.py {maps|tiles|digits|ties|magnitude|batches|large|buffers|range}"""
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
import permanova_ref as pr  # noqa: E402
import trait_ref as tr  # noqa: E402

PGA_ERR_RANGE = -2


class pga_permanova_in_t(C.Structure):
    _fields_ = [("q", C.c_void_p), ("label", C.c_void_p), ("n", C.c_int32), ("shift", C.c_int32), ("q_max", C.c_int32), ("n1", C.c_int32), ("n_perm", C.c_int32),
                ("seed", C.c_uint32), ("a_rows", C.c_void_p), ("b_rows", C.c_void_p), ("perm_rows", C.c_void_p)]


class pga_permanova_out_t(C.Structure):
    _fields_ = [("t", C.c_int64), ("a", C.c_int64), ("b", C.c_int64), ("k", C.c_int64)]


def fail(msg):
    print(msg, flush=True)
    sys.exit(1)


def direct(lib, qc, y, n, seed=11, batch=None, rows=True):
    """pga_pan_permanova on qc (N, N) and y (N,) 0/1: dict T, A, B, k and, with rows, a_rows, b_rows (nb,) and perm_rows (nb, W) of the first
    batch; or the status when it is not 0"""
    q = np.ascontiguousarray(qc, dtype=np.int32)
    y = np.asarray(y, dtype=np.uint8)
    N = len(y)
    W = (N + 31) // 32
    label = np.ascontiguousarray(tr.pack(y[None, :])[0])
    m = int(q.max()) if q.size else 0
    nb = max(min(n, batch if batch is not None else n), 1)
    ar, br = np.full(nb, -7, dtype=np.int64), np.full(nb, -7, dtype=np.int64)
    rw = np.full((nb, W), 0xFFFFFFFF, dtype=np.uint32)
    a = pga_permanova_in_t(q.ctypes.data, label.ctypes.data, N, pr.shift_of(m, N), m, int(y.sum()), n, seed, ar.ctypes.data if rows else None,
                           br.ctypes.data if rows else None, rw.ctypes.data if rows else None)
    out = pga_permanova_out_t()
    lib.pga_pan_permanova.restype = C.c_int
    rc = lib.pga_pan_permanova(C.byref(a), C.byref(out))
    if rc != 0:
        return rc
    res = {"T": out.t, "A": out.a, "B": out.b, "k": out.k}
    if rows:
        nb = min(n, nb)
        res.update(a_rows=ar[:nb], b_rows=br[:nb], perm_rows=rw[:nb])
    return res


def check(lib, qc, y, n, label, seed=11, batch=None):
    y = np.asarray(y, dtype=np.uint8)
    N = len(y)
    nb = min(n, batch if batch is not None else n)
    t0 = time.perf_counter()
    want = pr.direct(qc, y, n, seed, rows=max(nb, 1))
    t_ref = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = direct(lib, qc, y, n, seed, batch)
    t_lib = time.perf_counter() - t0
    if not isinstance(got, dict):
        fail("%s: status %d" % (label, got))
    bad = [key for key in ("T", "A", "B", "k") if got[key] != want[key]]
    if nb:
        if not np.array_equal(got["perm_rows"], tr.pack(tr.perm_labels(y, nb, seed))):
            bad.append("perm_rows")
        bad += [key for key in ("a_rows", "b_rows") if not np.array_equal(got[key], want[key][:nb])]
    print("%s N=%d n1=%d n=%d s=%d D=%d: A = %d, k = %d, restatement %.2f s, library %.3f s: %s" % (
        label, N, int(y.sum()), n, want["s"], pr.planes_of(int(pr.weights(qc, want["s"]).max())), want["A"], want["k"], t_ref, t_lib,
        "DIFFERENT in " + ", ".join(bad) if bad else "ok"), flush=True)
    if bad:
        key = bad[0]
        if key in ("a_rows", "b_rows"):
            at = np.nonzero(got[key] != want[key][:nb])[0]
            fail("  %s: %d of %d differ, first at %d: got %d, want %d" % (key, len(at), nb, at[0], got[key][at[0]], want[key][at[0]]))
        fail("  %s: got %s, want %s" % (key, got.get(key), want.get(key)))
    return got, want


def groups(N, seed, n1=None):
    rng = np.random.default_rng(seed)
    y = np.zeros(N, dtype=np.uint8)
    y[rng.permutation(N)[:n1 if n1 else max(N // 2, 1)]] = 1
    return y


def main():
    which = sys.argv[1]
    from pangene_amd import capi
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    lib = capi.load()
    lib.pga_permanova_batch.restype = C.c_int32
    batch = int(lib.pga_permanova_batch())  # read from the library, PANGENE_PERMA_BATCH included
    if which == "maps":
        # the lane maps, the mask and the symmetry doubling: every w distinct, so a value that lands in the wrong row, column or order shows
        N = 200
        q = pr.distinct_matrix(N)
        w = pr.weights(q, 0)
        assert len(np.unique(w[np.triu_indices(N, 1)])) == N * (N - 1) // 2
        check(lib, q, groups(N, 1), 130, "maps")
        check(lib, q, groups(N, 2, 7), 130, "maps, 7 ones")
    elif which == "tiles":
        for N in (3, 63, 64, 65, 127, 128, 129, 255, 257, 300):
            q = pr.random_matrix(N, N, hi=1 << 16)
            for n in (1, 127, 129):
                check(lib, q, groups(N, N + n, 1 if n == 1 else None), n, "tiles", seed=5)
    elif which == "digits":
        for D in (1, 2, 3, 5, 8):
            N = 8 if D == 8 else 140
            q = pr.digit_matrix(N, D, D)
            assert pr.shift_of(q.max(), N) == 0 and pr.planes_of(int(pr.weights(q, 0).max())) == D
            check(lib, q, groups(N, D), 140, "digits D=%d" % D)
        q = pr.digit_matrix(140, 3, 9, zero_plane=1)
        dg = pr.digits(pr.weights(q, 0), 3)
        assert not dg[1].any() and dg[0].any() and dg[2].any()
        check(lib, q, groups(140, 9), 140, "digits: an all-zero middle plane")
    elif which == "ties":
        N = 150
        q = pr.random_matrix(N, 1, hi=3) << 10
        _, want = check(lib, q, groups(N, 1), 400, "ties: three distances")
        q = pr.random_matrix(N, 2, hi=2) << 12
        check(lib, q, groups(N, 2, 3), 400, "ties: two distances, three ones")
        flat = (1 << 14) * (1 - np.eye(N, dtype=np.int64))
        _, want = check(lib, flat, groups(N, 3), 300, "ties: all equal")
        if want["k"] != 300:
            fail("ties: an all-equal matrix must give k = n")
    elif which == "magnitude":
        N = 129
        rng = np.random.default_rng(5)
        q = pr.random_matrix(N, 5, hi=1 << 20)
        y = groups(N, 6, 120)
        on = np.nonzero(y)[0]
        q[np.ix_(on, on)] = pr.IN_MAX - rng.integers(0, 1 << 12, size=(len(on), len(on)))
        q = np.triu(q, 1) + np.triu(q, 1).T
        _, want = check(lib, q, y, 200, "magnitude")
        if not (want["s"] == 6 and want["A"] > 1 << 59 and N * want["A"] > 1 << 63):
            fail("magnitude: the case must need the 128-bit compare")
    elif which == "batches":
        assert batch == 256, "run with PANGENE_PERMA_BATCH=256"
        q, y = pr.planted(140, 3)
        for n in (255, 256, 257, 773):
            check(lib, q, y, n, "batches (batch = %d)" % batch, batch=batch)
    elif which == "large":
        q, y = pr.planted(1001, 1)
        _, want = check(lib, q, y, 300, "large, planted groups")
        if want["k"] != 0:
            fail("large: no permutation may reach the planted split")
        check(lib, q, groups(1001, 2), 300, "large, random groups")
    elif which == "buffers":
        def both(q, L, given=None, **kw):
            want = pr.pan_permanova(q, L, 20, **kw)
            got = capi.pan_permanova(lib, q if given is None else given[0], L if given is None else given[1], **kw)
            ok = pr.same(got, want)
            print("buffers n=%d %s: k = %s: %s" % (q.shape[0], kw, want["k"].tolist(), "ok" if ok else "DIFFERENT"), flush=True)
            if not ok:
                sys.exit(1)

        def labels(n, seed):
            rng = np.random.default_rng(seed)
            L = np.stack([groups(n, seed), groups(n, seed + 1, 1)]).astype(np.int8)
            L[1, rng.random(n) < 0.2] = -1
            return L
        for i, n in enumerate((40, 700, 3, 2, 1, 129, 257, 700, 64, 31)):
            both(pr.random_matrix(n, 10 + i, hi=1 << (8 + 2 * i)), labels(n, 20 + i), n_perm=130, seed=7)
        q, L = pr.random_matrix(500, 3), labels(500, 8)
        both(q, L, given=(torch.from_numpy(q.astype(np.int32)).cuda(), torch.from_numpy(L).cuda()), n_perm=300)
        lib.pg_trim_host_cache(0)  # gives the buffers back; the next call allocates again
        both(pr.random_matrix(300, 99), labels(300, 9), n_perm=100)
        both(pr.random_matrix(300, 98), labels(300, 10), n_perm=0)
    elif which == "range":
        N = pr.LIMIT_N + 1
        y = groups(N, 1)
        t0 = time.perf_counter()
        rc = direct(lib, np.zeros((1, 1), dtype=np.int32), y, 10, rows=False)  # (the refusal comes before the matrix is looked at: one entry does)
        print("range N=%d: status %s after %.3f s" % (N, rc, time.perf_counter() - t0), flush=True)
        if rc != PGA_ERR_RANGE:
            sys.exit(1)
        check(lib, pr.random_matrix(300, 1), groups(300, 2), 20, "after the refusal")
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
