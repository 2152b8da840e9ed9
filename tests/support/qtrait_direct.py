"""TEST INFRASTRUCTURE: direct pga_pan_qtrait / pg_pan_qtrait cases for tests/test_qtrait_gpu.py, run in a child process of their own so
that the test can bound them with a timeout.  The product library (HIP kernels, the int8 MFMA count kernel among them) runs matrices no
GFA fixture reaches, and the numpy restatement (tests/support/qtrait_ref.py) checks a, D and k of every gene completely, never a
sample; where a case says so also the permuted rows and the D_p of the first batch, which come through the tests-only perm_rows and
d_rows pointers of pga_qtrait_in_t.  Prints one line per case and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/qtrait_direct.py {identity|tiles|digits|rows|batches|large|buffers|range|limit}"""
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
import qtrait_ref as qr  # noqa: E402
import trait_ref as tr  # noqa: E402

PGA_ERR_RANGE = -2


class pga_qtrait_in_t(C.Structure):
    _fields_ = [("bits", C.c_void_p), ("c2", C.c_void_p), ("n_gene", C.c_int32), ("n_col", C.c_int32), ("min_count", C.c_int32), ("n_perm", C.c_int32),
                ("seed", C.c_uint32), ("perm_rows", C.c_void_p), ("d_rows", C.c_void_p)]


class pga_qtrait_out_t(C.Structure):
    _fields_ = [("a", C.POINTER(C.c_int32)), ("d", C.POINTER(C.c_int32)), ("k", C.POINTER(C.c_int32))]


def fail(msg):
    print(msg, flush=True)
    sys.exit(1)


def direct(lib, B, c2, n, seed=11, min_count=1, rows=False, d_rows=False, batch=None):
    """pga_pan_qtrait on B (G, N) bool and c2 (N,): dict a, D, k (int32 (G,)) and, when asked, rows (nb, N) int16 and d_rows (nb, G) int32
    of the first batch; or the status when it is not 0"""
    B = np.asarray(B) != 0
    G, N = B.shape
    bits = np.ascontiguousarray(tr.pack(B)) if G and N else np.zeros((max(G, 1), max((N + 31) // 32, 1)), dtype=np.uint32)
    c = np.ascontiguousarray(np.asarray(c2), dtype=np.int16)
    if c.size == 0:
        c = np.zeros(1, dtype=np.int16)
    nb = min(n, batch if batch is not None else n)
    pr = np.full((max(nb, 1), max(N, 1)), -32768, dtype=np.int16)
    dr = np.full((max(nb, 1), max(G, 1)), -(2 ** 31), dtype=np.int32)
    a = pga_qtrait_in_t(bits.ctypes.data, c.ctypes.data, G, N, min_count, n, seed, pr.ctypes.data if rows else None, dr.ctypes.data if d_rows else None)
    out = pga_qtrait_out_t()
    lib.pga_pan_qtrait.restype = C.c_int
    rc = lib.pga_pan_qtrait(C.byref(a), C.byref(out))
    if rc != 0:
        return rc
    res = {key: np.ctypeslib.as_array(getattr(out, f), shape=(G,)).copy() if G else np.zeros(0, dtype=np.int32) for key, f in (("a", "a"), ("D", "d"), ("k", "k"))}
    if rows:
        res["rows"] = pr[:nb, :N]
    if d_rows:
        res["d_rows"] = dr[:nb, :G]
    return res


def check(lib, B, c2, n, label, seed=11, min_count=1, rows=False, d_rows=False, batch=None):
    t0 = time.perf_counter()
    nb = min(n, batch if batch is not None else n)
    a, D, k, el, first = qr.counts(B, c2, n, seed, min_count, d_rows=max(nb, 1))
    t_ref = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = direct(lib, B, c2, n, seed, min_count, rows, d_rows, batch)
    t_lib = time.perf_counter() - t0
    if not isinstance(got, dict):
        fail("%s: status %d" % (label, got))
    bad = [key for key, w in (("a", a), ("D", D), ("k", k)) if not np.array_equal(got[key], w)]
    if rows and not np.array_equal(got["rows"], qr.perm_rows(c2, nb, seed)):
        bad.append("rows")
    if d_rows and not np.array_equal(got["d_rows"], first[:nb]):
        bad.append("d_rows")
    print("%s G=%d N=%d n=%d c=%d: sum k = %d, restatement %.2f s, library %.3f s: %s" % (
        label, B.shape[0], B.shape[1], n, min_count, int(k.sum()), t_ref, t_lib, "DIFFERENT in " + ", ".join(bad) if bad else "ok"), flush=True)
    if bad:
        key = bad[0]
        w = {"a": a, "D": D, "k": k, "rows": qr.perm_rows(c2, nb, seed) if rows else None, "d_rows": first[:nb]}[key]
        at = np.argwhere(got[key] != w)
        fail("  %s: %d differ, first at %s: got %d, want %d" % (key, len(at), at[0].tolist(), got[key][tuple(at[0])], w[tuple(at[0])]))
    return got


def values(N, seed, ties=False):
    """c2 of N random values (distinct, or rounded so that they tie) that are not all equal"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=N)
    if ties:
        v = np.round(v * 2.0)
    v[0], v[-1] = -9.0, 9.0
    return qr.ranks(v)[0]


def matrix(G, N, seed):
    """random rows of every density, the first one full and the last one empty"""
    rng = np.random.default_rng(seed)
    B = rng.random((G, N)) < rng.random((G, 1))
    B[0] = True
    if G > 1:
        B[-1] = False
    return B


def main():
    which = sys.argv[1]
    from pangene_amd import capi
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    lib = capi.load()
    lib.pga_qtrait_batch.restype = C.c_int32
    batch = int(lib.pga_qtrait_batch())  # read from the library, PANGENE_QTRAIT_BATCH included
    if which == "identity":
        # the lane maps of the MFMA: gene g is column g alone, so D_p[g] is value g of permuted row p -- asymmetric data, every (gene, permutation)
        N = 200
        c2 = values(N, 1)
        assert len(set(c2.tolist())) == N
        got = check(lib, np.eye(N, dtype=bool), c2, 130, "identity", rows=True, d_rows=True)
        if not np.array_equal(got["d_rows"], got["rows"].astype(np.int32)):
            fail("identity: d_rows differs from perm_rows")
    elif which == "tiles":
        for N in (2, 3, 63, 64, 65, 255, 256, 257, 1000):
            c2 = values(N, N, ties=N % 2 == 1)
            for G in (1, 127, 128, 129, 300):
                B = matrix(G, N, G * 1000 + N)
                for n in (1, 127, 129):
                    check(lib, B, c2, n, "tiles", seed=5, min_count=2 if n == 127 else 1, d_rows=N in (65, 257, 1000))
    elif which == "digits":
        c2 = values(1000, 2)
        assert int(np.abs(c2).max()) == 999
        check(lib, matrix(300, 1000, 3), c2, 200, "digits: both bytes live", d_rows=True, rows=True)
        v = np.repeat([1.0, 2.0, 3.0], [300, 300, 400])
        np.random.default_rng(4).shuffle(v)
        check(lib, matrix(300, 1000, 5), qr.ranks(v)[0], 200, "digits: three tie groups", d_rows=True)
        check(lib, matrix(300, 100, 6), values(100, 7), 200, "digits: hi = 0", d_rows=True, rows=True)
        ones = np.ones((130, 1000), dtype=bool)
        got = check(lib, ones, c2, 150, "digits: rows of all ones", d_rows=True)
        if got["d_rows"].any() or got["D"].any():
            fail("digits: a full row must sum to 0 under every permutation")
        got = check(lib, np.zeros((130, 257), dtype=bool), values(257, 8), 150, "digits: empty rows", d_rows=True)
        if got["d_rows"].any() or got["k"].any():
            fail("digits: an empty row must sum to 0 and is not eligible")
    elif which == "rows":
        # the permuted rows themselves: the LDS form (N <= 256), the global form, and the device's 64-bit %
        for N in (31, 64, 256, 257, 4200):
            c2 = values(N, N)
            for seed in (11, 0xFFFFFFFF):
                got = direct(lib, np.zeros((0, N), dtype=bool), c2, 64, seed, rows=True)
                ok = isinstance(got, dict) and np.array_equal(got["rows"], qr.perm_rows(c2, 64, seed))
                print("rows N=%d seed=%d: %s" % (N, seed, "ok" if ok else "DIFFERENT"), flush=True)
                if not ok:
                    sys.exit(1)
    elif which == "batches":
        assert batch == 256, "run with PANGENE_QTRAIT_BATCH=256"
        B, c2 = matrix(300, 140, 3), values(140, 4, ties=True)
        for n in (255, 256, 257, 773):
            check(lib, B, c2, n, "batches (batch = %d)" % batch, min_count=2, rows=True, d_rows=True, batch=batch)
    elif which == "large":
        P = ar.planted(20003, 1001, 1, n_module=40)
        cnt = P.sum(axis=1)
        g = int(np.argmin(np.abs(cnt - 500)))
        v = 2.0 * P[g] + np.random.default_rng(2).normal(0.0, 0.3, size=1001)
        got = check(lib, P, qr.ranks(v)[0], 2000, "large")
        if got["k"][g] != 0 or int(got["k"].sum()) == 0:
            fail("large: the planted gene must have k = 0")
    elif which == "buffers":
        def both(P, V, given=None, **kw):
            want = qr.pan_qtrait(P, V, **kw)
            got = capi.pan_qtrait(lib, P if given is None else given[0], V if given is None else given[1], **kw)
            ok = all(np.array_equal(got[key], want[key]) for key in want)
            print("buffers G=%d A=%d %s: sum k = %d: %s" % (P.shape[0], P.shape[1], kw, int(want["k"].sum()), "ok" if ok else "DIFFERENT"), flush=True)
            if not ok:
                sys.exit(1)

        def vals(A, seed):
            rng = np.random.default_rng(seed)
            V = np.stack([rng.normal(size=A), np.round(rng.normal(size=A))])
            V[1, rng.random(A) < 0.2] = np.nan
            return V
        for i, (G, A) in enumerate([(40, 50), (3000, 700), (10, 2), (0, 9), (7, 0), (1, 1), (2, 4), (129, 33), (257, 300), (3000, 700), (1, 64), (50000, 9), (1000, 31)]):
            both(ar.planted(G, A, 10 + i), vals(A, 20 + i), n_perm=130, seed=7)
        Q, VQ = ar.planted(3000, 500, 3), vals(500, 8)
        both(Q, VQ, given=(torch.from_numpy(Q).cuda(), torch.from_numpy(VQ).cuda()), n_perm=300)
        lib.pg_trim_host_cache(0)  # gives the buffers back; the next call allocates again
        both(ar.planted(500, 300, 99), vals(300, 9), n_perm=100, min_count=3)
    elif which == "limit":
        # N at its limit: every digit the planes can hold, int32 accumulators over 32 000 columns, the largest |D| (qtrait_ref.limit_inputs)
        for label, B, c2 in qr.limit_inputs():
            got = check(lib, B, c2, qr.LIMIT_PERM, label, rows=True, d_rows=True)
            if len(c2) == qr.LIMIT_N and (int(got["D"][0]), int(got["D"][1])) != (qr.LIMIT_N ** 2 // 4, -(qr.LIMIT_N ** 2 // 4)):
                fail("limit: the rows of the largest and the smallest values must reach +-N^2 / 4")
    elif which == "range":
        N = 32001
        c2 = (2 * np.arange(N) - (N - 1)).clip(-32000, 32000)
        t0 = time.perf_counter()
        rc = direct(lib, np.ones((3, N), dtype=bool), c2, 10)
        print("range N=%d: status %s after %.3f s" % (N, rc, time.perf_counter() - t0), flush=True)
        if rc != PGA_ERR_RANGE:
            sys.exit(1)
        with np.errstate(all="ignore"):
            try:
                capi.pan_qtrait(lib, np.ones((3, N), dtype=bool), np.arange(N, dtype=np.float64), n_perm=10)
                fail("range: pg_pan_qtrait accepted N = 32 001")
            except RuntimeError as e:
                assert "status %d" % PGA_ERR_RANGE in str(e), e
        check(lib, matrix(5, 300, 1), values(300, 2), 20, "after the refusal")
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
