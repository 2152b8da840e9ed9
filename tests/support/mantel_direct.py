"""TEST INFRASTRUCTURE: direct pga_pan_mantel / pg_pan_mantel cases for tests/test_mantel_gpu.py, run in a child process of their own so that
the test can bound them with a timeout.  The product library (HIP kernels k_mantel_order, k_mantel_z, k_mantel_stat) runs matrices no GFA
fixture reaches, and the numpy / Python-int restatement (tests/support/mantel_ref.py) checks Z, n_ge, n_le and, through the tests-only
z_rows / ord_rows pointers of pga_mantel_in_t, Z_p and the order of EVERY permutation of the first batch, never a sample.  Prints one line
per case and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/mantel_direct.py {maps|tiles|classes|ties|magnitude|batches|limit|buffers|range}"""
import ctypes as C
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import curves_ref as cr  # noqa: E402
import mantel_ref as mr  # noqa: E402

PGA_ERR_RANGE = -2


class pga_mantel_in_t(C.Structure):
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("n", C.c_int32), ("max_a", C.c_int32), ("max_b", C.c_int32), ("n_perm", C.c_int32), ("seed", C.c_uint32),
                ("z_rows", C.c_void_p), ("ord_rows", C.c_void_p)]


class pga_mantel_out_t(C.Structure):
    _fields_ = [("z", C.c_int64), ("n_ge", C.c_int64), ("n_le", C.c_int64)]


def fail(msg):
    print(msg, flush=True)
    sys.exit(1)


def direct(lib, a, b, n, seed=11, batch=None, rows=True, N=None):
    """pga_pan_mantel on a, b (N, N) int32: dict Z, n_ge, n_le and, with rows, z_rows (nb,) and ord_rows (nb, N) of the first batch; or the
    status when it is not 0"""
    a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
    N = a.shape[0] if N is None else N
    nb = max(min(n, batch if batch is not None else n), 1)
    zr = np.full(nb, -7, dtype=np.int64)
    orr = np.full((nb, N), 0xFFFF, dtype=np.uint16)
    arg = pga_mantel_in_t(a.ctypes.data, b.ctypes.data, N, int(a.max()), int(b.max()), n, seed, zr.ctypes.data if rows else None, orr.ctypes.data if rows else None)
    out = pga_mantel_out_t()
    lib.pga_pan_mantel.restype = C.c_int
    rc = lib.pga_pan_mantel(C.byref(arg), C.byref(out))
    if rc != 0:
        return rc
    res = {"Z": out.z, "n_ge": out.n_ge, "n_le": out.n_le}
    if rows:
        nb = min(n, nb)
        res.update(z_rows=zr[:nb], ord_rows=orr[:nb])
    return res


def report(label, N, n, got, want, nb, t_ref, t_lib):
    """want: dict Z, n_ge, n_le, z_rows, ord_rows of the first nb permutations"""
    if not isinstance(got, dict):
        fail("%s: status %d" % (label, got))
    bad = [key for key in ("Z", "n_ge", "n_le") if got[key] != want[key]]
    if nb:
        bad += [key for key in ("ord_rows", "z_rows") if not np.array_equal(got[key].astype(np.int64), want[key][:nb])]
    print("%s N=%d n=%d: Z = %d, n_ge = %d, n_le = %d, restatement %.2f s, library %.3f s: %s" % (
        label, N, n, want["Z"], want["n_ge"], want["n_le"], t_ref, t_lib, "DIFFERENT in " + ", ".join(bad) if bad else "ok"), flush=True)
    if bad:
        key = bad[0]
        if key in ("z_rows", "ord_rows"):
            at = np.argwhere(got[key].astype(np.int64) != want[key][:nb])
            fail("  %s: %d entries differ, first at %s: got %d, want %d" % (key, len(at), at[0].tolist(), got[key][tuple(at[0])], want[key][tuple(at[0])]))
        fail("  %s: got %s, want %s" % (key, got.get(key), want.get(key)))


def check(lib, a, b, n, label, seed=11, batch=None):
    N = a.shape[0]
    nb = min(n, batch if batch is not None else n)
    t0 = time.perf_counter()
    want = mr.direct(a, b, n, seed, rows=max(nb, 1))
    t_ref = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = direct(lib, a, b, n, seed, batch)
    t_lib = time.perf_counter() - t0
    report(label, N, n, got, want, nb, t_ref, t_lib)
    return got, want


def check_quadratic(lib, N, n, label, seed=11):
    """a large N: a_ij = x_i xor x_j below 2^17 (cheap, irregular, symmetric, zero diagonal), b_ij = u_i u_j off the diagonal with u in
    [1, 2^8], so that Z of an order is the quadratic form u_o . a . u_o (a's diagonal is zero): one int64 matrix-vector product per
    permutation, in row chunks.  a b N (N - 1) < 2^17 2^16 2^28 = 2^61."""
    rng = np.random.default_rng(N)
    x = rng.integers(0, 1 << 17, size=N, dtype=np.int32)
    u = rng.integers(1, (1 << 8) + 1, size=N, dtype=np.int64)
    a = np.bitwise_xor(x[:, None], x[None, :])
    b = np.outer(u, u).astype(np.int32)
    np.fill_diagonal(b, 0)
    t0 = time.perf_counter()

    def quad(o):
        v = u[np.asarray(o, dtype=np.int64)]
        return int(sum(int(v[r:r + 2048] @ (a[r:r + 2048].astype(np.int64) @ v)) for r in range(0, N, 2048)))
    O = cr.orders(N, 1, n, seed).astype(np.int64)
    Z = quad(np.arange(N))
    zs = np.array([quad(o) for o in O], dtype=np.int64)
    want = {"Z": Z, "n_ge": int((zs >= Z).sum()), "n_le": int((zs <= Z).sum()), "z_rows": zs, "ord_rows": O}
    t_ref = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = direct(lib, a, b, n, seed)
    t_lib = time.perf_counter() - t0
    report(label, N, n, got, want, n, t_ref, t_lib)


def main():
    which = sys.argv[1]
    from pangene_amd import capi
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    lib = capi.load()
    lib.pga_mantel_batch.restype = C.c_int32
    batch = int(lib.pga_mantel_batch())  # read from the library, PANGENE_MANTEL_BATCH included
    if which == "maps":
        # every entry of a and of b distinct, so a value from a wrong row, column or order shows
        N = 200
        a, b = mr.distinct_matrix(N), mr.distinct_matrix(N, mul=3, add=7)
        iu = np.triu_indices(N, 1)
        assert len(np.unique(a[iu])) == len(np.unique(b[iu])) == N * (N - 1) // 2
        check(lib, a, b, 130, "maps")
    elif which == "tiles":
        for N in (3, 4, 63, 64, 65, 255, 256, 257, 1023, 1025):
            a, b = mr.random_matrix(N, N, hi=1 << 16), mr.random_matrix(N, N + 1, hi=1 << 16)
            for n in (1, 63, 65):
                check(lib, a, b, n, "tiles", seed=5)
    elif which == "classes":
        # the edges of the code's own size classes: a workgroup of k_mantel_z takes 16 rows and row N - 1 is never staged (N - 1 = 15, 16,
        # 17 and 2, 3 workgroups at 32, 33, 34); k_mantel_order keeps its rows in LDS up to N = 256 (in `tiles`); k_mantel_z asks for more
        # than 64 KiB of dynamic LDS, which takes a function attribute, from N = 10 913 on (64 + 6 N bytes)
        for N in (16, 17, 18, 33, 34):
            check(lib, mr.random_matrix(N, N, hi=1 << 16), mr.random_matrix(N, N + 1, hi=1 << 16), 65, "classes", seed=6)
        for N in (10912, 10913):
            check_quadratic(lib, N, 2, "classes")
    elif which == "ties":
        N = 150
        a = mr.random_matrix(N, 1, hi=1 << 12)
        flat = (1 << 14) * (1 - np.eye(N, dtype=np.int64))
        got, _ = check(lib, a, flat, 300, "ties: a constant b")
        if got["n_ge"] != 300 or got["n_le"] != 300:
            fail("ties: a constant b must give n_ge = n_le = n")
        a, b = mr.random_matrix(12, 5, hi=2) << 8, mr.random_matrix(12, 6, hi=2) << 8
        got, _ = check(lib, a, b, 400, "ties: two values")
        if got["n_ge"] + got["n_le"] <= 400:
            fail("ties: the two-valued case must have permutations with Z_p = Z")
    elif which == "magnitude":
        # a = b at the largest entry the bound allows: m^2 N (N - 1) < 2^62.  (Every term is non-negative, so no partial sum passes the
        # total and nothing wraps in 64 bits; the case holds the top of the range: Z is above 2^61.)
        N = 129
        m = math.isqrt(((1 << 62) - 1) // (N * (N - 1)))
        assert m * m * N * (N - 1) < 1 << 62 <= (m + 1) ** 2 * N * (N - 1) and m < 1 << 31
        a = m - mr.random_matrix(N, 5, hi=1 << 12)
        np.fill_diagonal(a, 0)
        a[0, 1] = a[1, 0] = m
        _, want = check(lib, a, a, 200, "magnitude")
        if not want["Z"] > 1 << 61:
            fail("magnitude: Z must be above 2^61")
        # entries of 2^29 - 1 through pg_pan_mantel, so that the shifts are derived and applied on the way to the device
        qx, qy = mr.random_matrix(N, 7, hi=1 << 29), mr.random_matrix(N, 8, hi=1 << 20)
        qx[2, 3] = qx[3, 2] = mr.IN_MAX
        want = mr.pan_mantel(qx, qy, 200, 3)
        got = capi.pan_mantel(lib, qx, qy, n_perm=200, seed=3)
        ok = mr.same(got, want) and want["sx"] == mr.shift_of(mr.IN_MAX, N) > 0 and want["sy"] == 0
        print("magnitude, shifts N=%d: sx = %d, sy = %d, Z = %d: %s" % (N, want["sx"], want["sy"], want["Z"], "ok" if ok else "DIFFERENT: %s" % got), flush=True)
        if not ok:
            sys.exit(1)
    elif which == "batches":
        assert batch == 256, "run with PANGENE_MANTEL_BATCH=256"
        a = mr.random_matrix(140, 3)
        b = mr.noisy_copy(a, 4, 1 << 18)
        for n in (255, 256, 257, 773):
            check(lib, a, b, n, "batches (batch = %d)" % batch, batch=batch)
    elif which == "limit":
        check_quadratic(lib, mr.LIMIT_N, 3, "limit")
    elif which == "buffers":
        def both(qx, qy, given=None, **kw):
            want = mr.pan_mantel(qx, qy, **kw)
            got = capi.pan_mantel(lib, *(given if given is not None else (qx, qy)), **kw)
            ok = mr.same(got, want)
            print("buffers n=%d %s: Z = %d, n_ge = %d: %s" % (qx.shape[0], kw, want["Z"], want["n_ge"], "ok" if ok else "DIFFERENT"), flush=True)
            if not ok:
                sys.exit(1)
        for i, n in enumerate((40, 700, 3, 2, 1, 129, 257, 700, 64, 31)):
            both(mr.random_matrix(n, 10 + i, hi=1 << (8 + 2 * i)), mr.random_matrix(n, 30 + i, hi=1 << (26 - 2 * i)), n_perm=130, seed=7)
        qx, qy = mr.random_matrix(500, 3), mr.random_matrix(500, 4)
        both(qx, qy, given=(torch.from_numpy(qx.astype(np.int32)).cuda(), torch.from_numpy(qy.astype(np.int32)).cuda()), n_perm=300)
        lib.pg_trim_host_cache(0)  # gives the buffers back; the next call allocates again
        both(mr.random_matrix(300, 99), mr.random_matrix(300, 98), n_perm=100)
        both(mr.random_matrix(300, 97), mr.random_matrix(300, 96), n_perm=0)
    elif which == "range":
        N = mr.LIMIT_N + 1
        t0 = time.perf_counter()
        one = np.zeros((1, 1), dtype=np.int32)
        rc = direct(lib, one, one, 10, rows=False, N=N)  # (the refusal comes before the matrices are looked at: one entry does)
        print("range N=%d: status %s after %.3f s" % (N, rc, time.perf_counter() - t0), flush=True)
        if rc != PGA_ERR_RANGE:
            sys.exit(1)
        check(lib, mr.random_matrix(300, 1), mr.random_matrix(300, 2), 20, "after the refusal")
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
