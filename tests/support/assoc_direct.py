"""TEST INFRASTRUCTURE: direct pg_pan_assoc cases for tests/test_assoc_gpu.py, run in a child process of their own so that the test can
bound them with a timeout.  The product library (HIP kernels) runs matrices no GFA fixture reaches; the checker build (host loops) and
the numpy restatement (exact integers) check every one of them completely: the output is sparse, so the full sorted record arrays
and the phi arrays are compared, never a sample.  Prints one line per case and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/assoc_direct.py {large|wide|sizes|edges|threshold|band337|band801} [--cpu-only]

--cpu-only runs the checker build against the restatement alone (to see that the cases stay affordable without a GPU)."""
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


def check(libs, P, label, given=None, **kw):
    """every library in libs against the restatement; given: the matrix as the libraries get it (a tensor)"""
    from pangene_amd import capi
    t0 = time.perf_counter()
    want, cnt = ar.select(P, kw.get("min_phi", 0.8), kw.get("min_count", 2), kw.get("sign", "both"))
    phi = ar.phi(want, cnt, P.shape[1])
    t_ref = time.perf_counter() - t0
    ok, ts = True, []
    for lib in libs:
        t0 = time.perf_counter()
        pairs, f = capi.pan_assoc(lib, P if given is None else given, **kw)
        ts.append(time.perf_counter() - t0)
        ok = ok and pairs.shape == want.shape and np.array_equal(pairs, want) and np.array_equal(f, phi)
    print("%s G=%d A=%d %s: %d pairs, restatement %.1f s, libraries %s s: %s" % (
        label, P.shape[0], P.shape[1], kw, len(want), t_ref, " ".join("%.2f" % t for t in ts), "ok" if ok else "DIFFERENT"), flush=True)
    if not ok:
        sys.exit(1)
    return len(want)


def check_band(libs, p, a, s, cmp):
    """band_matrix(a, s) at the thresholds p and p + 1 (and for D < 0 with the signs apart) against the records worked out from (a, s).
    pg_pan_assoc is called on the bytes as they are: at 16.7 M columns the copies of capi.pan_assoc cost as much as the call, and the
    phi it returns is computed by the wrapper from the records, not by the library."""
    import ctypes as C
    from pangene_amd import capi
    P = ar.band_matrix(a, s)
    cnt = [int(np.count_nonzero(r)) for r in P]
    if cnt != [a] * 4 or int(np.count_nonzero(P[0] & P[1])) != s or not np.array_equal(P[0], P[3]) or not np.array_equal(P[1], P[2]):
        sys.exit("band_matrix(%d, %d) does not have the counts asked for" % (a, s))
    D = s * ar.MAX_ASM - a * a
    ok, ts = True, []
    for at, sign in [(p, "both"), (p + 1, "both")] + ([(p, "neg"), (p, "pos")] if D < 0 else []):
        want = ar.band_expected(a, s, at, sign)[0]
        assert len(want) == (2 if sign != "neg" else 0) + (4 if (cmp >= 0 and at == p and sign != "pos") else 0)
        for lib in libs:
            t0 = time.perf_counter()
            got = np.full((8, 3), -1, dtype=np.int32)
            n = lib.pg_pan_assoc(P.ctypes.data_as(C.POINTER(C.c_uint8)), 4, P.shape[1], C.byref(capi.assoc_opt(lib, at / 1000.0, 2, sign)),
                                 got.ctypes.data_as(C.POINTER(C.c_int32)), len(got))
            ts.append(time.perf_counter() - t0)
            ok = ok and n == len(want) and np.array_equal(got[:len(want)], want)
    print("band p=%d a=%d s=%d D%s0 %s: libraries %.2f s: %s" % (p, a, s, "<" if D < 0 else ">", ("below", "equal", "above")[cmp + 1], sum(ts), "ok" if ok else "DIFFERENT"),
          flush=True)
    if not ok:
        sys.exit(1)


def main():
    which = sys.argv[1]
    cpu_only = "--cpu-only" in sys.argv[2:]
    from pangene_amd import capi
    import oracle_host
    ora = oracle_host.load()
    if cpu_only:
        hip, libs = None, [ora]
    else:
        import torch
        assert torch.cuda.is_available()
        torch.cuda.init()
        hip = capi.load()
        libs = [hip, ora]
    if which == "large":
        P = ar.planted(20003, 1001, 1, n_module=40)  # a U-shaped spectrum: about half of the rows are eligible; 32 words a row, the last partial
        n = check(libs, P, "large")
        assert n > 40
        check(libs, P, "large", min_phi=0.3, min_count=5, sign="neg")
        if hip is not None:
            # the second run: a capacity below the number of pairs; the result must be what the unforced run gave
            os.environ["PANGENE_ASSOC_CAP"] = str(max(1, n // 3))
            check([hip], P, "large, forced second run")
            os.environ["PANGENE_ASSOC_CAP"] = "1"
            check([hip], P, "large, forced second run from 1", min_phi=0.6)
            del os.environ["PANGENE_ASSOC_CAP"]
            import torch
            Q = ar.planted(3000, 500, 3)
            check([hip], Q, "torch cuda tensor", given=torch.from_numpy(Q).cuda(), min_phi=0.5)
    elif which == "wide":
        P = ar.planted(70001, 40, 2, n_module=30)  # more rows than pan_shared takes (65 535), 2 words a row
        assert check(libs, P, "wide", min_phi=0.9, min_count=3) > 0
        P = ar.planted(1000003, 12, 5, n_module=10)  # a million rows, few of them eligible at this count
        check(libs, P, "million rows", min_phi=0.95, min_count=6)
    elif which == "threshold":
        # the decision at equality: every slot of an off-diagonal and of a diagonal tile exactly on the threshold, one permille below it
        # and one above, on either side of D = 0 and under every sign; then the exact small cases of the checker's test
        for label, P, p, side, cross, same in ar.tie_tiles():
            for at in (p, p + 1, p - 1):
                for sign in ar.SIGNS:
                    n = check(libs, P, label, min_phi=at / 1000.0, min_count=2, sign=sign)
                    assert n == ar.tie_count(p, side, cross, same, at, sign), "the restatement misses the count the matrix was built for"
        for A, a, b, s, p in ar.exact_threshold_cases():
            P = ar.two_rows(A, a, b, s)
            for at, n in ((p, 1), (p + 1, 0), (p - 1, 1)):
                assert check(libs, P, "exact (a=%d b=%d s=%d)" % (a, b, s), min_phi=at / 1000.0, min_count=2) == n
    elif which in ("band337", "band801"):
        # the guard band at the documented limit A = 16 777 215, where the doubles of the pre-test round: every case of the search for one p
        cases = ar.band_cases(int(which[4:]))
        for p, a, s, cmp in cases:
            check_band(libs, p, a, s, cmp)
        print("band: %d cases" % len(cases), flush=True)
    elif which == "edges":
        # the shapes at which the tile body can go wrong: every row count against every row length.  min_count 1 and phi >= 0 select every
        # pair of rows that are not constant: with eligible rows E is the row count itself, and the matrix of every density has constant
        # rows among the others
        for G in ar.EDGE_ROWS:
            for A in ar.EDGE_COLS:
                check(libs, ar.edge_rows(G, A, G + A, eligible=A >= 2), "edges, every row eligible", min_phi=0.0, min_count=1)
                check(libs, ar.edge_rows(G, A, G + A), "edges", min_phi=0.0, min_count=1)
    else:
        # the cached device buffers: growing, shrinking and growing again in one process
        for i, (G, A) in enumerate([(40, 50), (3000, 700), (10, 2), (0, 9), (7, 0), (0, 0), (1, 1), (2, 4), (129, 33), (257, 4097),
                                    (3000, 700), (1, 64), (100000, 9), (1000, 31)]):
            check(libs, ar.planted(G, A, 10 + i), "sizes", min_phi=0.7)
        if hip is not None:
            hip.pg_trim_host_cache(0)  # gives the buffers back; the next call allocates again
        check(libs, ar.planted(500, 300, 99), "after trim", min_phi=0.5, min_count=1)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
