"""TEST INFRASTRUCTURE: direct pg_pan_join / pg_pan_tree cases for tests/test_tree_gpu.py, run in a child process of their own so that
the test can bound them with a timeout.  The product library (HIP kernels of k_join.hpp) joins matrices no GFA fixture reaches; the
numpy restatement (tests/support/tree_ref.py) checks them where that is affordable, the checker build (host loops of tree.cpp) where it
is not.  Prints one line per case and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/tree_direct.py {sizes|large|cached|equal|presence|parts|signed}"""
import ctypes as C
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


PGA_ERR_RANGE = -2


class pga_join_in_t(C.Structure):
    _fields_ = [("q", C.c_void_p), ("n", C.c_int32), ("method", C.c_int32)]


class pga_join_out_t(C.Structure):
    _fields_ = [("rec", C.POINTER(C.c_int64)), ("n_rec", C.c_int32)]


def backend_join(lib, q, method):
    """pga_pan_join itself, without the checks pg_pan_join makes on the host before it: the records, or the status when it is not 0"""
    q = np.ascontiguousarray(q, dtype=np.int32)
    cin, cout = pga_join_in_t(q.ctypes.data, q.shape[0], tr.METHODS.index(method)), pga_join_out_t()
    lib.pga_pan_join.restype, lib.pga_pan_join.argtypes = C.c_int, [C.POINTER(pga_join_in_t), C.POINTER(pga_join_out_t)]
    rc = lib.pga_pan_join(C.byref(cin), C.byref(cout))
    if rc != 0:
        return rc
    return np.ctypeslib.as_array(cout.rec, shape=(cout.n_rec, 6)).copy()


def restated(q, method):
    """the restatement's records, or PGA_ERR_RANGE where it raises RangeError"""
    try:
        return tr.joins(q, method)
    except tr.RangeError:
        return PGA_ERR_RANGE


def agree(got, want):
    if isinstance(want, int) or isinstance(got, int):  # a status on either side: both must be that status
        return isinstance(want, int) and isinstance(got, int) and got == want
    return np.array_equal(got, want)


def library_join(lib, q, method):
    from pangene_amd import capi
    try:
        return capi.pan_join(lib, q, method)
    except RuntimeError as e:
        assert "status %d" % PGA_ERR_RANGE in str(e), e
        return PGA_ERR_RANGE


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
    elif which == "signed":
        # entries of either sign at the full magnitude of the definition: product and checker build against the restatement
        for n in tr.SIGNED_SIZES:
            q = tr.signed_matrix(n, n)
            for method in tr.METHODS:
                want = restated(q, method)
                report("signed", n, method, agree(library_join(hip, q, method), want) and agree(library_join(ora, q, method), want))
        # a neighbour-joining run that peaks three below the range limit and stays inside
        q, peak, leaving = tr.peak_search()
        report("peak %d" % peak, 5, "nj", peak >= (1 << 30) - (1 << 20) and agree(library_join(hip, q, "nj"), tr.joins(q, "nj")))
        report("peak, upgma", 5, "upgma", agree(library_join(hip, q, "upgma"), tr.joins(q, "upgma")))
        if leaving is not None:
            report("leaves the range on the way", 5, "nj", agree(library_join(hip, leaving, "nj"), PGA_ERR_RANGE) and agree(library_join(ora, leaving, "nj"), PGA_ERR_RANGE))
        # the device's own input flag: pga_pan_join is called directly, because pg_pan_join refuses such an entry on the host.  One
        # entry of exactly +-2^29 in one place at a time -- first row, last row, the last column (at n = 257 the second column a lane
        # of the init kernel reads; ld = 8 at n = 5 .. 7, ld = 260 at n = 257) -- is a range error; +-(2^29 - 1) in all those places is not
        for n in (5, 6, 7, 257):
            base = tr.signed_matrix(n, 1000 + n)
            places = ((0, 1), (n - 1, n - 2), (1, n - 1))
            for method in tr.METHODS:
                ok = True
                for sign in (1, -1):
                    for i, j in places:
                        q = base.copy()
                        q[i, j] = sign * (1 << 29)
                        ok = ok and agree(backend_join(hip, q, method), PGA_ERR_RANGE)
                    q = base.copy()
                    for i, j in places:
                        q[i, j] = q[j, i] = sign * tr.IN_MAX
                    ok = ok and agree(backend_join(hip, q, method), restated(q, method))
                report("input flag", n, method, ok)
        q = matrix(300, 40, 3)
        report("after the refusals", 40, "nj", agree(backend_join(hip, q, "nj"), tr.joins(q, "nj")))
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
