"""TEST INFRASTRUCTURE: direct pga_pan_pairs / pg_pan_pairs cases for tests/test_pairs_gpu.py, run in a child process of their own so that
the test can bound them with a timeout.  The product library (the HIP kernel of k_pairs.hpp) runs trees no GFA fixture reaches; the
restatement (tests/support/pairs_ref.py) checks them where that is affordable, the checker build (host loops of trait.cpp) where it is
not.  Prints one line per case and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/pairs_direct.py {sizes|rows|shapes|deep|buffers|heavier|refused}"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pairs_ref as pr  # noqa: E402

BLOCK = 128  # lanes of a workgroup of k_pairs
KEYS = ("pairs", "supp", "opp")


class pga_pairs_in_t(C.Structure):
    _fields_ = [("op", C.c_void_p), ("bits", C.c_void_p), ("label", C.c_void_p), ("n_gene", C.c_int32), ("n_leaf", C.c_int32), ("n_row", C.c_int32)]


class pga_pairs_out_t(C.Structure):
    _fields_ = [("out", C.c_void_p)]


def bit_rows(P):
    """(G, A) bool -> uint32 (A, W), bit (g & 31) of word g >> 5 of row a = gene g is in assembly a"""
    G, A = P.shape
    W = (G + 31) // 32
    pad = np.zeros((W * 32, A), dtype=np.uint8)
    pad[:G] = P
    return np.ascontiguousarray(np.packbits(np.ascontiguousarray(pad.T).reshape(A, W, 32), axis=2, bitorder="little")).view(np.uint32).reshape(A, W)


def raw(lib, op, bits, label, G, A, R):
    fn = lib.pga_pan_pairs
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(pga_pairs_in_t), C.POINTER(pga_pairs_out_t)]
    cin = pga_pairs_in_t(op.ctypes.data, bits.ctypes.data, label.ctypes.data, G, A, R)
    cout = pga_pairs_out_t()
    rc = fn(C.byref(cin), C.byref(cout))
    if rc != 0 or R * G == 0:
        return rc, None
    return 0, np.ctypeslib.as_array(C.cast(cout.out, C.POINTER(C.c_int32)), shape=(R, G, 3)).copy()


def entry(lib, P, L, kids):
    """pga_pan_pairs itself, with the program of pairs_ref: (status, dict as capi.pan_pairs returns it, stack need)"""
    G, A = P.shape
    op, order, need = pr.program(kids, A)
    bits = np.ascontiguousarray(bit_rows(P)[order]) if A else np.zeros((0, 1), dtype=np.uint32)
    label = np.ascontiguousarray(np.asarray(L, dtype=np.int8).reshape(-1, A)[:, order])
    rc, out = raw(lib, op, bits, label, G, A, label.shape[0])
    return rc, None if out is None else {k: np.ascontiguousarray(out[:, :, i]) for i, k in enumerate(KEYS)}, need


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS)


def random_records(rng, A):
    live, rec = list(range(A)), []
    while len(live) > 1:
        i, j = (int(v) for v in rng.choice(live, size=2, replace=False))
        rec.append((i, j, 0, 0, 0, len(live)))
        live.remove(j)
    return np.array(rec, dtype=np.int64).reshape(-1, 6)


def labels(rng, T, A):
    L = rng.integers(0, 2, size=(T, A)).astype(np.int8)
    L[rng.random((T, A)) < 0.2] = -1
    return L


def alternating(A, G):
    """G genes over A leaves whose types alternate along the leaves: the label row is 1, 0, 1, 0, ...; gene g is the labels (types 3, 0:
    every sibling pair supports), their complement (2, 1: opposes), and six mixtures of the two in blocks of 2^(g % 8) leaves"""
    y = (np.arange(A) % 2 == 0)
    P = np.empty((G, A), dtype=bool)
    for g in range(G):
        k = g % 8
        P[g] = y if k == 0 else ~y if k == 1 else y ^ ((np.arange(A) >> k) % 2 == 1)
    return P, y.astype(np.int8)[None, :]


def report(label, what, ok):
    print("%s %s: %s" % (label, what, "ok" if ok else "DIFFERENT"), flush=True)
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
    rng = np.random.default_rng(5)
    if which == "sizes":  # gene counts around a word, a wave and a workgroup; entry and C API against the restatement
        A = 37
        rec = random_records(rng, A)
        kids = pr.tree(rec, A, "upgma")
        L = labels(rng, 2, A)
        for G in (1, 31, 32, 33, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 5):
            P = rng.random((G, A)) < 0.5
            want = pr.counts(P, L, rec, "upgma")
            rc, got, _ = entry(hip, P, L, kids)
            report("sizes", "G=%d entry" % G, rc == 0 and same(got, want))
            report("sizes", "G=%d pg_pan_pairs" % G, same(capi.pan_pairs(hip, P, L, rec, "upgma"), want))
        rc, got = raw(hip, *[np.zeros(1, dtype=np.uint8)] * 3, 0, 0, 0)
        report("sizes", "nothing at all", rc == 0)
    elif which == "rows":  # 1, 2 and 5 label rows, among them a row without values and rows of one type
        A, G = 50, 70
        rec = random_records(rng, A)
        kids = pr.tree(rec, A, "upgma")
        P = rng.random((G, A)) < 0.5
        P[3] = True  # with a constant label row: every leaf of one type
        L5 = labels(rng, 5, A)
        L5[1] = -1
        L5[3] = 1
        for T in (1, 2, 5):
            L = L5[:T] if T != 1 else L5[4:5]
            want = pr.counts(P, L, rec, "upgma")
            rc, got, _ = entry(hip, P, L, kids)
            report("rows", "%d rows entry" % T, rc == 0 and same(got, want))
            report("rows", "%d rows pg_pan_pairs" % T, same(capi.pan_pairs(hip, P, L, rec, "upgma"), want))
        report("rows", "no pairs in the empty and the constant row", not want["pairs"][1].any() and not want["pairs"][3].any() and want["pairs"][0].any())
        for method in ("nj", "upgma"):  # and through real trees, torch tensors on the device
            Pl = (rng.random((90, 21)) < 0.5)
            r2, _ = capi.pan_tree(hip, Pl, "jaccard", method)
            Ll = labels(rng, 3, 21)
            got = capi.pan_pairs(hip, torch.from_numpy(Pl).cuda(), torch.from_numpy(Ll).cuda(), r2, method)
            report("rows", "pg_pan_tree's records " + method, same(got, pr.counts(Pl, Ll, r2, method)) and same(got, capi.pan_pairs(ora, Pl, Ll, r2, method)))
    elif which == "shapes":  # a caterpillar (stack 2) and balanced trees of 2^k leaves (stack k + 1)
        A = 200
        rec = pr.caterpillar_records(A)
        P, L = rng.random((65, A)) < 0.5, labels(rng, 2, A)
        rc, got, need = entry(hip, P, L, pr.tree(rec, A, "upgma"))
        report("shapes", "caterpillar of 200, need %d" % need, rc == 0 and need == 2 and same(got, pr.counts(P, L, rec, "upgma")))
        for k in range(1, 9):
            A = 1 << k
            rec = pr.balanced_records(A)
            P, L = rng.random((40, A)) < 0.5, labels(rng, 2, A)
            want = pr.counts(P, L, rec, "upgma")
            rc, got, need = entry(hip, P, L, pr.tree(rec, A, "upgma"))
            report("shapes", "balanced 2^%d, need %d" % (k, need), rc == 0 and need == k + 1 and same(got, want))
            report("shapes", "balanced 2^%d pg_pan_pairs" % k, same(capi.pan_pairs(hip, P, L, rec if A >= 3 else None, "upgma"), want))
    elif which == "deep":  # the depth limit and the packing's extremes: 65 535 leaves, alternating types, pairs = 32 767
        for A, with_ref in ((4095, True), (65535, False)):
            rec = pr.balanced_records(A)
            P, L = alternating(A, 64)
            kids = pr.tree(rec, A, "upgma")
            rc, got, need = entry(hip, P, L, kids)
            report("deep", "A=%d entry, need %d" % (A, need), rc == 0 and need == A.bit_length())
            report("deep", "A=%d pairs %d supp %d opp %d" % (A, got["pairs"][0, 0], got["supp"][0, 0], got["opp"][0, 1]),
                   got["pairs"][0, 0] == A // 2 and got["supp"][0, 0] == A // 2 and got["opp"][0, 0] == 0 and got["opp"][0, 1] == A // 2 and got["supp"][0, 1] == 0)
            report("deep", "A=%d checker build" % A, same(got, capi.pan_pairs(ora, P, L, rec, "upgma")) and same(got, capi.pan_pairs(hip, P, L, rec, "upgma")))
            if with_ref:
                report("deep", "A=%d restatement" % A, same(got, pr.counts(P, L, rec, "upgma")))
    elif which == "buffers":  # the cached buffers: growing, shrinking, given back, and again
        for i, (A, G, T) in enumerate(((10, 40, 1), (300, 700, 3), (3, 5, 1), (120, 2000, 2), (64, 100, 4))):
            rec = random_records(rng, A)
            P, L = rng.random((G, A)) < 0.5, labels(rng, T, A)
            report("buffers", "A=%d G=%d T=%d" % (A, G, T), same(capi.pan_pairs(hip, P, L, rec, "upgma"), capi.pan_pairs(ora, P, L, rec, "upgma")))
        hip.pg_trim_host_cache(0)
        rec = random_records(rng, 150)
        P, L = rng.random((500, 150)) < 0.5, labels(rng, 2, 150)
        want = capi.pan_pairs(ora, P, L, rec, "upgma")
        report("buffers", "after trim", same(capi.pan_pairs(hip, P, L, rec, "upgma"), want))
        hip.pg_trim_host_cache(0)
        report("buffers", "and again", same(capi.pan_pairs(hip, P, L, rec, "upgma"), want))
    elif which == "heavier":  # records whose heavier child sits in slot i in some joins and in slot j in others
        for A in (9, 33, 90):
            for it in range(4):
                rec = random_records(rng, A)
                kids = pr.tree(rec, A, "upgma")
                need = [1] * A
                for a, b in kids:
                    need.append(need[a] + 1 if need[a] == need[b] else max(need[a], need[b]))
                i_heavier = sum(need[a] > need[b] for a, b in kids)
                j_heavier = sum(need[a] < need[b] for a, b in kids)
                P, L = rng.random((66, A)) < 0.5, labels(rng, 2, A)
                want = pr.counts(P, L, rec, "upgma")
                rc, got, _ = entry(hip, P, L, kids)
                report("heavier", "A=%d: slot i heavier in %d joins, slot j in %d" % (A, i_heavier, j_heavier),
                       i_heavier > 0 and j_heavier > 0 and rc == 0 and same(got, want) and same(capi.pan_pairs(hip, P, L, rec, "upgma"), want))
    elif which == "refused":  # programs and sizes the entry must turn away before anything is launched
        P, L = rng.random((10, 4)) < 0.5, labels(rng, 1, 4)
        bits, lab = bit_rows(P), np.ascontiguousarray(L)
        for name, op, want in (("a join of one entry", [0, 1, 0, 0, 1, 0, 1], -3), ("two entries left", [0, 0, 0, 1, 0, 0, 1], -3), ("an op of 2", [0, 0, 2, 0, 1, 0, 1], -3),
                               ("a good one", [0, 0, 1, 0, 1, 0, 1], 0)):
            rc, _ = raw(hip, np.array(op, dtype=np.uint8), bits, lab, 10, 4, 1)
            report("refused", name, rc == want)
        A = 17  # seventeen pushes, then the joins: a stack of 17
        P, L = rng.random((10, A)) < 0.5, labels(rng, 1, A)
        rc, _ = raw(hip, np.array([0] * A + [1] * (A - 1), dtype=np.uint8), bit_rows(P), np.ascontiguousarray(L), 10, A, 1)
        report("refused", "a stack of 17", rc == -2)
        rc, _ = raw(hip, np.array([0] * 16 + [1] * 15 + [0, 1], dtype=np.uint8), bit_rows(P), np.ascontiguousarray(L), 10, A, 1)
        report("refused", "a stack of 16 is taken", rc == 0)
        A = 65536
        rc, _ = raw(hip, np.zeros(2 * A - 1, dtype=np.uint8), np.zeros((A, 1), dtype=np.uint32), np.zeros((1, A), dtype=np.int8), 10, A, 1)
        report("refused", "65 536 leaves", rc == -2)
        wide = np.zeros((1, A), dtype=bool)
        try:
            capi.pan_pairs(hip, wide, np.zeros(A, dtype=np.int8), pr.caterpillar_records(A), "upgma")
            report("refused", "pg_pan_pairs, 65 536 assemblies", False)
        except RuntimeError as e:
            report("refused", "pg_pan_pairs, 65 536 assemblies", "status -2" in str(e))
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
