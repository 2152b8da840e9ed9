"""TEST INFRASTRUCTURE: direct pga_pan_phylosig / pg_pan_phylosig cases for tests/test_phylosig_gpu.py, run in a child process of their own
so that the test can bound them with a timeout.  The product library (the HIP kernels of k_phylosig.hpp) runs trees and sizes no GFA
fixture reaches; the restatement (tests/support/phylosig_ref.py) checks every word of the first batch's orders and costs, and n_le, n_ge
and sum.  file:NAME and memory:NAME put a fixture through pg_phylosig_file and pg_write_phylosig of the product and of the checker build
for every option set, in this one process, so that the device comes up once.  Prints one line per case and "ALL OK" at the end; exits 1
at the first difference.

    python tests/support/phylosig_direct.py {shapes|trees|deep|costs|counts|batches|buffers|refused|range|file:NAME|memory:NAME}"""
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
import phylosig_ref as ps  # noqa: E402
from pairs_direct import random_records  # noqa: E402

COSTS = ((1, 1), (2, 1), (1, 2), (5, 3), (255, 255))
N_CLS = (1, 2, 3, 4, 5, 9)  # 1, CLS, CLS + 1 and 2 CLS + 1 for each of the CLS = 1, 2, 4 classes a lane of k_ps_cost may carry
POISON16, POISON32 = 0xA5A5, 0x5A5A5A5A


class pga_phylosig_in_t(C.Structure):
    _fields_ = [("op", C.c_void_p), ("leaf", C.c_void_p), ("n_leaf", C.c_int32), ("gain", C.c_int32), ("loss", C.c_int32), ("n_cls", C.c_int32), ("cls", C.c_void_p),
                ("n_item", C.c_int32), ("item_cls", C.c_void_p), ("item_cost", C.c_void_p), ("n_perm", C.c_int32), ("seed", C.c_uint32), ("cost_rows", C.c_void_p),
                ("rank_rows", C.c_void_p)]


class pga_phylosig_out_t(C.Structure):
    _fields_ = [("n_le", C.c_void_p), ("n_ge", C.c_void_p), ("sum", C.c_void_p)]


def batch(lib, n_cls):
    lib.pga_phylosig_batch.restype, lib.pga_phylosig_batch.argtypes = C.c_int32, [C.c_int32]
    return lib.pga_phylosig_batch(n_cls)


def raw(lib, op, leaf, L, g, l, cls, item_cls, item_cost, n_perm, seed, cost_rows=None, rank_rows=None, n_cls=None, n_item=None):
    """(status, n_le, n_ge, sum) of pga_pan_phylosig itself"""
    fn = lib.pga_pan_phylosig
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(pga_phylosig_in_t), C.POINTER(pga_phylosig_out_t)]
    op, leaf = np.ascontiguousarray(op, dtype=np.uint8), np.ascontiguousarray(leaf, dtype=np.int32)
    cls, item_cls, item_cost = (np.ascontiguousarray(a, dtype=np.int32) for a in (cls, item_cls, item_cost))
    nc, ni = len(cls) if n_cls is None else n_cls, len(item_cls) if n_item is None else n_item
    cin = pga_phylosig_in_t(op.ctypes.data, leaf.ctypes.data, L, g, l, nc, cls.ctypes.data, ni, item_cls.ctypes.data, item_cost.ctypes.data, n_perm, seed,
                            cost_rows.ctypes.data if cost_rows is not None else None, rank_rows.ctypes.data if rank_rows is not None else None)
    cout = pga_phylosig_out_t()
    rc = fn(C.byref(cin), C.byref(cout))
    if rc != 0:
        return rc, None, None, None
    le = np.ctypeslib.as_array(C.cast(cout.n_le, C.POINTER(C.c_int32)), shape=(ni,)).copy() if ni else np.zeros(0, dtype=np.int32)
    ge = np.ctypeslib.as_array(C.cast(cout.n_ge, C.POINTER(C.c_int32)), shape=(ni,)).copy() if ni else np.zeros(0, dtype=np.int32)
    tot = np.ctypeslib.as_array(C.cast(cout.sum, C.POINTER(C.c_int64)), shape=(nc,)).copy() if nc else np.zeros(0, dtype=np.int64)
    return 0, le, ge, tot


def pick_classes(rng, A, n_cls):
    """n_cls distinct class sizes in 1 .. A - 1, ascending (fewer when the tree has fewer), the smallest and the largest among them"""
    n_cls = min(n_cls, A - 1)
    rest = [n for n in range(2, A - 1)]
    cls = {1, A - 1} if n_cls >= 2 else {int(rng.integers(1, A))}
    while len(cls) < n_cls:
        cls.add(int(rng.choice(rest)))
    return np.array(sorted(cls), dtype=np.int32)


def entry_same(lib, kids, A, cls, n_item, n_perm, seed, g=1, l=1, rng=None, want_need=None, item_cost=None, item_cls=None, mixed=None):
    """pga_pan_phylosig with the program of pairs_ref.program against the restatement: every word of the first batch's orders and costs,
    n_le, n_ge and sum over all batches.  The items' classes and observed costs are drawn around the class's own costs, so that all three
    of <, == and > occur; mixed: a dict that counts them"""
    op, order, need = pr.program(kids, A)
    if want_need is not None and need != want_need:
        return False
    rng = rng or np.random.default_rng(seed)
    B = batch(lib, len(cls))
    nb = min(n_perm, B)
    nbs = (nb + 63) // 64 * 64
    first_rk = ps.orders(A, seed, 1, nbs)  # (the columns past nb too: "a permutation nobody reads" is still the pinned one)
    rows = np.zeros((len(cls), n_perm), dtype=np.int64)
    for p0 in range(0, n_perm, B):
        n = min(B, n_perm - p0)
        rows[:, p0:p0 + n] = ps.replicate_costs(kids, A, cls, n, seed, g, l, first=1 + p0, rk=first_rk if p0 == 0 else None)
    if item_cls is None:
        item_cls = rng.integers(0, len(cls), size=n_item)
        item_cost = rows[item_cls, rng.integers(0, n_perm, size=n_item)] + rng.integers(-1, 2, size=n_item) * (rng.random(n_item) < 0.3)
    cost_rows = np.full((len(cls), nb), POISON32, dtype=np.int32)
    rank_rows = np.full((A, nbs), POISON16, dtype=np.uint16)
    rc, le, ge, tot = raw(lib, op, order, A, g, l, cls, item_cls, item_cost, n_perm, seed, cost_rows, rank_rows)
    if rc != 0:
        return False
    want_le, want_ge = ps.counts(rows, item_cls, item_cost)
    if mixed is not None:
        obs = np.asarray(item_cost, dtype=np.int64)[:, None]
        for k, v in (("lt", rows[item_cls] < obs), ("eq", rows[item_cls] == obs), ("gt", rows[item_cls] > obs)):
            mixed[k] = mixed.get(k, 0) + int(v.sum())
    return (np.array_equal(rank_rows, first_rk.astype(np.uint16)) and np.array_equal(cost_rows, rows[:, :nb]) and np.array_equal(le, want_le) and np.array_equal(ge, want_ge)
            and np.array_equal(tot, rows.sum(axis=1)))


def report(label, what, ok):
    print("%s %s: %s" % (label, what, "ok" if ok else "DIFFERENT"), flush=True)
    if not ok:
        sys.exit(1)


def file_table(lib, gfa, tmp, **kw):
    """what pg_phylosig_file of this library prints for a GFA file"""
    from pangene_amd import capi
    lib.pg_set_output(tmp.encode())
    try:
        rc = lib.pg_phylosig_file(gfa.encode(), C.byref(capi.phylosig_opt(lib, **ps.capi_options(**kw))))
    finally:
        lib.pg_set_output(None)
    with open(tmp, "rb") as f:
        text = f.read()
    os.unlink(tmp)  # (pg_set_output appends)
    return rc, text


def main():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    from pangene_amd import capi
    hip = capi.load()
    which = sys.argv[1]
    rng = np.random.default_rng(5)
    good_op, good_leaf = [0, 0, 1, 0, 1, 0, 1], [2, 0, 3, 1]
    if which == "shapes":  # permutations around the wave and the workgroup of 128 lanes, the class remainder, leaves around the 32-op word and the LDS / scratch switch of the orders
        NB = (1, 63, 64, 65, 127, 128, 129, 257)
        for k, A in enumerate((2, 3, 31, 32, 33, 65, 256, 257)):
            kids = pr.tree(random_records(rng, A), A, "upgma")
            ok = []
            for j, nb in enumerate(NB):
                n_cls = N_CLS[(k + j) % len(N_CLS)] if A > 3 else A - 1
                n_item = (1, 64, 65, 1000)[(k + j) % 4]
                g, l = COSTS[(k + j) % len(COSTS)]
                ok.append(entry_same(hip, kids, A, pick_classes(rng, A, n_cls), n_item, nb, 11 + k + j, g, l, rng))
            report("shapes", "n_leaf=%d, 8 permutation counts" % A, all(ok))
        kids = pr.tree(random_records(rng, 40), 40, "upgma")  # every class remainder at one size
        for n_cls in N_CLS:
            report("shapes", "n_cls=%d" % n_cls, entry_same(hip, kids, 40, pick_classes(rng, 40, n_cls), 65, 129, 3, 2, 1, rng))
        rc, le, ge, tot = raw(hip, good_op, good_leaf, 4, 1, 1, [], [], [], 10, 1)
        report("shapes", "no class, no item", rc == 0 and le.shape == (0,) and tot.shape == (0,))
        rc, le, ge, tot = raw(hip, good_op, good_leaf, 4, 1, 1, [1, 2], [0, 1], [1, 1], 0, 1)
        report("shapes", "no permutation", rc == 0 and not le.any() and not ge.any() and not tot.any())
        rc, le, ge, tot = raw(hip, good_op, good_leaf, 4, 1, 1, [1, 2], [], [], 10, 1)
        report("shapes", "no item", rc == 0 and not tot.any())
        for method in ("nj", "upgma"):  # real trees through the C API, against the checker build too
            import oracle_host
            ora = oracle_host.load()
            P = rng.random((90, 21)) < rng.random(90)[:, None]
            rec, _ = capi.pan_tree(hip, P, "jaccard", method)
            got = capi.pan_phylosig(hip, torch.from_numpy(P).cuda() if method == "nj" else P, rec, method, 2, 1, 200, 7, 2)
            report("shapes", "pg_pan_tree's records " + method, ps.same(got, ps.pan_phylosig(P, pr.tree(rec, 21, method), 2, 1, 200, 7, 2)) and
                   ps.same(got, {k: np.asarray(v, dtype=np.int64) for k, v in capi.pan_phylosig(ora, P, rec, method, 2, 1, 200, 7, 2).items()}))
    elif which == "trees":  # a caterpillar (stack 2) and balanced trees of 2^k leaves (stack k + 1)
        A = 300
        kids = pr.tree(pr.caterpillar_records(A), A, "upgma")
        report("trees", "caterpillar of 300, need 2", entry_same(hip, kids, A, pick_classes(rng, A, 9), 130, 130, 4, 2, 1, rng, want_need=2))
        for k in range(1, 11):
            A = 1 << k
            kids = pr.tree(pr.balanced_records(A), A, "upgma")
            g, l = COSTS[k % len(COSTS)]
            report("trees", "balanced 2^%d, need %d" % (k, k + 1), entry_same(hip, kids, A, pick_classes(rng, A, 5), 70, 70, 20 + k, g, l, rng, want_need=k + 1))
    elif which == "deep":  # the depth limit with the full LDS footprint: a balanced tree of 32 768 leaves, 128 permutations x 8 classes
        A = 32768
        kids = pr.tree(pr.balanced_records(A), A, "upgma")
        cls = np.array([1, 2, 100, 5000, 16384, 20000, 32766, 32767], dtype=np.int32)
        report("deep", "balanced 2^15, 128 permutations x 8 classes, need 16", entry_same(hip, kids, A, cls, 65, 128, 2, 1, 1, rng, want_need=16))
    elif which == "costs":  # the five cost pairs on 65 leaves
        A = 65
        kids = pr.tree(random_records(rng, A), A, "upgma")
        for g, l in COSTS:
            report("costs", "g=%d l=%d" % (g, l), entry_same(hip, kids, A, pick_classes(rng, A, 9), 100, 150, 6, g, l, rng))
    elif which == "counts":  # 257 real items over 65 leaves, P = 200: <, == and > must all occur in the restatement before the device is asked
        A, M, n_perm, seed = 65, 257, 200, 13
        rec = random_records(rng, A)
        kids = pr.tree(rec, A, "upgma")
        P = rng.random((M, A)) < np.where(np.arange(M) % 3 == 0, 0.5, rng.random(M))[:, None]
        P[:8] = False
        for k in range(8):  # some items that follow the tree: the leaves under one join each
            members = [[x] for x in range(A)]
            for a, b in kids:
                members.append(members[a] + members[b])
            big = [m for m in members[A:] if 2 <= len(m) <= A - 2]
            P[k, big[(7 * k) % len(big)]] = True
        want = ps.pan_phylosig(P, kids, 1, 1, n_perm, seed, 2)
        tested = np.nonzero(want["tested"])[0]
        item_cls = np.searchsorted(want["cls"], want["present"][tested])
        rows, obs = want["cost_rows"][item_cls], want["cost"][tested][:, None]
        report("counts", "the restatement meets cost < obs, == obs and > obs (%d, %d, %d)" % ((rows < obs).sum(), (rows == obs).sum(), (rows > obs).sum()),
               (rows < obs).any() and (rows == obs).any() and (rows > obs).any())
        report("counts", "257 items, %d tested, %d classes" % (len(tested), len(want["cls"])),
               entry_same(hip, kids, A, want["cls"], len(tested), n_perm, seed, 1, 1, rng, item_cost=want["cost"][tested], item_cls=item_cls))
        report("counts", "pg_pan_phylosig", ps.same(capi.pan_phylosig(hip, P, rec, "upgma", 1, 1, n_perm, seed, 2), want))
    elif which == "batches":  # PANGENE_PHYLOSIG_BATCH=64 in this process: the counts and the sums add across batches
        A = 40
        report("batches", "the batch is 64", batch(hip, 7) == 64)
        kids = pr.tree(random_records(rng, A), A, "upgma")
        for n_perm in (63, 64, 65, 200):
            mixed = {}
            ok = entry_same(hip, kids, A, pick_classes(rng, A, 7), 300, n_perm, 17, 2, 1, rng, mixed=mixed)
            report("batches", "%d permutations %s" % (n_perm, mixed), ok and all(mixed[k] > 0 for k in ("lt", "eq", "gt")))
    elif which == "buffers":  # the cached buffers: growing, shrinking, given back, and again
        def one(A, n_cls, n_item, n_perm):
            kids = pr.tree(random_records(rng, A), A, "upgma")
            return entry_same(hip, kids, A, pick_classes(rng, A, n_cls), n_item, n_perm, A, 1, 2, rng)
        for A, n_cls, n_item, n_perm in ((10, 3, 40, 30), (300, 20, 700, 200), (3, 2, 5, 1), (120, 9, 2000, 500), (64, 4, 100, 64)):
            report("buffers", "A=%d classes=%d items=%d perms=%d" % (A, n_cls, n_item, n_perm), one(A, n_cls, n_item, n_perm))
        hip.pg_trim_host_cache(0)
        report("buffers", "after trim", one(150, 9, 500, 100))
        hip.pg_trim_host_cache(0)
        report("buffers", "and again", one(150, 9, 500, 100))
    elif which == "refused":  # inputs the entry must turn away before anything is launched
        def rc_of(op=good_op, leaf=good_leaf, L=4, cls=(1, 2), item_cls=(0, 1), **kw):
            return raw(hip, op, leaf, L, 1, 1, list(cls), list(item_cls), [1] * len(item_cls), 10, 1, **kw)[0]
        for name, kw, want in (("a good one", {}, 0), ("a join of one entry", {"op": [0, 1, 0, 0, 1, 0, 1]}, -3), ("two entries left", {"op": [0, 0, 0, 1, 0, 0, 1]}, -3),
                               ("an op of 2", {"op": [0, 0, 2, 0, 1, 0, 1]}, -3), ("a leaf twice", {"leaf": [2, 0, 2, 1]}, -3), ("a leaf of 4", {"leaf": [2, 0, 4, 1]}, -3),
                               ("a leaf of -1", {"leaf": [2, 0, -1, 1]}, -3), ("classes not ascending", {"cls": (2, 1)}, -3), ("a class twice", {"cls": (2, 2)}, -3),
                               ("a class of 0", {"cls": (0, 2)}, -3), ("a class of n_leaf", {"cls": (1, 4)}, -3), ("an item's class of 2", {"item_cls": (0, 2)}, -3),
                               ("an item's class of -1", {"item_cls": (-1, 1)}, -3), ("n_cls = -1", {"n_cls": -1}, -3), ("n_item = -1", {"n_item": -1}, -3)):
            report("refused", name, rc_of(**kw) == want)
        A = 17  # seventeen pushes, then the joins: a stack of 17
        report("refused", "a stack of 17", rc_of(op=[0] * A + [1] * (A - 1), leaf=list(range(A)), L=A) == -2)
        op = [0] * 16 + [1] * 15 + [0, 1]
        rc, le, ge, tot = raw(hip, op, list(range(A)), A, 1, 1, [1], [0], [1], 10, 1)
        report("refused", "a stack of 16 is taken", rc == 0 and le[0] == 10 and ge[0] == 10 and tot[0] == 10)
    elif which == "range":  # sizes and costs the entry turns away before anything is launched
        A = 65536
        rc = raw(hip, np.zeros(2 * A - 1, dtype=np.uint8), np.arange(A), A, 1, 1, [1], [0], [1], 10, 1)[0]
        report("range", "65 536 leaves", rc == -2)
        for g, l in ((0, 1), (256, 1), (1, 0), (1, 256)):
            report("range", "g=%d l=%d" % (g, l), raw(hip, good_op, good_leaf, 4, g, l, [1], [0], [1], 10, 1)[0] == -2)
        report("range", "16 777 216 items", raw(hip, good_op, good_leaf, 4, 1, 1, [1], [0], [1], 10, 1, n_item=16777216)[0] == -2)
        report("range", "2^31 - 1 permutations", raw(hip, good_op, good_leaf, 4, 1, 1, [1], [0], [1], 2147483647, 1)[0] == -2)
        report("range", "-1 permutations", raw(hip, good_op, good_leaf, 4, 1, 1, [1], [0], [1], -1, 1)[0] == -3)
        report("range", "g = l = 255 is taken", raw(hip, good_op, good_leaf, 4, 255, 255, [1], [0], [1], 10, 1)[0] == 0)
        report("range", "the batch for 1 class is 4 096, for 2^20 classes 64", batch(hip, 1) == 4096 and batch(hip, 1 << 20) == 64 and batch(hip, 32768) == 2048)
        try:
            capi.pan_phylosig(hip, np.zeros((1, A), dtype=bool), pr.caterpillar_records(A), "upgma")
            report("range", "pg_pan_phylosig, 65 536 assemblies", False)
        except RuntimeError as e:
            report("range", "pg_pan_phylosig, 65 536 assemblies", "status -2" in str(e))
    elif which.startswith("file:") or which.startswith("memory:"):  # a fixture through both builds, every option set
        import tempfile
        import oracle_host
        ora = oracle_host.load()
        C.c_int.in_dll(hip, "pg_verbose").value = 0
        C.c_int.in_dll(ora, "pg_verbose").value = 0
        route, name = which.split(":")
        gold = os.path.join(ROOT, "tests", "golden")
        with tempfile.TemporaryDirectory() as td:
            tmp = os.path.join(td, "out.tsv")
            if route == "file":
                gfa = os.path.join(gold, name + ".gfa.gz")
            else:  # the GFA of the same run, and its PAF files
                files = sorted(os.path.join(gold, name, f) for f in os.listdir(os.path.join(gold, name)) if ".paf" in f)
                gfa = os.path.join(td, "g.gfa")
                with open(gfa, "wb") as f:
                    f.write(capi.run(hip, files, []))
            for kw in ps.OPTION_SETS + ({"max_p": 0.05},):
                rc1, a = file_table(hip, gfa, tmp, **kw)
                rc2, b = file_table(ora, gfa, tmp, **kw)
                ok = rc1 == 0 and rc2 == 0 and a == b and a.count(b"\n") >= 1
                if route == "file":
                    ok = ok and a == ps.table(gfa, **kw)
                else:
                    ok = ok and a == capi.run(hip, files, ps.option_args(**kw)[1])
                report(which, "%s" % (kw or "defaults"), ok)
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
