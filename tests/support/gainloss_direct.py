"""TEST INFRASTRUCTURE: direct pga_pan_gainloss / pg_pan_gainloss cases for tests/test_gainloss_gpu.py, run in a child process of their own
so that the test can bound them with a timeout.  The product library (the HIP kernels of k_gainloss.hpp) runs trees and sizes no GFA
fixture reaches; the restatement (tests/support/gainloss_ref.py) checks gene, node and every word of the state rows.  file:NAME and
memory:NAME put a fixture through pg_gainloss_file and pg_write_gainloss of the product and of the checker build for every option set, in
this one process, so that the device comes up once.  Prints one line per case and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/gainloss_direct.py {shapes|trees|deep|refused|ties|chunks|buffers|range|file:NAME|memory:NAME}"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gainloss_ref as gr  # noqa: E402
import pairs_ref as pr  # noqa: E402
from pairs_direct import bit_rows, random_records  # noqa: E402

COSTS = ((1, 1), (2, 1), (1, 2), (5, 3), (255, 255))
MODES = ("late", "early")


class pga_gainloss_in_t(C.Structure):
    _fields_ = [("op", C.c_void_p), ("bits", C.c_void_p), ("par", C.c_void_p), ("n_gene", C.c_int32), ("n_leaf", C.c_int32), ("gain", C.c_int32),
                ("loss", C.c_int32), ("mode", C.c_int32), ("st_rows", C.c_void_p)]


class pga_gainloss_out_t(C.Structure):
    _fields_ = [("gene", C.c_void_p), ("node", C.c_void_p)]


def chunk(lib, n_leaf):
    lib.pga_gainloss_chunk.restype, lib.pga_gainloss_chunk.argtypes = C.c_int32, [C.c_int32]
    return lib.pga_gainloss_chunk(n_leaf)


def raw(lib, op, bits, par, G, L, g=1, l=1, mode=0, st_rows=None):
    """(status, gene (G, 4) int32, node (2 L - 1, 3) int64) of pga_pan_gainloss itself"""
    fn = lib.pga_pan_gainloss
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(pga_gainloss_in_t), C.POINTER(pga_gainloss_out_t)]
    cin = pga_gainloss_in_t(op.ctypes.data, bits.ctypes.data, par.ctypes.data, G, L, g, l, mode, st_rows.ctypes.data if st_rows is not None else None)
    cout = pga_gainloss_out_t()
    rc = fn(C.byref(cin), C.byref(cout))
    if rc != 0:
        return rc, None, None
    n_op = max(2 * L - 1, 0)
    gene = np.ctypeslib.as_array(C.cast(cout.gene, C.POINTER(C.c_int32)), shape=(G, 4)).copy() if G else np.zeros((0, 4), dtype=np.int32)
    node = np.ctypeslib.as_array(C.cast(cout.node, C.POINTER(C.c_int64)), shape=(n_op, 3)).copy() if n_op else np.zeros((0, 3), dtype=np.int64)
    return 0, gene, node


def entry_same(lib, P, kids, g=1, l=1, mode="late", ties=None, want_need=None):
    """pga_pan_gainloss with the program of gainloss_ref against the restatement: gene, node in op order, every word of the state rows of
    the first chunk"""
    M, A = P.shape
    op, order, need, node_of, par = gr.program(kids, A)
    if want_need is not None and need != want_need:
        return False
    bits = np.ascontiguousarray(bit_rows(P)[order])
    first = min(M, chunk(lib, A))
    WW = (first + 63) // 64
    st = np.full((len(op), WW), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc, gene, node = raw(lib, op, bits, par, M, A, g, l, MODES.index(mode), st)
    if rc != 0:
        return False
    want = gr.reconstruct(P, kids, g, l, mode, ties)
    ok = all(np.array_equal(gene[:, i], want[k]) for i, k in enumerate(("cost", "gains", "losses", "root")))
    ok = ok and all(np.array_equal(node[:, i], want[k][node_of]) for i, k in enumerate(("node_present", "node_gains", "node_losses")))
    return ok and np.array_equal(st, gr.state_words(want["state"][node_of][:, :first], WW))


def par_of(op):
    """the op of the parent of the node every op of a well-formed program makes, -1 for the last"""
    par, stack = np.full(len(op), -1, dtype=np.int32), []
    for k, o in enumerate(op):
        if o:
            par[stack.pop()] = k
            par[stack.pop()] = k
        stack.append(k)
    return par


def report(label, what, ok):
    print("%s %s: %s" % (label, what, "ok" if ok else "DIFFERENT"), flush=True)
    if not ok:
        sys.exit(1)


def file_table(lib, gfa, tmp, **kw):
    """what pg_gainloss_file of this library prints for a GFA file"""
    from pangene_amd import capi
    lib.pg_set_output(tmp.encode())
    try:
        rc = lib.pg_gainloss_file(gfa.encode(), C.byref(capi.gainloss_opt(lib, **gr.capi_options(**kw))))
    finally:
        lib.pg_set_output(None)
    with open(tmp, "rb") as f:
        text = f.read()
    os.unlink(tmp)  # (pg_set_output appends)
    return rc, text


def mixed_items(rng, M, A):
    """M items: a third at density 1/2, the others at a density of their own drawn from (0, 1)"""
    dens = np.where(np.arange(M) % 3 == 0, 0.5, rng.random(M))
    return rng.random((M, A)) < dens[:, None]


def main():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.init()
    from pangene_amd import capi
    hip = capi.load()
    which = sys.argv[1]
    rng = np.random.default_rng(5)
    if which == "shapes":  # items around the ballot word and the workgroup of 128 lanes, leaves around the 32-op word and the 32-leaf gather
        for A in (1, 2, 3, 4, 31, 32, 33, 64, 65):
            rec = random_records(rng, A)
            kids = pr.tree(rec, A, "upgma")
            ok = []
            for M in (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4097):
                P = mixed_items(rng, M, A)
                g, l = COSTS[(A + M) % len(COSTS)]
                mode = MODES[M % 2]
                ok.append(entry_same(hip, P, kids, g, l, mode))
                if M in (65, 257):  # and through the C API, torch tensors on the device
                    got = capi.pan_gainloss(hip, torch.from_numpy(P).cuda(), rec if A >= 3 else None, "upgma", g, l, mode)
                    ok.append(gr.same(got, gr.reconstruct(P, kids, g, l, mode)))
            report("shapes", "n_leaf=%d, 11 item counts" % A, all(ok))
        rc, gene, node = raw(hip, *[np.zeros(1, dtype=np.uint8)] * 3, 0, 0)
        report("shapes", "nothing at all", rc == 0 and gene.shape == (0, 4) and node.shape == (0, 3))
        for method in ("nj", "upgma"):  # real trees, against the checker build too
            import oracle_host
            ora = oracle_host.load()
            P = mixed_items(rng, 90, 21)
            rec, _ = capi.pan_tree(hip, P, "jaccard", method)
            got = capi.pan_gainloss(hip, P, rec, method, 2, 1, "early")
            report("shapes", "pg_pan_tree's records " + method, gr.same(got, gr.reconstruct(P, pr.tree(rec, 21, method), 2, 1, "early")) and
                   gr.same(got, {k: np.asarray(v, dtype=np.int64) for k, v in capi.pan_gainloss(ora, P, rec, method, 2, 1, "early").items()}))
    elif which == "trees":  # a caterpillar (stack 2) and balanced trees of 2^k leaves (stack k + 1)
        A = 300
        kids = pr.tree(pr.caterpillar_records(A), A, "upgma")
        report("trees", "caterpillar of 300, need 2", entry_same(hip, mixed_items(rng, 130, A), kids, 2, 1, "late", want_need=2))
        for k in range(1, 11):
            A = 1 << k
            rec = pr.balanced_records(A)
            kids = pr.tree(rec, A, "upgma")
            g, l = COSTS[k % len(COSTS)]
            P = mixed_items(rng, 70, A)
            report("trees", "balanced 2^%d, need %d" % (k, k + 1), entry_same(hip, P, kids, g, l, MODES[k % 2], want_need=k + 1))
            if k in (1, 5, 10):
                report("trees", "balanced 2^%d pg_pan_gainloss" % k, gr.same(capi.pan_gainloss(hip, P, rec if A >= 3 else None, "upgma", g, l, MODES[k % 2]),
                                                                           gr.reconstruct(P, kids, g, l, MODES[k % 2])))
    elif which == "deep":  # the depth limit with the full LDS footprint: a balanced tree of 32 768 leaves, 65 items
        A = 32768
        kids = pr.tree(pr.balanced_records(A), A, "upgma")
        report("deep", "balanced 2^15 x 65 items, need 16", entry_same(hip, mixed_items(rng, 65, A), kids, 1, 1, "late", want_need=16))
    elif which == "refused":  # programs the entry must turn away before anything is launched
        A = 4
        P = mixed_items(rng, 10, A)
        bits = bit_rows(P)
        good_op, good_par = [0, 0, 1, 0, 1, 0, 1], [2, 2, 4, 4, 6, 6, -1]
        for name, op, par, want in (("a good one", good_op, good_par, 0), ("a join of one entry", [0, 1, 0, 0, 1, 0, 1], good_par, -3),
                                    ("two entries left", [0, 0, 0, 1, 0, 0, 1], good_par, -3), ("an op of 2", [0, 0, 2, 0, 1, 0, 1], good_par, -3),
                                    ("a root with a parent", good_op, [2, 2, 4, 4, 6, 6, 0], -3), ("a leaf under the wrong join", good_op, [2, 4, 4, 4, 6, 6, -1], -3),
                                    ("a join under itself", good_op, [2, 2, 2, 4, 6, 6, -1], -3), ("a parent of -1 below the root", good_op, [2, 2, 4, 4, -1, 6, -1], -3),
                                    ("a parent out of range", good_op, [2, 2, 4, 4, 6, 7, -1], -3)):
            rc, _, _ = raw(hip, np.array(op, dtype=np.uint8), bits, np.array(par, dtype=np.int32), 10, A)
            report("refused", name, rc == want)
        rc, _, _ = raw(hip, np.array(good_op, dtype=np.uint8), bits, np.array(good_par, dtype=np.int32), 10, A, mode=2)
        report("refused", "mode 2", rc == -3)
        A = 17  # seventeen pushes, then the joins: a stack of 17 whose par is right
        P = mixed_items(rng, 10, A)
        op = np.array([0] * A + [1] * (A - 1), dtype=np.uint8)
        rc, _, _ = raw(hip, op, bit_rows(P), par_of(op), 10, A)
        report("refused", "a stack of 17", rc == -2)
        op = np.array([0] * 16 + [1] * 15 + [0, 1], dtype=np.uint8)
        rc, gene, node = raw(hip, op, bit_rows(P), par_of(op), 10, A)
        report("refused", "a stack of 16 is taken", rc == 0 and np.array_equal(node[:16, 0], P.sum(axis=0)[:16]))
    elif which == "ties":  # the five cost pairs and both tie rules on 257 items over 65 leaves; every tie occurs
        A = 65
        kids = pr.tree(random_records(rng, A), A, "upgma")
        P = mixed_items(rng, 257, A)
        for g, l in COSTS:
            ties = {}
            for mode in MODES:
                report("ties", "g=%d l=%d %s" % (g, l, mode), entry_same(hip, P, kids, g, l, mode, ties))
            report("ties", "g=%d l=%d: the restatement met %s" % (g, l, ties), all(ties[k] >= 1 for k in gr.TIES))
    elif which == "chunks":  # PANGENE_GAINLOSS_CHUNK=1024 in this process: the node totals add across chunks
        A = 40
        report("chunks", "the chunk is 1 024", chunk(hip, A) == 1024)
        kids = pr.tree(random_records(rng, A), A, "upgma")
        for M in (1023, 1024, 1025, 3000):
            report("chunks", "%d items" % M, entry_same(hip, mixed_items(rng, M, A), kids, 2, 1, "late"))
    elif which == "buffers":  # the cached buffers: growing, shrinking, given back, and again
        def one(A, M):
            kids = pr.tree(random_records(rng, A), A, "upgma")
            return entry_same(hip, mixed_items(rng, M, A), kids, 1, 2, "early")
        for A, M in ((10, 40), (300, 700), (3, 5), (120, 2000), (64, 100)):
            report("buffers", "A=%d M=%d" % (A, M), one(A, M))
        hip.pg_trim_host_cache(0)
        report("buffers", "after trim", one(150, 500))
        hip.pg_trim_host_cache(0)
        report("buffers", "and again", one(150, 500))
    elif which == "range":  # sizes and costs the entry turns away before anything is launched
        A = 65536
        rc, _, _ = raw(hip, np.zeros(2 * A - 1, dtype=np.uint8), np.zeros((A, 1), dtype=np.uint32), np.zeros(2 * A - 1, dtype=np.int32), 10, A)
        report("range", "65 536 leaves", rc == -2)
        P = mixed_items(rng, 10, 4)
        op, par = np.array([0, 0, 1, 0, 1, 0, 1], dtype=np.uint8), np.array([2, 2, 4, 4, 6, 6, -1], dtype=np.int32)
        for g, l in ((0, 1), (256, 1), (1, 0), (1, 256)):
            rc, _, _ = raw(hip, op, bit_rows(P), par, 10, 4, g, l)
            report("range", "g=%d l=%d" % (g, l), rc == -2)
        rc, _, _ = raw(hip, op, bit_rows(P), par, 16777216, 4)
        report("range", "16 777 216 items", rc == -2)
        rc, _, _ = raw(hip, op, bit_rows(P), par, 10, 4, 255, 255)
        report("range", "g = l = 255 is taken", rc == 0)
        try:
            capi.pan_gainloss(hip, np.zeros((1, A), dtype=bool), pr.caterpillar_records(A), "upgma")
            report("range", "pg_pan_gainloss, 65 536 assemblies", False)
        except RuntimeError as e:
            report("range", "pg_pan_gainloss, 65 536 assemblies", "status -2" in str(e))
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
            for kw in gr.OPTION_SETS:
                rc1, a = file_table(hip, gfa, tmp, **kw)
                rc2, b = file_table(ora, gfa, tmp, **kw)
                ok = rc1 == 0 and rc2 == 0 and a == b and a.count(b"\n") >= 1
                if route == "file":
                    ok = ok and a == gr.table(gfa, **kw)
                else:
                    ok = ok and a == capi.run(hip, files, gr.option_args(**kw)[1])
                report(which, "%s" % (kw or "defaults"), ok)
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
