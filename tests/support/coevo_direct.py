"""TEST INFRASTRUCTURE: direct pga_pan_coevo / pg_pan_coevo cases for tests/test_coevo_gpu.py, run in a child process of their own so that
the test can bound them with a timeout.  The product library (the HIP kernels of k_coevo.hpp over k_gainloss.hpp) runs trees and sizes no
GFA fixture reaches; the restatement (tests/support/coevo_ref.py) checks the events, every pair record and every word of the event rows
(the tests-only ev_rows output).  file:NAME and memory:NAME put a fixture through pg_coevo_file and pg_write_coevo of the product and of the
checker build for every option set, in this one process, so that the device comes up once.  Prints one line per case and "ALL OK" at the
end; exits 1 at the first difference.

    python tests/support/coevo_direct.py {shapes|leaves|wide|tiles|chunks|cap|buffers|refused|range|file:NAME|memory:NAME}"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import coevo_ref as cr  # noqa: E402
import gainloss_ref as gr  # noqa: E402
import pairs_ref as pr  # noqa: E402
from gainloss_direct import mixed_items, par_of, report  # noqa: E402
from pairs_direct import bit_rows, random_records  # noqa: E402

MODES = ("late", "early")
SENTINEL = 0xA5A5A5A5


class pga_coevo_in_t(C.Structure):
    _fields_ = [("op", C.c_void_p), ("bits", C.c_void_p), ("par", C.c_void_p), ("n_gene", C.c_int32), ("n_leaf", C.c_int32), ("gain", C.c_int32),
                ("loss", C.c_int32), ("mode", C.c_int32), ("min_events", C.c_int32), ("r_permille", C.c_int32), ("sign", C.c_int32), ("max_pair", C.c_int64),
                ("ev_rows", C.c_void_p), ("ev_cap", C.c_int64)]


class pga_coevo_out_t(C.Structure):
    _fields_ = [("events", C.c_void_p), ("n_pair", C.c_int64), ("pair", C.c_void_p)]


def chunk(lib, n_leaf):
    lib.pga_coevo_chunk.restype, lib.pga_coevo_chunk.argtypes = C.c_int32, [C.c_int32]
    return lib.pga_coevo_chunk(n_leaf)


def raw(lib, op, bits, par, G, L, g=1, l=1, mode=0, c=2, p=800, sign=0, max_pair=1 << 24, ev=None):
    """(status, events (G,) int32, pairs (n, 4) int32, n) of pga_pan_coevo itself"""
    fn = lib.pga_pan_coevo
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(pga_coevo_in_t), C.POINTER(pga_coevo_out_t)]
    cin = pga_coevo_in_t(op.ctypes.data, bits.ctypes.data, par.ctypes.data, G, L, g, l, mode, c, p, sign, max_pair, ev.ctypes.data if ev is not None else None,
                         ev.shape[0] if ev is not None else 0)
    cout = pga_coevo_out_t()
    rc = fn(C.byref(cin), C.byref(cout))
    if rc != 0:
        return rc, None, None, cout.n_pair
    events = np.ctypeslib.as_array(C.cast(cout.events, C.POINTER(C.c_int32)), shape=(G,)).copy() if G else np.zeros(0, dtype=np.int32)
    n = cout.n_pair
    pairs = np.ctypeslib.as_array(C.cast(cout.pair, C.POINTER(C.c_int32)), shape=(n, 4)).copy() if n else np.zeros((0, 4), dtype=np.int32)
    return 0, events, pairs, n


def entry_same(lib, P, kids, g=1, l=1, mode="late", c=2, p=800, sign="both", want_E=None, want_more_than=None):
    """pga_pan_coevo with the program of gainloss_ref against the restatement: the events, every pair record, every word of the event rows
    (one row of room past the E the restatement expects, which must stay untouched)"""
    M, A = P.shape
    op, order, need, node_of, par = gr.program(kids, A)
    bits = np.ascontiguousarray(bit_rows(P)[order])
    B = max(2 * A - 2, 0)
    WB = (B + 31) // 32
    if A >= 2:
        X, _ = cr.events(P, kids, g, l, mode)
        e_want, p_want = cr.select(P, kids, g, l, mode, p / 1000.0, c, sign)
        X_op = X[node_of[:B]]
    else:
        X_op, e_want, p_want = np.zeros((0, M), dtype=np.int8), np.zeros(M, dtype=np.int64), np.zeros((0, 4), dtype=np.int64)
    el = np.flatnonzero(e_want >= c)
    if want_E is not None and len(el) != want_E:
        return False
    if want_more_than is not None and len(p_want) <= want_more_than:
        return False
    ev = np.full((len(el) + 1, 2, max(WB, 1)), SENTINEL, dtype=np.uint32)
    rc, events, pairs, n = raw(lib, op, bits, par, M, A, g, l, MODES.index(mode), c, p, cr.SIGNS.index(sign), ev=ev)
    if rc != 0:
        return False
    ok = np.array_equal(events, e_want) and n == len(p_want) and np.array_equal(pairs, p_want)
    if A >= 2 and len(el) > 0:
        ok = ok and np.array_equal(ev[:len(el), :, :WB], cr.event_rows(X_op, el, WB))
    return ok and bool((ev[len(el)] == SENTINEL).all())


def items_with(rng, M, where, A, kids, c=2):
    """M items of which exactly those at `where` have at least c events: random rows there (drawn again while they have fewer), constant
    rows elsewhere"""
    P = np.zeros((M, A), dtype=bool)
    P[1::2] = True
    P[where] = False
    todo = np.asarray(where)
    while len(todo):
        P[todo] = rng.random((len(todo), A)) < 0.5
        res = gr.reconstruct(P[todo], kids)
        todo = todo[(res["gains"] + res["losses"]) < c]
    return P


def file_table(lib, gfa, tmp, **kw):
    """what pg_coevo_file of this library prints for a GFA file"""
    from pangene_amd import capi
    lib.pg_set_output(tmp.encode())
    try:
        rc = lib.pg_coevo_file(gfa.encode(), C.byref(capi.coevo_opt(lib, **cr.capi_options(**kw))))
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
    rng = np.random.default_rng(15)
    if which == "shapes":  # items around the ballot word and the workgroup of 128 lanes
        for A in (3, 17):
            rec = random_records(rng, A)
            kids = pr.tree(rec, A, "upgma")
            ok = []
            for M in (1, 63, 64, 65, 129, 4097):
                P = mixed_items(rng, M, A)
                g, l = ((1, 1), (2, 1), (1, 3))[M % 3]
                ok.append(entry_same(hip, P, kids, g, l, MODES[M % 2], c=1 + M % 2, p=(300, 800)[A == 3], sign=cr.SIGNS[M % 3]))
                if M in (65, 129):  # and through the C API, torch tensors on the device
                    e, pairs = capi.pan_coevo(hip, torch.from_numpy(P).cuda(), rec, "upgma", g, l, MODES[M % 2], 0.5, 1, "both")
                    we, wp = cr.select(P, kids, g, l, MODES[M % 2], 0.5, 1, "both")
                    ok.append(np.array_equal(e, we) and np.array_equal(pairs, wp))
            report("shapes", "n_leaf=%d, 6 item counts" % A, all(ok))
        rc, events, pairs, n = raw(hip, *[np.zeros(1, dtype=np.uint8)] * 3, 0, 0)
        report("shapes", "nothing at all", rc == 0 and events.shape == (0,) and n == 0)
        import oracle_host
        ora = oracle_host.load()
        for method in ("nj", "upgma"):  # real trees, against the checker build too
            P = mixed_items(rng, 300, 21)
            rec, _ = capi.pan_tree(hip, P, "jaccard", method)
            e, pairs = capi.pan_coevo(hip, P, rec, method, 2, 1, "early", 0.4, 2, "both")
            we, wp = cr.select(P, pr.tree(rec, 21, method), 2, 1, "early", 0.4, 2, "both")
            oe, op_ = capi.pan_coevo(ora, P, rec, method, 2, 1, "early", 0.4, 2, "both")
            report("shapes", "pg_pan_tree's records " + method, len(wp) > 0 and np.array_equal(e, we) and np.array_equal(pairs, wp) and np.array_equal(e, oe) and
                   np.array_equal(pairs, op_))
    elif which == "leaves":  # B = 0, 2, 4, 32, 64, 66, 128 branches: the 32-bit word, the 64-branch ballot group; caterpillars and balanced trees
        for A in (1, 2, 3, 17, 33, 34, 65):
            for name, rec in (("caterpillar", pr.caterpillar_records(A)), ("balanced", pr.balanced_records(A))):
                kids = pr.tree(rec, A, "upgma")
                P = mixed_items(rng, 130, A)
                report("leaves", "%s of %d" % (name, A), entry_same(hip, P, kids, 1, 1, MODES[A % 2], c=1, p=500))
    elif which == "wide":  # B = 1 024 and 1 026: one span of k_ce_rows and one K chunk of k_ce_pairs exactly, and one word more
        for A in (513, 514):
            for name, rec in (("caterpillar", pr.caterpillar_records(A)), ("balanced", pr.balanced_records(A))):
                kids = pr.tree(rec, A, "upgma")
                P = mixed_items(rng, 140, A)
                P[::7] ^= rng.random((len(P[::7]), A)) < 0.01  # (and a few items with few events)
                report("wide", "%s of %d" % (name, A), entry_same(hip, P, kids, 1, 1, "late", c=2, p=200, want_more_than=0))
    elif which == "tiles":  # E around the 128 x 128 tile
        A = 24
        kids = pr.tree(random_records(rng, A), A, "upgma")
        for E in (1, 2, 127, 128, 129, 257):
            M = E + 40
            where = np.sort(rng.choice(M, size=E, replace=False))
            report("tiles", "E=%d of %d items" % (E, M), entry_same(hip, items_with(rng, M, where, A, kids), kids, p=300, want_E=E))
        M = 3000  # a scattered tenth: the places matter
        where = np.sort(rng.choice(M, size=300, replace=False))
        report("tiles", "E=300 scattered over 3 000 items", entry_same(hip, items_with(rng, M, where, A, kids), kids, p=300, want_E=300, want_more_than=100))
    elif which == "chunks":  # PANGENE_COEVO_CHUNK=1024 in this process: rows written by different chunks meet in one tile
        A = 40
        report("chunks", "the chunk is 1 024", chunk(hip, A) == 1024)
        kids = pr.tree(random_records(rng, A), A, "upgma")
        for M in (1023, 1024, 1025, 3000):
            where = np.sort(rng.choice(M, size=200, replace=False))
            P = items_with(rng, M, where, A, kids)
            report("chunks", "%d items, 200 eligible" % M, entry_same(hip, P, kids, p=400, want_E=200, want_more_than=10))
        report("chunks", "3 000 items, all random", entry_same(hip, mixed_items(rng, 3000, A), kids, 2, 1, "early", c=3, p=600, want_more_than=10))
    elif which == "cap":  # PANGENE_COEVO_CAP=16 in this process: the second run of k_ce_pairs
        A = 30
        kids = pr.tree(random_records(rng, A), A, "upgma")
        for M in (200, 700):
            report("cap", "%d items, more than 16 pairs" % M, entry_same(hip, mixed_items(rng, M, A), kids, p=400, want_more_than=16))
        op, order, need, node_of, par = gr.program(kids, A)
        P = mixed_items(rng, 200, A)
        rc, _, _, n = raw(hip, op, np.ascontiguousarray(bit_rows(P)[order]), par, 200, A, p=400, max_pair=20)
        report("cap", "max_pair below the count", rc == -2 and n == len(cr.select(P, kids, min_r=0.4)[1]) > 20)
    elif which == "buffers":  # the cached buffers: growing, shrinking, given back, and again
        def one(A, M):
            kids = pr.tree(random_records(rng, A), A, "upgma")
            return entry_same(hip, mixed_items(rng, M, A), kids, 1, 2, "early", p=500)
        for A, M in ((10, 40), (300, 700), (3, 5), (120, 2000), (64, 100)):
            report("buffers", "A=%d M=%d" % (A, M), one(A, M))
        hip.pg_trim_host_cache(0)
        report("buffers", "after trim", one(150, 500))
        hip.pg_trim_host_cache(0)
        report("buffers", "and again", one(150, 500))
    elif which == "refused":  # programs and options the entry must turn away before anything is launched
        A = 4
        P = mixed_items(rng, 10, A)
        bits = bit_rows(P)
        good_op, good_par = [0, 0, 1, 0, 1, 0, 1], [2, 2, 4, 4, 6, 6, -1]
        for name, op, par, want in (("a good one", good_op, good_par, 0), ("a join of one entry", [0, 1, 0, 0, 1, 0, 1], good_par, -3),
                                    ("two entries left", [0, 0, 0, 1, 0, 0, 1], good_par, -3), ("an op of 2", [0, 0, 2, 0, 1, 0, 1], good_par, -3),
                                    ("a root with a parent", good_op, [2, 2, 4, 4, 6, 6, 0], -3), ("a leaf under the wrong join", good_op, [2, 4, 4, 4, 6, 6, -1], -3),
                                    ("a join under itself", good_op, [2, 2, 2, 4, 6, 6, -1], -3), ("a parent of -1 below the root", good_op, [2, 2, 4, 4, -1, 6, -1], -3),
                                    ("a parent out of range", good_op, [2, 2, 4, 4, 6, 7, -1], -3)):
            rc, _, _, _ = raw(hip, np.array(op, dtype=np.uint8), bits, np.array(par, dtype=np.int32), 10, A)
            report("refused", name, rc == want)
        op, par = np.array(good_op, dtype=np.uint8), np.array(good_par, dtype=np.int32)
        for name, kw in (("mode 2", {"mode": 2}), ("min_events 0", {"c": 0}), ("r_permille 1001", {"p": 1001}), ("r_permille -1", {"p": -1}), ("sign 3", {"sign": 3}),
                         ("max_pair -1", {"max_pair": -1})):
            rc, _, _, _ = raw(hip, op, bits, par, 10, A, **kw)
            report("refused", name, rc == -3)
        A = 17  # seventeen pushes, then the joins: a stack of 17 whose par is right
        P = mixed_items(rng, 10, A)
        op = np.array([0] * A + [1] * (A - 1), dtype=np.uint8)
        rc, _, _, _ = raw(hip, op, bit_rows(P), par_of(op), 10, A)
        report("refused", "a stack of 17", rc == -2)
        op = np.array([0] * 16 + [1] * 15 + [0, 1], dtype=np.uint8)
        rc, events, _, _ = raw(hip, op, bit_rows(P), par_of(op), 10, A)
        report("refused", "a stack of 16 is taken", rc == 0 and events.shape == (10,))
    elif which == "range":  # sizes and costs the entry turns away before anything is launched
        A = 65536
        rc, _, _, _ = raw(hip, np.zeros(2 * A - 1, dtype=np.uint8), np.zeros((A, 1), dtype=np.uint32), np.zeros(2 * A - 1, dtype=np.int32), 10, A)
        report("range", "65 536 leaves", rc == -2)
        P = mixed_items(rng, 10, 4)
        op, par = np.array([0, 0, 1, 0, 1, 0, 1], dtype=np.uint8), np.array([2, 2, 4, 4, 6, 6, -1], dtype=np.int32)
        for g, l in ((0, 1), (256, 1), (1, 0), (1, 256)):
            rc, _, _, _ = raw(hip, op, bit_rows(P), par, 10, 4, g, l)
            report("range", "g=%d l=%d" % (g, l), rc == -2)
        rc, _, _, _ = raw(hip, op, bit_rows(P), par, 16777216, 4)
        report("range", "16 777 216 items", rc == -2)
        rc, _, _, _ = raw(hip, op, bit_rows(P), par, 10, 4, 255, 255)
        report("range", "g = l = 255 is taken", rc == 0)
        try:
            capi.pan_coevo(hip, np.zeros((1, A), dtype=bool), pr.caterpillar_records(A), "upgma")
            report("range", "pg_pan_coevo, 65 536 assemblies", False)
        except RuntimeError as e:
            report("range", "pg_pan_coevo, 65 536 assemblies", "status -2" in str(e))
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
            for kw in ({},) + cr.OPTION_SETS:
                rc1, a = file_table(hip, gfa, tmp, **kw)
                rc2, b = file_table(ora, gfa, tmp, **kw)
                ok = rc1 == 0 and rc2 == 0 and a == b and a.startswith(cr.HEADER)
                if route == "file":
                    cr.compare(a, cr.table_rows(gfa, **kw))
                else:
                    ok = ok and a == capi.run(hip, files, cr.option_args(**kw)[1])
                report(which, "%s, %d lines" % (kw or "defaults", a.count(b"\n")), ok)
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
