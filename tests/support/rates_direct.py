"""TEST INFRASTRUCTURE: direct pga_pan_rates / pg_pan_rates cases for tests/test_rates_gpu.py, run in a child process of their own so that
the test can bound them with a timeout.  The product library (the HIP kernels of k_rates.hpp) runs trees, sizes and tables no GFA
fixture reaches, with tables made by numpy; the restatement (tests/support/rates_ref.py) checks every likelihood with the exponents
aligned, gene, node and every entry of the posterior rows, within the bounds that follow from the arithmetic (rates_ref.tolerances).
file:NAME and memory:NAME put a fixture through pg_rates_file and `--rates` of the product and of the checker build, each compared with
the restatement.  Prints one line per case and "ALL OK" at the end; exits 1 at the first difference.

    python tests/support/rates_direct.py {shapes|trees|deep|exact|post|chunks|refused|buffers|same|fit|file:NAME|memory:NAME}"""
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
import rates_ref as rr  # noqa: E402
import tree_ref as tr  # noqa: E402
from gainloss_direct import mixed_items, par_of  # noqa: E402
from pairs_direct import bit_rows, random_records  # noqa: E402


class pga_rates_in_t(C.Structure):
    _fields_ = [("op", C.c_void_p), ("bits", C.c_void_p), ("par", C.c_void_p), ("n_gene", C.c_int32), ("n_leaf", C.c_int32), ("n_set", C.c_int32),
                ("tab", C.c_void_p), ("pi", C.c_void_p), ("post", C.c_int32), ("n_sum", C.c_int32), ("post_rows", C.c_void_p)]


class pga_rates_out_t(C.Structure):
    _fields_ = [("lik_m", C.c_void_p), ("lik_e", C.c_void_p), ("gene", C.c_void_p), ("node", C.c_void_p)]


def chunk(lib, n_leaf):
    lib.pga_rates_chunk.restype, lib.pga_rates_chunk.argtypes = C.c_int32, [C.c_int32]
    return lib.pga_rates_chunk(n_leaf)


def raw(lib, op, bits, par, G, L, tab, pi, n_set=None, post=0, n_sum=None, post_rows=None):
    """(status, lik_m (S, G), lik_e (S, G), gene (G, 3) or None, node (2 L - 1, 3) or None) of pga_pan_rates itself"""
    fn = lib.pga_pan_rates
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(pga_rates_in_t), C.POINTER(pga_rates_out_t)]
    S = len(pi) if n_set is None else n_set
    cin = pga_rates_in_t(op.ctypes.data, bits.ctypes.data, par.ctypes.data, G, L, S, tab.ctypes.data, pi.ctypes.data, post, G if n_sum is None else n_sum,
                         post_rows.ctypes.data if post_rows is not None else None)
    cout = pga_rates_out_t()
    rc = fn(C.byref(cin), C.byref(cout))
    if rc != 0:
        return rc, None, None, None, None
    n_op = max(2 * L - 1, 0)
    arr = lambda p, ty, shape: np.ctypeslib.as_array(C.cast(p, C.POINTER(ty)), shape=shape).copy() if shape[0] * shape[1] else np.zeros(shape)  # noqa: E731
    m, e = arr(cout.lik_m, C.c_double, (S, G)), arr(cout.lik_e, C.c_int32, (S, G))
    if not post:
        return 0, m, e, None, None
    return 0, m, e, arr(cout.gene, C.c_double, (G, 3)), arr(cout.node, C.c_double, (n_op, 3))


def random_tables(rng, n, n_set):
    """n_set parameter sets over a tree of n nodes: rates log-uniform in [2^-4, 2^4], branch lengths a random split of 1 with the floor"""
    t = rng.random(n) ** 3
    t = np.maximum(t / t.sum(), rr.T_FLOOR)
    t[-1] = 0.0
    sets = [rr.tables(2.0 ** rng.uniform(-4, 4), 2.0 ** rng.uniform(-4, 4), t) for _ in range(n_set)]
    return np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])


def entry_same(lib, P, kids, tabs, pis, post=0, n_sum=None, want_need=None, brute=False):
    """pga_pan_rates with the program of gainloss_ref against the restatement.  tabs (S, n, 4) and pis (S, 2) in node id order.  Every L
    with the exponents aligned; with post gene, node in op order and every entry of the first chunk's posterior rows."""
    M, A = P.shape
    op, order, need, node_of, par = gr.program(kids, A)
    if want_need is not None and need != want_need:
        return False
    bits = np.ascontiguousarray(bit_rows(P)[order])
    tab_op = np.ascontiguousarray(tabs[:, node_of])
    first = min(M, chunk(lib, A))
    rows = np.full((len(op), first), -7.0) if post else None
    rc, m, e, gene, node = raw(lib, op, bits, par, M, A, tab_op, np.ascontiguousarray(pis), post=post, n_sum=n_sum, post_rows=rows)
    if rc != 0:
        return False
    tol_L, tol_post, tol_node = rr.tolerances(A, M if n_sum is None else n_sum)
    for s in range(len(pis)):
        inn, _, wm, we = rr.up(P, kids, tabs[s], pis[s])
        if not (np.all((m[s] == 0) == (wm == 0)) and np.all((m[s] == 0) | ((m[s] >= 0.5) & (m[s] < 1.0)))):
            return False
        if not rr.close(np.ldexp(m[s], (e[s] - we).astype(np.int64)), wm, tol_L, 0.0):
            return False
        if s == 0 and post:
            present, g, l = rr.down(inn, kids, tabs[0], pis[0])
            k = M if n_sum is None else n_sum
            ok = rr.close(gene[:, 0], g.sum(axis=0), tol_post) and rr.close(gene[:, 1], l.sum(axis=0), tol_post) and rr.close(gene[:, 2], present[-1], tol_post)
            ok = ok and rr.close(rows, present[node_of][:, :first], tol_post)
            ok = ok and all(rr.close(node[:, c], w[node_of][:, :k].sum(axis=1), tol_node) for c, w in enumerate((present, g, l)))
            ok = ok and node[-1, 1] == 0 and node[-1, 2] == 0
            if not ok:
                return False
            if brute:  # and against the enumeration over all inner assignments
                for i in range(M):
                    L, bp, bg, bl = rr.brute(P[i], kids, tabs[0], pis[0])
                    if not (rr.close(np.ldexp(m[0, i], int(e[0, i])), L, 1e-12) and rr.close(rows[:, i], bp[node_of], 1e-12, 1e-15) and
                            rr.close(gene[i], [bg.sum(), bl.sum(), bp[-1]], 1e-12, 1e-15)):
                        return False
    return True


def report(label, what, ok):
    print("%s %s: %s" % (label, what, "ok" if ok else "DIFFERENT"), flush=True)
    if not ok:
        sys.exit(1)


def file_table(lib, gfa, tmp, **kw):
    """what pg_rates_file of this library prints for a GFA file"""
    from pangene_amd import capi
    lib.pg_set_output(tmp.encode())
    try:
        rc = lib.pg_rates_file(gfa.encode(), C.byref(capi.rates_opt(lib, **rr.capi_options(**kw))))
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
    rng = np.random.default_rng(11)
    if which == "shapes":  # items around the wave and the workgroup of 128 lanes, leaves around the 32-op word and the 32-leaf gather
        for A in (1, 2, 3, 31, 32, 33, 65):
            kids = pr.tree(random_records(rng, A), A, "upgma")
            ok = []
            for M in (1, 63, 64, 65, 127, 129, 257, 4097):
                n_set = (1, 2, 25)[(A + M) % 3]
                tabs, pis = random_tables(rng, 2 * A - 1, n_set)
                ok.append(entry_same(hip, mixed_items(rng, M, A), kids, tabs, pis, post=(M // 64) % 2))
            report("shapes", "n_leaf=%d, 8 item counts" % A, all(ok))
        one = np.zeros(1, dtype=np.uint8)
        rc, m, e, _, _ = raw(hip, one, one, one, 0, 0, np.zeros(4), np.ones((1, 2)))
        report("shapes", "nothing at all", rc == 0 and m.shape == (1, 0))
    elif which == "trees":  # a caterpillar (stack 2) and balanced trees of 2^k leaves (stack k + 1)
        A = 300
        kids = pr.tree(pr.caterpillar_records(A), A, "upgma")
        tabs, pis = random_tables(rng, 2 * A - 1, 2)
        report("trees", "caterpillar of 300, need 2", entry_same(hip, mixed_items(rng, 130, A), kids, tabs, pis, post=1, want_need=2))
        for k in range(1, 11):
            A = 1 << k
            kids = pr.tree(pr.balanced_records(A), A, "upgma")
            tabs, pis = random_tables(rng, 2 * A - 1, 1 + k % 2)
            report("trees", "balanced 2^%d, need %d" % (k, k + 1), entry_same(hip, mixed_items(rng, 70, A), kids, tabs, pis, post=1, want_need=k + 1))
    elif which == "deep":  # the depth limit with the full LDS footprint of both kernels: a balanced tree of 32 768 leaves, 65 items
        A = 32768
        kids = pr.tree(pr.balanced_records(A), A, "upgma")
        tabs, pis = random_tables(rng, 2 * A - 1, 1)
        report("deep", "balanced 2^15 x 65 items, need 16", entry_same(hip, mixed_items(rng, 65, A), kids, tabs, pis, post=1, want_need=16))
    elif which == "exact":  # every table entry 0.5: every L is exactly 2^-1200, below fp64's range without the rescaling
        A = 1200
        kids = pr.tree(pr.caterpillar_records(A), A, "upgma")
        op, order, need, node_of, par = gr.program(kids, A)
        P = mixed_items(rng, 130, A)
        rc, m, e, _, _ = raw(hip, op, np.ascontiguousarray(bit_rows(P)[order]), par, 130, A, np.full((1, 2 * A - 1, 4), 0.5), np.full((1, 2), 0.5))
        report("exact", "caterpillar of 1 200, L = 2^-1200", rc == 0 and bool(np.all(m == 0.5)) and bool(np.all(e == -1199)))
        _, _, wm, we = rr.up(P, kids, np.full((2 * A - 1, 4), 0.5), np.full(2, 0.5))
        report("exact", "and the restatement says so", bool(np.all(wm == 0.5)) and bool(np.all(we == -1199)))
        _, _, wm, _ = rr.up(P, kids, np.full((2 * A - 1, 4), 0.5), np.full(2, 0.5), rescale=False)
        report("exact", "which without the rescaling is zero", bool(np.all(wm == 0)))
    elif which == "post":  # the posteriors against the restatement, and against the enumeration at 7 and 9 leaves
        for A in (7, 9):
            for method in ("upgma", "nj"):
                P = mixed_items(rng, 40, A)
                rec = gr.records(P, "jaccard", method)
                kids, ln = rr.lengths(rec, A, method)
                t, _ = rr.normalise(ln)
                sets = [rr.tables(lam, mu, t) for lam, mu in ((0.7, 2.3), (4.0, 0.3))]
                report("post", "%d leaves, %s, brute force" % (A, method), entry_same(hip, P, kids, np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets]), post=1, brute=True))
        for A, M in ((33, 257), (65, 129), (200, 300)):
            kids = pr.tree(random_records(rng, A), A, "upgma")
            tabs, pis = random_tables(rng, 2 * A - 1, 3)
            report("post", "A=%d M=%d" % (A, M), entry_same(hip, mixed_items(rng, M, A), kids, tabs, pis, post=1, n_sum=M - 3))
    elif which == "chunks":  # PANGENE_RATES_CHUNK=256 in this process: the node totals add across chunks and leave the pseudo-item out
        A = 40
        report("chunks", "the chunk is 256", chunk(hip, A) == 256)
        kids = pr.tree(random_records(rng, A), A, "upgma")
        for M in (255, 256, 257, 1000):
            P = mixed_items(rng, M, A)
            P[-1] = False  # the trailing all-absent item
            tabs, pis = random_tables(rng, 2 * A - 1, 2)
            report("chunks", "%d items" % M, entry_same(hip, P, kids, tabs, pis, post=1, n_sum=M - 1))
    elif which == "refused":  # what the entry must turn away before anything is launched
        A = 4
        P = mixed_items(rng, 10, A)
        bits = bit_rows(P)
        tab, pi = random_tables(rng, 7, 1)
        good_op, good_par = [0, 0, 1, 0, 1, 0, 1], [2, 2, 4, 4, 6, 6, -1]
        for name, op, par, want in (("a good one", good_op, good_par, 0), ("a join of one entry", [0, 1, 0, 0, 1, 0, 1], good_par, -3),
                                    ("two entries left", [0, 0, 0, 1, 0, 0, 1], good_par, -3), ("an op of 2", [0, 0, 2, 0, 1, 0, 1], good_par, -3),
                                    ("a root with a parent", good_op, [2, 2, 4, 4, 6, 6, 0], -3), ("a leaf under the wrong join", good_op, [2, 4, 4, 4, 6, 6, -1], -3),
                                    ("a join under itself", good_op, [2, 2, 2, 4, 6, 6, -1], -3), ("a parent out of range", good_op, [2, 2, 4, 4, 6, 7, -1], -3)):
            rc = raw(hip, np.array(op, dtype=np.uint8), bits, np.array(par, dtype=np.int32), 10, A, tab, pi, post=1)[0]
            report("refused", name, rc == want)
        op, par = np.array(good_op, dtype=np.uint8), np.array(good_par, dtype=np.int32)
        for name, at, v in (("a NaN in tab", (0, 3, 1), np.nan), ("a negative entry of tab", (0, 5, 2), -1e-300), ("an infinite entry of tab", (0, 0, 0), np.inf)):
            bad = tab.copy()
            bad[at] = v
            report("refused", name, raw(hip, op, bits, par, 10, A, bad, pi)[0] == -3)
        report("refused", "a NaN in pi", raw(hip, op, bits, par, 10, A, tab, np.array([[np.nan, 0.5]]))[0] == -3)
        report("refused", "n_set 0", raw(hip, op, bits, par, 10, A, tab, pi, n_set=0)[0] == -3)
        report("refused", "n_set 65", raw(hip, op, bits, par, 10, A, np.repeat(tab, 65, axis=0), np.repeat(pi, 65, axis=0))[0] == -2)
        report("refused", "n_set 64 is taken", raw(hip, op, bits, par, 10, A, np.repeat(tab, 64, axis=0), np.repeat(pi, 64, axis=0))[0] == 0)
        report("refused", "post 2", raw(hip, op, bits, par, 10, A, tab, pi, post=2)[0] == -3)
        report("refused", "n_sum above n_gene", raw(hip, op, bits, par, 10, A, tab, pi, post=1, n_sum=11)[0] == -3)
        A = 17  # seventeen pushes, then the joins: a stack of 17 whose par is right
        P = mixed_items(rng, 10, A)
        tab, pi = random_tables(rng, 2 * A - 1, 1)
        op = np.array([0] * A + [1] * (A - 1), dtype=np.uint8)
        report("refused", "a stack of 17", raw(hip, op, bit_rows(P), par_of(op), 10, A, tab, pi, post=1)[0] == -2)
        op = np.array([0] * 16 + [1] * 15 + [0, 1], dtype=np.uint8)
        rc, m, _, _, node = raw(hip, op, bit_rows(P), par_of(op), 10, A, tab, pi, post=1)
        report("refused", "a stack of 16 is taken", rc == 0 and bool(np.all(m > 0)) and rr.close(node[:16, 0], P.sum(axis=0)[:16], 1e-12))
        rc = raw(hip, np.zeros(2 * 65536 - 1, dtype=np.uint8), np.zeros((65536, 1), dtype=np.uint32), np.zeros(2 * 65536 - 1, dtype=np.int32), 10, 65536, tab, pi)[0]
        report("refused", "65 536 leaves", rc == -2)
    elif which == "buffers":  # the cached buffers: growing, shrinking, given back, and again
        def one(A, M, post):
            kids = pr.tree(random_records(rng, A), A, "upgma")
            tabs, pis = random_tables(rng, 2 * A - 1, 2)
            return entry_same(hip, mixed_items(rng, M, A), kids, tabs, pis, post=post)
        for A, M, post in ((10, 40, 1), (300, 700, 0), (3, 5, 1), (120, 2000, 1), (64, 100, 0)):
            report("buffers", "A=%d M=%d post=%d" % (A, M, post), one(A, M, post))
        hip.pg_trim_host_cache(0)
        report("buffers", "after trim", one(150, 500, 1))
        hip.pg_trim_host_cache(0)
        report("buffers", "and again", one(150, 500, 1))
    elif which == "same":  # two calls return equal bits
        A, M = 65, 1000
        kids = pr.tree(random_records(rng, A), A, "upgma")
        op, order, need, node_of, par = gr.program(kids, A)
        bits = np.ascontiguousarray(bit_rows(mixed_items(rng, M, A))[order])
        tabs, pis = random_tables(rng, 2 * A - 1, 3)
        a = raw(hip, op, bits, par, M, A, np.ascontiguousarray(tabs[:, node_of]), pis, post=1)
        b = raw(hip, op, bits, par, M, A, np.ascontiguousarray(tabs[:, node_of]), pis, post=1)
        report("same", "two calls", a[0] == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:])))
    elif which == "fit":  # named cases of the fit through pg_pan_rates, torch tensors on the device among them
        for M, A, seed in ((300, 20, 1), (257, 65, 3)):
            for method in ("upgma", "nj"):
                report("fit", "lineage_presence(%d, %d, %d) %s" % (M, A, seed, method), rr.fit_same(hip, M, A, seed, method))
        P = tr.lineage_presence(300, 20, 1)
        P[5] = P[77] = False  # items absent everywhere: NaN rows, left out of the fit
        rec = gr.records(P, "jaccard", "upgma")
        got = capi.pan_rates(hip, torch.from_numpy(P).cuda(), rec, "upgma", 1.25, 0.75)
        report("fit", "given rates, two items absent everywhere", rr.model_same(got, rr.model(P, rec, "upgma", 1.25, 0.75), P) and bool(np.isnan(got["gains"][[5, 77]]).all()))
        same = P[:, :1].repeat(4, axis=1)  # all assemblies identical: no tree length, no model
        got = capi.pan_rates(hip, same, gr.records(same, "jaccard", "upgma"), "upgma")
        report("fit", "a tree without length", got["T"] == 0 and np.isnan(got["gain"]) and bool(np.isnan(got["lnL_item"]).all()))
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
            for kw in rr.OPTION_SETS:
                if route == "file":
                    rc1, a = file_table(hip, gfa, tmp, **kw)
                    rc2, b = file_table(ora, gfa, tmp, **kw)
                else:
                    rc1, a = 0, capi.run(hip, files, rr.option_args(**kw)[1])
                    rc2, b = 0, capi.run(ora, files, rr.option_args(**kw)[1])
                why = rr.check_table(a, gfa, **kw) or rr.check_table(b, gfa, **kw)
                report(which, "%s%s" % (kw or "defaults", ": " + why if why else ""), rc1 == 0 and rc2 == 0 and why == "" and a.count(b"\n") >= 2)
    else:
        sys.exit("unknown case " + which)
    print("ALL OK", flush=True)


if __name__ == "__main__":
    main()
