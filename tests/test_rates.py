"""Gain and loss rates (`pangene rates`, `pangene --rates`, pg_pan_rates) through the checker build: the host driver linked against the
oracle backend, whose table has no pan_rates entry, so the likelihoods and posteriors come from the plain loops of pan_rates.hpp over the
records' tree, node by node in join order.  Everything is compared with the numpy restatement of tests/support/rates_ref.py within the
bounds that follow from the arithmetic, and that with a brute force over all inner-node assignments."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
sys.path.insert(0, ROOT)
import gainloss_ref as gr  # noqa: E402
import pairs_ref as pr  # noqa: E402
import rates_ref as rr  # noqa: E402
import tree_ref as tr  # noqa: E402

NAMES = ["C4", "bact20", "human8"]
RATES = ((1.0, 1.0), (0.7, 2.3), (4.0, 0.3), (1e-3, 50.0))


def run_cli(args, exe=CLI):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.returncode, r.stdout, r.stderr


def gfa_of(name):
    return os.path.join(GOLD, name + ".gfa.gz")


def pafs_of(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    return oracle_host.load()


def all_patterns(A):
    return (np.arange(1 << A)[:, None] >> np.arange(A)[None, :] & 1).astype(bool)


def test_restatement_against_brute_force():
    """the two passes of the restatement against the enumeration over all 2^(A - 1) inner assignments: A = 3 .. 9, both methods, four
    rate pairs; L, every node's posterior and every branch's gain and loss at 1e-12"""
    rng = np.random.default_rng(2)
    for A in range(3, 10):
        P = all_patterns(A) if A <= 5 else rng.random((12, A)) < 0.5
        for method in ("upgma", "nj"):
            Q = rng.random((40, A)) < 0.5  # the items the tree is built from
            kids, ln = rr.lengths(gr.records(Q, "jaccard", method), A, method)
            t, T = rr.normalise(ln)
            assert T > 0
            for lam, mu in RATES:
                tab, pi = rr.tables(lam, mu, t)
                inn, _, m, e = rr.up(P, kids, tab, pi)
                present, g, l = rr.down(inn, kids, tab, pi)
                for i in range(len(P)):
                    L, bp, bg, bl = rr.brute(P[i], kids, tab, pi)
                    assert rr.close(math.ldexp(m[i], int(e[i])), L, 1e-12), (A, method, lam, mu, i)
                    assert rr.close(present[:, i], bp, 1e-12, 1e-15) and rr.close(g[:, i], bg, 1e-12, 1e-15) and rr.close(l[:, i], bl, 1e-12, 1e-15), (A, method, lam, mu, i)


def _newick_lengths(text):
    """{frozenset of leaf names: the length printed above that subtree} of a Newick line without quoted names"""
    out, pos = {}, 0

    def node():
        nonlocal pos
        if text[pos] == "(":
            pos += 1
            leaves = set()
            while True:
                leaves |= node()
                if text[pos] == ",":
                    pos += 1
                    continue
                pos += 1  # ")"
                break
            while text[pos] not in ":,);":  # (a support label)
                pos += 1
        else:
            a = pos
            while text[pos] not in ":,);":
                pos += 1
            leaves = {text[a:pos]}
        if text[pos] == ":":
            a = pos + 1
            pos = a
            while text[pos] not in ",);":
                pos += 1
            out[frozenset(leaves)] = float(text[a:pos])
        return leaves
    node()
    return out


@pytest.mark.parametrize("name", NAMES)
def test_lengths_against_newick(built, name):
    """the raw branch lengths against the numbers in the line `pangene tree` prints (six decimals): every branch but the two under the
    root as printed; under NJ's root the third branch of the closing record, halved"""
    for method in ("upgma", "nj"):
        rc, out, err = run_cli(["tree", "-a", method, gfa_of(name)])
        assert rc == 0, err
        names, _, P, rec = rr.items_tree(gfa_of(name), method=method)
        A = len(names)
        assert not any(c in n for n in names for c in "(),:;[]' ")
        kids, ln = rr.lengths(rec, A, method)
        printed = _newick_lengths(out.decode().strip())
        below = [frozenset([n]) for n in names]
        for a, b in kids:
            below.append(below[a] | below[b])
        top = kids[-1]
        checked = 0
        for v in range(A + len(kids) - 1):
            if method == "nj" and v in top:
                z = top[1]
                assert abs(ln[v] / 2.0 ** 20 - printed[below[z]] / 2) <= 5e-7
            else:
                assert abs(ln[v] / 2.0 ** 20 - printed[below[v]]) <= 5e-7, (method, v)
            checked += 1
        assert checked == 2 * A - 2


@pytest.mark.parametrize("name", NAMES)
def test_file_route(built, name):
    """`pangene rates` of the checker build against the restatement for the five option sets: given rates, then the fit"""
    for kw in rr.OPTION_SETS:
        rc, out, err = run_cli(["rates"] + rr.option_args(**kw)[0] + [gfa_of(name)])
        assert rc == 0, err
        assert rr.check_table(out, gfa_of(name), **kw) == "", kw
        assert out.count(b"\n") > 2 or kw.get("min_changes")
    rc, out, err = run_cli(["rates", gfa_of(name)])  # and the defaults without any option
    assert rc == 0 and out.startswith(rr.GENE_HEADER) and rr.check_table(out, gfa_of(name)) == ""


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, tmp_path, name):
    """`pangene --rates ... *.paf` against the restatement over the GFA of the same run"""
    files = pafs_of(name)
    rc, gfa, err = run_cli(files)
    assert rc == 0, err
    path = str(tmp_path / "g.gfa")
    with open(path, "wb") as f:
        f.write(gfa)
    for kw in rr.OPTION_SETS:
        rc, a, err = run_cli(rr.option_args(**kw)[1] + files)
        assert rc == 0, err
        assert rr.check_table(a, path, **kw) == "", kw
    if name == "C4":  # and capi.run, the same route in-process
        import ctypes as C
        import oracle_host
        from pangene_amd import capi
        lib = oracle_host.load()
        C.c_int.in_dll(lib, "pg_verbose").value = 0
        kw = rr.OPTION_SETS[1]
        assert rr.check_table(capi.run(lib, files, rr.option_args(**kw)[1]), path, **kw) == ""
        with pytest.raises(ValueError):
            capi.run(lib, files, ["--rates-gain=2", "--rates-loss=1"])
        with pytest.raises(ValueError):
            capi.run(lib, files, ["--rates", "--rates-gain=2"])
        with pytest.raises(ValueError):
            capi.run(lib, files, ["--rates", "--gainloss"])


@pytest.mark.parametrize("name", NAMES)
def test_entry_on_fixtures(ora, name):
    """pg_pan_rates of the checker build on the fixtures' items and records: every number against the restatement at given rates; fitted,
    every number at the rates it returns"""
    from pangene_amd import capi
    for method in ("upgma", "nj"):
        _, _, P, rec = rr.items_tree(gfa_of(name), method=method)
        got = capi.pan_rates(ora, P, rec, method, 1.5, 2.0)
        assert got["rounds"] == 0 and got["converged"] == 1 and got["gain"] == 1.5 and got["loss"] == 2.0
        assert rr.model_same(got, rr.model(P, rec, method, 1.5, 2.0), P)
        got = capi.pan_rates(ora, P, rec, method)
        assert got["rounds"] >= 12 and rr.model_same(got, rr.model(P, rec, method, got["gain"], got["loss"]), P)


@pytest.mark.parametrize("case", [(300, 20, 1), (500, 40, 2), (257, 65, 3)])
def test_named_fits(ora, case):
    """The named cases of the fit: the restatement's smallest gap between the best and the second-best lattice value is at least 100
    times the bound on lnL (rates_ref.fit_same checks that itself), so the lattice paths coincide and the rates agree at 1e-12"""
    for method in ("upgma", "nj"):
        assert rr.fit_same(ora, *case, method), method


def test_invariants(ora):
    """the sums over the items' gains and losses are the sums over the nodes'; a leaf's posterior is its bit; lnL at the fitted point is
    at least lnL at its eight lattice neighbours; items absent everywhere are NaN and change nothing"""
    from pangene_amd import capi
    P = tr.lineage_presence(300, 20, 1)
    M, A = P.shape
    rec = gr.records(P, "jaccard", "upgma")
    got = capi.pan_rates(ora, P, rec, "upgma")
    tol = rr.tolerances(A, M)[2] + M * rr.EPS
    assert rr.close(np.nansum(got["gains"]), got["node_gains"].sum(), tol) and rr.close(np.nansum(got["losses"]), got["node_losses"].sum(), tol)
    assert rr.close(got["node_present"][:A], P.sum(axis=0), tol)
    assert got["node_gains"][-1] == 0 and got["node_losses"][-1] == 0 and rr.close(np.nansum(got["lnL_item"]), got["lnL"], 1e-12)
    h = 2.0 ** -10
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            other = capi.pan_rates(ora, P, rec, "upgma", got["gain"] * 2.0 ** (i * h), got["loss"] * 2.0 ** (j * h))
            assert other["lnL"] <= got["lnL"] + 2 * rr.model(P, rec, "upgma", got["gain"], got["loss"])["bound"], (i, j)
    Q = np.vstack([P[:100], np.zeros((2, A), dtype=bool), P[100:]])
    more = capi.pan_rates(ora, Q, rec, "upgma", got["gain"], got["loss"])
    keep = np.r_[0:100, 102:M + 2]
    assert np.isnan(more["gains"][100:102]).all() and np.isnan(more["rate"][100:102]).all()
    same = capi.pan_rates(ora, P, rec, "upgma", got["gain"], got["loss"])
    assert more["lnL"] == same["lnL"] and np.array_equal(more["gains"][keep], same["gains"], equal_nan=True) and np.array_equal(more["node_present"], same["node_present"])


def test_extended_precision():
    """the 64-bit up pass against the 80-bit one stays inside the bound of an L, 8 (2 A - 1) 2^-53, on a random tree of 65 leaves, a
    caterpillar of 1 200 and a balanced tree of 1 024 leaves"""
    assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble has no 64-bit mantissa here"
    rng = np.random.default_rng(4)
    from pairs_direct import random_records
    for A, rec in ((65, random_records(rng, 65)), (1200, pr.caterpillar_records(1200)), (1024, pr.balanced_records(1024))):
        kids = pr.tree(rec, A, "upgma")
        t = rng.random(2 * A - 1) ** 3
        t = np.maximum(t / t.sum(), rr.T_FLOOR)
        tab, pi = rr.tables(1.3, 2.1, t)
        P = rng.random((50, A)) < rng.random(50)[:, None]
        _, _, m, e = rr.up(P, kids, tab, pi)
        _, _, ml, el = rr.up(P, kids, tab, pi, dtype=np.longdouble)
        d = np.abs(np.ldexp(m.astype(np.longdouble), (e - el).astype(np.int64)) - ml) / ml
        assert float(d.max()) <= rr.tolerances(A)[0], (A, float(d.max()))


def test_option_errors(built):
    """one rate without the other, rates out of range and unknown words: status 1 and nothing on stdout"""
    gfa = gfa_of("C4")
    for args in (["-g", "1"], ["-l", "2"], ["-g", "0", "-l", "1"], ["-g", "-1", "-l", "1"], ["-g", "nan", "-l", "1"], ["-g", "1e10", "-l", "1"], ["-g", "x", "-l", "1"],
                 ["-o", "tree"], ["-t", "walk"], ["-m", "shared"], ["-a", "ml"], ["-c", "-1"], ["-c", "x"]):
        rc, out, err = run_cli(["rates"] + args + [gfa])
        assert rc == 1 and out == b"" and err != b"", args
    files = pafs_of("C4")
    for args in (["--rates-gain=1", "--rates-loss=1"], ["--rates", "--rates-gain=1"], ["--rates=tree"], ["--rates", "--rates-loss=0"], ["--rates", "--gainloss"]):
        rc, out, err = run_cli(args + files)
        assert rc == 1 and out == b"" and err != b"", args
    rc, out, err = run_cli(["--gpus", "2", "--rates"] + files)
    assert rc == 1 and out == b"" and b"--rates" in err


def test_no_model(built, ora, tmp_path):
    """fewer than two assemblies, or assemblies that are all identical: the header only, a note on stderr, status 0; pg_pan_rates returns
    NaN rates"""
    from pangene_amd import capi
    gfa = str(tmp_path / "same.gfa")
    with open(gfa, "w") as f:
        f.write("S\tg1\t*\nS\tg2\t*\n")
        for a in ("x", "y", "z"):
            f.write("W\t%s\t0\tc\t0\t10\t>g1>g2\n" % a)
    for out_kind, head in (("gene", rr.GENE_HEADER), ("node", rr.NODE_HEADER)):
        rc, out, err = run_cli(["rates", "-o", out_kind, gfa])
        assert rc == 0 and out == head and b"no model" in err, (out, err)
    P = np.ones((5, 3), dtype=bool)
    got = capi.pan_rates(ora, P, gr.records(P, "jaccard", "upgma"), "upgma")
    assert got["T"] == 0 and math.isnan(got["gain"]) and np.isnan(got["gains"]).all()
    got = capi.pan_rates(ora, np.ones((5, 1), dtype=bool), None, "upgma")
    assert math.isnan(got["gain"]) and got["rounds"] == 0
    with pytest.raises(RuntimeError, match="status -3"):
        capi.pan_rates(ora, P, np.array([[0, 0, 0, 0, 0, 3], [0, 2, 0, 0, 0, 2]]), "upgma")
    with pytest.raises(ValueError):
        capi.pan_rates(ora, P, gr.records(P, "jaccard", "upgma"), "upgma", 1.0, 0.0)
