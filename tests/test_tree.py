"""Trees of the assemblies (`pangene tree`, `pangene --tree`, pg_pan_join, pg_pan_tree) through the checker build: the host driver
linked against the oracle backend, whose table has no pan_join entry, so the joins run as the plain loops of tree.cpp.  Everything is
compared with the numpy restatement of tests/support/tree_ref.py."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
sys.path.insert(0, ROOT)
import dist_ref as dr  # noqa: E402
import tree_ref as tr  # noqa: E402

GFAS = sorted(os.path.join(GOLD, f) for f in os.listdir(GOLD) if f.endswith(".gfa.gz")) + \
    sorted(os.path.join(GOLD, "bubble", f) for f in os.listdir(os.path.join(GOLD, "bubble")) if f.endswith(".gfa"))


def run_cli(args, exe=CLI):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    return oracle_host.load()


@pytest.mark.parametrize("gfa", GFAS, ids=[os.path.relpath(g, GOLD) for g in GFAS])
def test_fixture_files(built, gfa):
    for kind in ("gene", "adj"):
        names, P = dr.presence(gfa, kind)
        S = dr.shared(P)
        for metric in tr.METRICS:
            for method in tr.METHODS:
                args = ["tree", "-t", kind, "-m", metric, "-a", method, gfa]
                rc, out, err = run_cli(args)
                assert rc == 0, err
                assert out == tr.text(names, S, metric, method), " ".join(args)
    rc, out, _ = run_cli(["tree", gfa])
    assert rc == 0 and out == tr.text(*_gene(gfa))


def _gene(gfa):
    names, P = dr.presence(gfa, "gene")
    return names, dr.shared(P)


# (A, method) -> (items, seed, share of exact copies): lineage-structured presence matrices for which the restatement meets a tied minimum
JOIN_CASES = {
    (3, "nj"): (40, 1, 0.5), (3, "upgma"): (40, 2, 0.5), (4, "nj"): (40, 1, 0.5), (4, "upgma"): (40, 2, 0.5),
    (5, "nj"): (40, 1, 0.5), (5, "upgma"): (40, 2, 0.5), (17, "nj"): (200, 1, 0.3), (17, "upgma"): (200, 1, 0.3),
    (64, "nj"): (500, 1, 0.15), (64, "upgma"): (500, 1, 0.15), (65, "nj"): (500, 1, 0.15), (65, "upgma"): (500, 1, 0.15),
    (129, "nj"): (800, 1, 0.15), (129, "upgma"): (800, 1, 0.15), (300, "nj"): (1000, 1, 0.15), (300, "upgma"): (1000, 1, 0.15),
}


@pytest.mark.parametrize("A,method", sorted(JOIN_CASES), ids=["A%d-%s" % c for c in sorted(JOIN_CASES)])
def test_pan_join_against_the_restatement(ora, A, method):
    from pangene_amd import capi
    M, seed, dup = JOIN_CASES[(A, method)]
    P = tr.lineage_presence(M, A, seed, dup=dup)
    metric = "jaccard" if A % 2 else "diff"
    q, F = tr.fixed(dr.shared(P), metric)
    stats = {}
    want = tr.joins(q, method, stats)
    if not (A == 3 and method == "nj"):  # (three leaves under nj: the closing record alone, no minimum is ever taken)
        assert stats["n_tied"] >= 1, "the input has no tied minimum: pick another seed"
    got = capi.pan_join(ora, q.astype(np.int32), method)
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)
    rec, F2 = capi.pan_tree(ora, P, metric, method)
    assert F2 == F and np.array_equal(rec, want)


# a 12-leaf tree, edge lengths in units of 2^-9 (even multiples of 2^-10): (children or leaf number, length)
KNOWN = [([([(0, 2), (1, 4)], 6), ([(2, 8), (3, 2)], 4)], 2),
         ([([(4, 6), ([(5, 2), (6, 10)], 4)], 8), (7, 12)], 2),
         ([([(8, 4), (9, 4)], 6), ([(10, 2), (11, 16)], 2)], 10)]
UNIT = 1 << 11  # 2^-9 in units of 2^-20


def _known_edges():
    """{leaves below the edge (the side without leaf 11, as a frozenset): length} and the leaf-to-leaf distances"""
    edges = {}

    def walk(node):
        sub, ln = node
        leaves = [sub] if isinstance(sub, int) else [x for c in sub for x in walk(c)]
        edges[frozenset(leaves)] = ln
        return leaves

    all_leaves = []
    for c in KNOWN:
        all_leaves += walk(c)
    n = len(all_leaves)
    dist = np.zeros((n, n), dtype=np.int64)
    for s, ln in edges.items():  # an edge lies on the path between x and y when exactly one of them is below it
        m = np.array([x in s for x in range(n)])
        dist += ln * (m[:, None] != m[None, :])
    full = frozenset(range(n))
    return {(s if 11 not in s else full - s): ln for s, ln in edges.items()}, dist


def test_additive_matrix_gives_back_its_tree(ora):
    from pangene_amd import capi
    want, dist = _known_edges()
    assert len(want) == 2 * 12 - 3
    rng = np.random.default_rng(5)
    order = rng.permutation(12)  # the leaves in another order than the tree lists them
    q = (dist[np.ix_(order, order)] * UNIT).astype(np.int32)
    rec = capi.pan_join(ora, q, "nj")
    assert np.array_equal(rec, tr.joins(q, "nj"))
    below = {x: frozenset([int(order[x])]) for x in range(12)}
    got = {}
    full = frozenset(range(12))

    def put(s, ln):
        assert ln.denominator == 1 and int(ln) % UNIT == 0
        got[s if 11 not in s else full - s] = int(ln) // UNIT

    for i, j, dij, Ri, Rj, r in (tuple(int(v) for v in row) for row in rec[:-1]):
        li = (dij + Fraction(Ri - Rj, r - 2)) / 2
        put(below[i], li)
        put(below[j], dij - li)
        below[i] = below[i] | below[j]
    x, y, z, dxy, dxz, dyz = (int(v) for v in rec[-1])
    put(below[x], Fraction(dxy + dxz - dyz, 2))
    put(below[y], Fraction(dxy + dyz - dxz, 2))
    put(below[z], Fraction(dxz + dyz - dxy, 2))
    assert got == want


HAND = "S\tg1\t*\tLN:i:1\nS\tg2\t*\tLN:i:1\nS\tg3\t*\tLN:i:1\nS\tg4\t*\tLN:i:1\n"


def test_one_and_two_assemblies(built, tmp_path):
    g = tmp_path / "one.gfa"
    g.write_text(HAND + "W\ts1\t0\tc1\t0\t3\t>g1>g2>g3\n")
    for method in tr.METHODS:
        rc, out, _ = run_cli(["tree", "-a", method, str(g)])
        assert rc == 0 and out == b"(s1#0);\n"
    g = tmp_path / "two.gfa"
    g.write_text(HAND + "W\ts1\t0\tc1\t0\t3\t>g1>g2>g3\nW\ts2\t1\tc1\t0\t3\t>g1>g2\n")
    for method in tr.METHODS:
        rc, out, _ = run_cli(["tree", "-a", method, str(g)])
        assert rc == 0 and out == b"(s1#0:0.166667,s2#1:0.166667);\n"  # jaccard 1/3 as 349525 / 2^20, halved
        rc, out, _ = run_cli(["tree", "-m", "diff", "-a", method, str(g)])
        assert rc == 0 and out == b"(s1#0:0.500000,s2#1:0.500000);\n"
    g = tmp_path / "none.gfa"
    g.write_text(HAND)
    rc, out, _ = run_cli(["tree", str(g)])
    assert rc == 0 and out == b";\n"


def test_name_quoting(built, tmp_path):
    g = tmp_path / "q.gfa"
    g.write_text(HAND + "W\ta b\t0\tc\t0\t3\t>g1>g2>g3\nW\tit's\t0\tc\t0\t3\t>g1>g2\nW\tx(1)\t0\tc\t0\t3\t>g1>g4\nW\tplain\t0\tc\t0\t3\t>g2>g3>g4\n"
                 "W\tu,v;w:[z]\t0\tc\t0\t3\t>g4\n")
    names, S = _gene(str(g))
    assert names == ["a b#0", "it's#0", "x(1)#0", "plain#0", "u,v;w:[z]#0"]
    for method in tr.METHODS:
        rc, out, _ = run_cli(["tree", "-a", method, str(g)])
        assert rc == 0 and out == tr.text(names, S, "jaccard", method)
        for leaf in (b"'a b#0':", b"'it''s#0':", b"'x(1)#0':", b"'u,v;w:[z]#0':", b"plain#0:"):
            assert leaf in out
        assert b"'plain#0'" not in out and out.endswith(b";\n") and out.count(b"\n") == 1


def test_hand_worked_joins(ora):
    """Four leaves, two cherries: d(0, 1) = d(2, 3) = 2, everything else 6.  Every Q of a cherry is 2 * 2 - 14 - 14 = -24, a non-cherry gives
    2 * 6 - 28 = -16: the two cherries tie and slots (0, 1) win."""
    from pangene_amd import capi
    q = np.array([[0, 2, 6, 6], [2, 0, 6, 6], [6, 6, 0, 2], [6, 6, 2, 0]], dtype=np.int32)
    assert capi.pan_join(ora, q, "nj").tolist() == [[0, 1, 2, 14, 14, 4], [0, 2, 3, 5, 5, 2]]
    assert capi.pan_join(ora, q, "upgma").tolist() == [[0, 1, 2, 1, 1, 4], [2, 3, 2, 1, 1, 3], [0, 2, 6, 2, 2, 2]]
    odd = np.array([[0, 3, 4], [3, 0, 2], [4, 2, 0]], dtype=np.int32)  # upgma floors: (1 * 3 + 1 * 4) // 2 = 3
    assert capi.pan_join(ora, odd, "upgma").tolist() == [[1, 2, 2, 1, 1, 3], [0, 1, 3, 1, 2, 2]]
    neg = np.array([[0, 1, 1], [1, 0, 4], [1, 4, 0]], dtype=np.int32)
    assert capi.pan_join(ora, neg, "nj").tolist() == [[0, 1, 2, 1, 1, 4]]


def test_argument_and_range_errors(ora):
    from pangene_amd import capi
    q = np.zeros((4, 4), dtype=np.int32)
    q[0, 1] = q[1, 0] = 1 << 29
    for method in tr.METHODS:
        with pytest.raises(RuntimeError, match="status -2"):  # PGA_ERR_RANGE
            capi.pan_join(ora, q, method)
    q[0, 1] = q[1, 0] = (1 << 29) - 1
    assert capi.pan_join(ora, q, "upgma").shape == (3, 6)
    q[1, 0] = 5
    with pytest.raises(RuntimeError, match="status -3"):  # not symmetric: PGA_ERR_ARG
        capi.pan_join(ora, q, "nj")
    with pytest.raises(RuntimeError, match="status -3"):
        capi.pan_join(ora, np.zeros((2, 2), dtype=np.int32), "nj")
    with pytest.raises(ValueError):
        capi.pan_tree(ora, np.ones((5, 4), dtype=bool), "shared")


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", ["C4", "bact20"])
def test_in_memory_route_equals_file_route(built, tmp_path, name):
    files = _paf_dir(name)
    rc, gfa, _ = run_cli(files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    for kind, metric, method in (("gene", "jaccard", "nj"), ("adj", "diff", "upgma")):
        rc1, a, _ = run_cli(["--tree=" + kind, "--tree-metric=" + metric, "--tree-method=" + method] + files)
        rc2, b, _ = run_cli(["tree", "-t", kind, "-m", metric, "-a", method, str(tmp_path / "g.gfa")])
        assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(b"(") and a.endswith(b");\n"), kind
    rc, d, _ = run_cli(["--tree"] + files)
    assert rc == 0 and d == run_cli(["tree", str(tmp_path / "g.gfa")])[1]


def test_python_run_equals_command_line(ora):
    from pangene_amd import capi
    files = _paf_dir("C4")
    args = ["--tree=adj", "--tree-method=upgma"]
    assert capi.run(ora, files, args) == run_cli(args + files)[1]


def test_refusals(built, tmp_path):
    files = _paf_dir("C4")
    rc, out, err = run_cli(["--gpus", "2", "--tree"] + files)
    assert rc == 1 and out == b"" and b"--tree" in err
    for extra in (["--matrix"], ["--call"], ["--curves"], ["--dist"], ["--assoc"]):
        rc, out, err = run_cli(["--tree"] + extra + files)
        assert rc == 1 and out == b"" and b"--tree" in err
    for bad in (["--tree=genes"], ["--tree", "--tree-metric=shared"], ["--tree", "--tree-method=ml"]):
        rc, out, err = run_cli(bad + files)
        assert rc == 1 and out == b"" and err != b""
    g = os.path.join(GOLD, "C4.gfa.gz")
    for bad in (["-t", "x"], ["-m", "shared"], ["-a", "ml"]):
        rc, out, err = run_cli(["tree"] + bad + [g])
        assert rc == 1 and out == b"" and err != b""
    rc, out, _ = run_cli(["tree", str(tmp_path / "none.gfa")])
    assert rc == 1 and out == b""


def test_usage(built):
    rc, out, _ = run_cli(["tree"])
    assert rc == 0 and out.startswith(b"Usage: pangene tree [options] <in.gfa>\n") and b"negative branch lengths" in out
    rc, _, err = run_cli([])
    assert b"pangene tree [-t gene|adj]" in err and b"--tree[=STR]" in err


@pytest.mark.parametrize("n", tr.SIGNED_SIZES)
def test_signed_matrices(ora, n):
    """the matrices of the `signed` GPU cases: entries of either sign up to 2^29 - 1 in size; floor(x / 2) and the floored division of
    UPGMA on negative sums, in the checker build as in the restatement"""
    from pangene_amd import capi
    q = tr.signed_matrix(n, n)
    assert np.array_equal(q, q.T) and not np.diag(q).any() and int(np.abs(q).max()) <= tr.IN_MAX
    if n >= 63:
        assert int(q.min()) < -(1 << 28) and int(q.max()) > 1 << 28 and int(np.abs(q).max()) > tr.IN_MAX - (1 << 20)
    for method in tr.METHODS:
        stats = {}
        want = tr.joins(q, method, stats)
        if n >= 63:  # joined distances below zero, and under nj a run that leaves the input's range
            assert int(want[:n - 3, 2].min()) < 0 and (method == "upgma" or stats["peak"] > 1 << 29)
        assert np.array_equal(capi.pan_join(ora, q, method), want), method


def test_peak_below_the_range_limit(ora):
    """the hill-climb of tree_ref.peak_search: a neighbour-joining run over 5 slots that peaks within 2^20 of the range limit 2^30 and
    stays inside; the checker build gives the restatement's records"""
    from pangene_amd import capi
    q, peak, leaving = tr.peak_search()
    stats = {}
    want = tr.joins(q, "nj", stats)
    assert (1 << 30) - (1 << 20) <= peak == stats["peak"] < 1 << 30 and int(np.abs(q).max()) <= tr.IN_MAX
    assert np.array_equal(capi.pan_join(ora, q, "nj"), want)
    assert np.array_equal(capi.pan_join(ora, q, "upgma"), tr.joins(q, "upgma"))
    if leaving is not None:
        with pytest.raises(RuntimeError, match="status -2"):
            capi.pan_join(ora, leaving, "nj")
