"""Co-evolution on the tree (`pangene coevo`, `pangene --coevo`, pg_pan_coevo) through the checker build: the host driver linked against
the oracle backend, whose table has no pan_coevo entry, so the events, the pair counts and the selection come from the plain loops of
pan_coevo.hpp over the tree records.  Everything is compared with the numpy restatement of tests/support/coevo_ref.py -- names and integer
columns byte for byte, r within 1e-4 absolute and p_hyper within 1e-3 relative, the rule tests/test_trait.py uses for printed floats -- and
that with a brute force that recounts pair by pair."""
import ctypes as C
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
import coevo_ref as cr  # noqa: E402
import pairs_ref as pr  # noqa: E402

NAMES = ["C4", "bact20", "human8", "dense"]


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


def random_records(rng, A):
    """upgma-shaped records of a random rooted tree: any two live slots are joined"""
    live, rec = list(range(A)), []
    while len(live) > 1:
        i, j = (int(v) for v in rng.choice(live, size=2, replace=False))
        rec.append((i, j, 0, 0, 0, len(live)))
        live.remove(j)
    return np.array(rec, dtype=np.int64).reshape(-1, 6)


_want = {}


def want_rows(path, key, **kw):
    """the restatement's rows of a fixture and option set, computed once"""
    k = (key, tuple(sorted(kw.items())))
    if k not in _want:
        _want[k] = cr.table_rows(path, **kw)
    return _want[k]


@pytest.mark.parametrize("name", NAMES)
def test_file_route(built, name):
    """pg_coevo_file through the command line against the restatement for the five option sets"""
    for kw in cr.OPTION_SETS:
        sub, _ = cr.option_args(**kw)
        rc, out, err = run_cli(["coevo"] + sub + [gfa_of(name)])
        assert rc == 0, err
        cr.compare(out, want_rows(gfa_of(name), name, **kw))


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, tmp_path, name):
    """`pangene --coevo ... *.paf` prints what `pangene coevo` prints for the GFA of the same run, and what the restatement does"""
    files = pafs_of(name)
    rc, gfa, err = run_cli(files)
    assert rc == 0, err
    path = str(tmp_path / "g.gfa")
    with open(path, "wb") as f:
        f.write(gfa)
    for kw in cr.OPTION_SETS:
        sub, long = cr.option_args(**kw)
        rc1, a, err = run_cli(long + files)
        rc2, b, _ = run_cli(["coevo"] + sub + [path])
        assert rc1 == 0 and rc2 == 0, err
        assert a == b, kw
        cr.compare(a, cr.table_rows(path, **kw))
    rc, a, _ = run_cli(["--coevo"] + files)
    rc2, b, _ = run_cli(["coevo", path])
    assert rc == 0 and rc2 == 0 and a == b
    if name == "C4":  # and capi.run, the same route in-process
        import oracle_host
        from pangene_amd import capi
        lib = oracle_host.load()
        C.c_int.in_dll(lib, "pg_verbose").value = 0
        kw = cr.OPTION_SETS[4]
        assert capi.run(lib, files, cr.option_args(**kw)[1]) == run_cli(["coevo"] + cr.option_args(**kw)[0] + [path])[1]
        with pytest.raises(ValueError):
            capi.run(lib, files, ["--coevo-gain=2"])
        with pytest.raises(ValueError):
            capi.run(lib, files, ["--coevo", "--coevo-gain=0"])
        with pytest.raises(ValueError):
            capi.run(lib, files, ["--coevo", "--gainloss"])


def test_fixtures_are_not_vacuous(built):
    """the defaults (jaccard, g = l = 1, late) and -t adj on the fixtures: the counts of the restatement, which the command must print"""
    table = {("bact20", "gene"): (65, 69), ("bact20", "adj"): (1822, 1776), ("human8", "adj"): (4, 3), ("dense", "gene"): (962, 932), ("C4", "gene"): (0, 0)}
    neg = {"upgma": 7, "nj": 9}
    for (name, kind), counts in table.items():
        for method, n in zip(("upgma", "nj"), counts):
            kw = {"kind": kind, "method": method}
            rows = want_rows(gfa_of(name), name, **kw)
            assert len(rows) == n, (name, kind, method, len(rows))
            rc, out, err = run_cli(["coevo", "-t", kind, "-a", method, gfa_of(name)])
            assert rc == 0, err
            cr.compare(out, rows)
            assert (out.count(b"\n") > 1) == (n > 0)
            if (name, kind) == ("bact20", "gene"):
                assert sum(1 for r in rows if r[6] < r[7]) == neg[method] > 0
    for method in ("upgma", "nj"):
        kw = {"kind": "adj", "method": method, "min_events": 1, "min_r": 0.5}
        rc, out, _ = run_cli(["coevo"] + cr.option_args(**kw)[0] + [gfa_of("C4")])
        assert rc == 0 and out.count(b"\n") == 3
        cr.compare(out, want_rows(gfa_of("C4"), "C4", **kw))
    rc, out, _ = run_cli(["coevo", gfa_of("C4")])
    assert rc == 0 and out == cr.HEADER


def test_random_matrices_and_trees(ora):
    """capi.pan_coevo on random matrices over random trees: events and every pair record against the restatement, and for at most 8
    leaves every selected pair and a sample of all pairs against the brute force"""
    from pangene_amd import capi
    rng = np.random.default_rng(12)
    for A, M in ((2, 9), (3, 20), (5, 40), (8, 60), (13, 90), (33, 120), (70, 64)):
        P = rng.random((M, A)) < rng.random(M)[:, None]
        rec = random_records(rng, A)
        kids = pr.tree(rec, A, "upgma")
        for g, l, mode, r, c, sign in ((1, 1, "late", 0.8, 2, "both"), (2, 1, "early", 0.5, 1, "pos"), (1, 3, "late", 0.3, 2, "neg"), (1, 1, "early", 0.0, 1, "both")):
            e, pairs = capi.pan_coevo(ora, P, rec if A >= 3 else None, "upgma", g, l, mode, r, c, sign)
            we, wp = cr.select(P, kids, g, l, mode, r, c, sign)
            assert np.array_equal(e, we) and np.array_equal(pairs, wp), (A, M, g, l, mode, r, c, sign)
            if A <= 8:
                for i, j, same, opp in pairs[:40].tolist():
                    assert cr.brute(P, kids, i, j, g, l, mode) == (same, opp)
        if A <= 8:  # r = 0, c = 1, both: every pair of items with an event is listed, so the last call covers the whole triangle
            assert len(pairs) == (e >= 1).sum() * ((e >= 1).sum() - 1) // 2
    for method in ("upgma", "nj"):  # real trees
        P = rng.random((150, 21)) < 0.4
        rec, _ = capi.pan_tree(ora, P, "jaccard", method)
        e, pairs = capi.pan_coevo(ora, P, rec, method, min_r=0.4)
        we, wp = cr.select(P, pr.tree(rec, 21, method), min_r=0.4)
        assert np.array_equal(e, we) and np.array_equal(pairs, wp) and len(wp) > 0
        assert np.array_equal(e, capi.pan_gainloss(ora, P, rec, method)["gains"] + capi.pan_gainloss(ora, P, rec, method)["losses"])


def boundary_matrix():
    """A balanced tree of 16 leaves (cherries (0, 1), (2, 3), ...) whose right half carries nothing.  An item present in one leaf of each of
    the four left cherries costs 4 either way in the left half, the root is absent and under `late` nothing switches above the leaves: four
    gains on leaf branches.  Its complement has four losses there.  Item 0 gains at 0, 2, 4, 6; item 1 at 0, 2, 5, 7 (same = 2, d = 2);
    item 2 is present everywhere but 0, 2, 5, 7, where it is lost (with item 0: opp = 2, d = -2)."""
    A = 16
    P = np.zeros((3, A), dtype=bool)
    P[0, [0, 2, 4, 6]] = True
    P[1, [0, 2, 5, 7]] = True
    P[2] = True
    P[2, [0, 2, 5, 7]] = False
    return P, pr.balanced_records(A)


def test_selection_boundary(ora):
    """e_i = e_j = 4 and d = 2: 10^6 * 4 = p^2 * 16 at p = 500, so the pair is selected at p = 500 and not at 501 (r = 0.5004 still reads
    as 500, 0.5006 as 501); d = -2 the same under neg and both and never under pos"""
    from pangene_amd import capi
    P, rec = boundary_matrix()
    kids = pr.tree(rec, 16, "upgma")
    X, res = cr.events(P, kids)
    assert res["gains"].tolist() == [4, 4, 0] and res["losses"].tolist() == [0, 0, 4]
    assert cr.brute(P, kids, 0, 1) == (2, 0) and cr.brute(P, kids, 0, 2) == (0, 2)
    for r, sign, want_pos, want_neg in ((0.5, "both", True, True), (0.501, "both", False, False), (0.5, "pos", True, False), (0.5, "neg", False, True),
                                        (0.501, "pos", False, False), (0.501, "neg", False, False), (0.5004, "both", True, True), (0.5006, "both", False, False)):
        e, pairs = capi.pan_coevo(ora, P, rec, "upgma", min_r=r, sign=sign)
        got = {(i, j): (s, o) for i, j, s, o in pairs.tolist()}
        assert ((0, 1) in got) == want_pos and ((0, 2) in got) == want_neg, (r, sign, got)
        assert np.array_equal(pairs, cr.select(P, kids, min_r=r, sign=sign)[1])
        if want_pos:
            assert got[(0, 1)] == (2, 0)
        if want_neg:
            assert got[(0, 2)] == (0, 2)


def test_constant_items_are_never_listed(ora):
    from pangene_amd import capi
    rng = np.random.default_rng(9)
    A = 12
    P = rng.random((30, A)) < 0.5
    P[3], P[17] = True, False
    rec = random_records(rng, A)
    for c in (1, 2):
        e, pairs = capi.pan_coevo(ora, P, rec, "upgma", min_r=0.0, min_events=c)
        assert e[3] == 0 and e[17] == 0 and len(pairs) > 0
        assert not np.isin(pairs[:, :2], (3, 17)).any()
    e, pairs = capi.pan_coevo(ora, P[[3, 17]], rec, "upgma", min_r=0.0, min_events=1)
    assert e.tolist() == [0, 0] and pairs.shape == (0, 4)


def test_small_shapes(ora):
    """one assembly (no branch), two (two branches, no records), and no items"""
    from pangene_amd import capi
    e, pairs = capi.pan_coevo(ora, np.array([[1], [0]], dtype=bool), None, "upgma", min_events=1, min_r=0.0)
    assert e.tolist() == [0, 0] and pairs.shape == (0, 4)
    P = np.array([[0, 0], [1, 0], [0, 1], [1, 1], [1, 0]], dtype=bool)
    e, pairs = capi.pan_coevo(ora, P, None, "nj", min_events=1, min_r=0.0)
    we, wp = cr.select(P, [(0, 1)], min_events=1, min_r=0.0)
    assert np.array_equal(e, we) and np.array_equal(pairs, wp) and [1, 4, 1, 0] in pairs.tolist()
    e, pairs = capi.pan_coevo(ora, np.zeros((0, 5), dtype=bool), random_records(np.random.default_rng(1), 5), "upgma")
    assert e.shape == (0,) and pairs.shape == (0, 4)
    e, pairs = capi.pan_coevo(ora, np.zeros((3, 0), dtype=bool), None, "upgma")
    assert e.tolist() == [0, 0, 0] and pairs.shape == (0, 4)


def test_empty_inputs_print_the_header_only(built, tmp_path):
    empty = tmp_path / "empty.gfa"
    empty.write_text("")
    rc, got, err = run_cli(["coevo", str(empty)])
    assert rc == 0 and got == cr.HEADER, err
    one = tmp_path / "one.gfa"  # one assembly: no branch
    one.write_text("S\tg1\t*\nS\tg2\t*\nL\tg1\t+\tg2\t+\t0M\nW\ts1\t0\tc1\t*\t*\t>g1>g2\n")
    rc, got, _ = run_cli(["coevo", "-c", "1", "-r", "0", str(one)])
    assert rc == 0 and got == cr.HEADER


def test_too_many_pairs(built, ora):
    """-x exceeded: the error assoc gives and no table"""
    from pangene_amd import capi
    gfa = gfa_of("bact20")
    rc, out, err = run_cli(["coevo", "-x", "64", gfa])
    assert rc == 1 and out == b"" and b"65 item pairs passed, more than the 64 allowed (-x)" in err
    rc, out, err = run_cli(["coevo", "-x", "65", gfa])
    assert rc == 0 and out.count(b"\n") == 66
    rc, out, err = run_cli(["--coevo", "--coevo-max=10"] + pafs_of("bact20"))
    assert rc != 0 and out == b"" and b"more than the 10 allowed" in err
    rng = np.random.default_rng(2)
    P = rng.random((40, 9)) < 0.5
    with pytest.raises(RuntimeError, match="status -2"):
        capi.pan_coevo(ora, P, random_records(rng, 9), "upgma", min_r=0.0, min_events=1, max_pair=5)


def test_refusals_and_usage(built, ora, tmp_path):
    from pangene_amd import capi
    gfa = gfa_of("C4")
    for bad in (["-g", "0"], ["-g", "256"], ["-l", "0"], ["-l", "x"], ["-e", "middle"], ["-a", "ml"], ["-m", "shared"], ["-t", "exon"], ["-c", "0"], ["-c", "x"],
                ["-r", "1.5"], ["-r", "-0.1"], ["-s", "up"], ["-x", "-1"]):
        rc, out, err = run_cli(["coevo"] + bad + [gfa])
        assert rc == 1 and out == b"" and bad[0].encode() in err, bad
    files = pafs_of("C4")
    for bad in ("--coevo=2", "--coevo-gain=0", "--coevo-loss=256", "--coevo-resolve=x", "--coevo-method=ml", "--coevo-metric=shared", "--coevo-type=exon",
                "--coevo-min=0", "--coevo-sign=up", "--coevo-max=-1"):
        rc, out, err = run_cli(["--coevo", bad] + files)
        assert rc == 1 and out == b"" and bad.split("=")[0].encode() in err, bad
    rc, out, err = run_cli(["--coevo-gain=2"] + files)
    assert rc == 1 and out == b"" and b"need --coevo" in err
    rc, out, err = run_cli(["--coevo", "--gainloss"] + files)
    assert rc == 1 and out == b"" and b"cannot be combined" in err
    rc, out, err = run_cli(["--gpus", "2", "--coevo"] + files)
    assert rc == 1 and out == b"" and b"--coevo" in err
    rc, out, err = run_cli(["coevo", str(tmp_path / "missing.gfa")])
    assert rc == 1 and out == b""
    rc, out, err = run_cli(["coevo"])
    assert rc == 0 and out.startswith(b"Usage: pangene coevo [options] <in.gfa>\n")
    assert all(w in out for w in (b"-g INT", b"-l INT", b"-e STR", b"-r FLOAT", b"-c INT", b"-s STR", b"-x INT", b"((x, y), z)", b"[upgma]", b"[0.8]", b"[16777216]",
                                  b"every pair of strain-specific genes of one assembly scores 1"))
    rc, out, err = run_cli([])
    assert b"--coevo[=FLOAT]" in err and b"pangene coevo [-t gene|adj]" in err
    # pg_pan_coevo itself: NULLs, option values out of range and bad records are PGA_ERR_ARG (-3), sizes out of range PGA_ERR_RANGE (-2)
    P = np.ascontiguousarray(np.random.default_rng(2).random((6, 4)) < 0.5, dtype=np.uint8)
    rec = np.ascontiguousarray(random_records(np.random.default_rng(2), 4))
    ev, pair = np.zeros(6, dtype=np.int32), np.zeros((16, 4), dtype=np.int32)
    pp, rp = P.ctypes.data_as(C.POINTER(C.c_uint8)), rec.ctypes.data_as(C.POINTER(C.c_int64))
    ep, qp = ev.ctypes.data_as(C.POINTER(C.c_int32)), pair.ctypes.data_as(C.POINTER(C.c_int32))

    def call(p=pp, r=rp, method=1, o=None, e=ep, q=qp, cap=16, M=6, A=4, **kw):
        opt = capi.coevo_opt(ora)
        for k, v in kw.items():
            setattr(opt, k, v)
        return ora.pg_pan_coevo(p, M, A, r, method, None if o == "null" else C.byref(opt), e, q, cap)

    assert call() >= 0 and call(e=None) >= 0 and call(q=None, cap=0) >= 0
    assert call(gain=0) == -3 and call(gain=256) == -3 and call(loss=0) == -3 and call(loss=256) == -3 and call(mode=2) == -3 and call(mode=-1) == -3
    assert call(min_events=0) == -3 and call(min_r=1.5) == -3 and call(min_r=-0.5) == -3 and call(sign=3) == -3 and call(sign=-1) == -3 and call(max_pair=-1) == -3
    assert call(o="null") == -3 and call(p=None) == -3 and call(r=None) == -3 and call(q=None) == -3 and call(method=2) == -3 and call(cap=-1) == -3
    assert call(M=-1) == -3 and call(A=-1) == -3
    for bad in ([(0, 0)], [(0, 4)], [(0, 1), (1, 2)], [(-1, 2)]):  # a slot twice in a join, out of range, retired, negative
        r2 = rec.copy()
        for t, (i, j) in enumerate(bad):
            r2[t, 0], r2[t, 1] = i, j
        assert call(r=r2.ctypes.data_as(C.POINTER(C.c_int64))) == -3, bad
    assert call(A=65536) == -2 and call(M=16777216) == -2
    assert C.sizeof(capi.pg_coevo_opt_t) == 48
    for kw in ({"gain": 0}, {"min_r": 1.1}, {"min_events": 0}, {"sign": "up"}, {"mode": "x"}, {"max_pair": -1}, {"type": "exon"}):
        with pytest.raises(ValueError):
            capi.coevo_opt(ora, **kw)
    with pytest.raises(ValueError):
        capi.pan_coevo(ora, P, rec[:2], "upgma")
