"""Gene associations (`pangene assoc`, `pangene --assoc`, pg_pan_assoc) through the checker build: the host driver linked against the
oracle backend, whose table has no pan_assoc entry, so the selection runs as the plain host loops of assoc.cpp.  Everything is
compared with the numpy restatement of tests/support/assoc_ref.py, which decides the selection in exact integers."""
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
import assoc_ref as ar  # noqa: E402

GFAS = sorted(os.path.join(GOLD, f) for f in os.listdir(GOLD) if f.endswith(".gfa.gz")) + \
    sorted(os.path.join(GOLD, "bubble", f) for f in os.listdir(os.path.join(GOLD, "bubble")) if f.endswith(".gfa"))
HEADER = b"GeneA\tGeneB\tnA\tnB\tnAB\tphi\n"


def run_cli(args, exe=CLI):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    return oracle_host.load()


two_rows = ar.two_rows


def test_hand_worked_boundary(ora):
    """A = 8, a = b = 4: s = 3 gives D = 8, V_g V_h = 256, phi = 0.5 exactly; s = 1 gives phi = -0.5"""
    from pangene_amd import capi
    P = two_rows(8, 4, 4, 3)
    pairs, phi = capi.pan_assoc(ora, P, min_phi=0.5)
    assert pairs.dtype == np.int32 and pairs.tolist() == [[0, 1, 3]] and phi.dtype == np.float64 and phi.tolist() == [0.5]
    assert capi.pan_assoc(ora, P, min_phi=0.501)[0].shape == (0, 3)
    assert capi.pan_assoc(ora, P, min_phi=0.5, sign="pos")[0].tolist() == [[0, 1, 3]]
    assert capi.pan_assoc(ora, P, min_phi=0.5, sign="neg")[0].shape == (0, 3)
    N = two_rows(8, 4, 4, 1)
    pairs, phi = capi.pan_assoc(ora, N, min_phi=0.5)
    assert pairs.tolist() == [[0, 1, 1]] and phi.tolist() == [-0.5]
    assert capi.pan_assoc(ora, N, min_phi=0.5, sign="neg")[0].tolist() == [[0, 1, 1]]
    assert capi.pan_assoc(ora, N, min_phi=0.5, sign="pos")[0].shape == (0, 3)
    assert capi.pan_assoc(ora, N, min_phi=0.501, sign="neg")[0].shape == (0, 3)
    # D = 0 counts as positive: a = b = 4, s = 2
    Z = two_rows(8, 4, 4, 2)
    assert capi.pan_assoc(ora, Z, min_phi=0.0, sign="pos")[0].tolist() == [[0, 1, 2]]
    assert capi.pan_assoc(ora, Z, min_phi=0.0, sign="neg")[0].shape == (0, 3)


exact_threshold_cases = ar.exact_threshold_cases


def test_exact_threshold_cases(ora):
    """the equality branch of 10^6 D^2 >= p^2 V_g V_h at thresholds that are not round: selected at p, not at p + 1"""
    from pangene_amd import capi
    cases = exact_threshold_cases()
    assert len(cases) >= 5
    assert len({c[4] for c in cases}) >= 3
    for A, a, b, s, p in cases[:: max(1, len(cases) // 60)]:
        P = two_rows(A, a, b, s)
        for r, want in ((p / 1000.0, 1), ((p + 1) / 1000.0, 0), ((p - 1) / 1000.0, 1)):
            assert ar.permille(r) == round(r * 1000)
            got = capi.pan_assoc(ora, P, min_phi=r, min_count=2)[0]
            ref = ar.select(P, r, 2)[0]
            assert len(got) == want and np.array_equal(got, ref), (A, a, b, s, p, r)


SHAPES = [(g, a) for g in (0, 1, 2, 127, 128, 129, 257, 1025) for a in (0, 1, 2, 31, 32, 33, 65, 4097)]
SETTINGS = [(0.8, 2, "both"), (0.5, 1, "pos"), (0.333, 3, "neg"), (0.0, 2, "both"), (1.0, 1, "both")]


@pytest.mark.parametrize("G,A", SHAPES, ids=["G%d-A%d" % s for s in SHAPES])
def test_random_shapes(ora, G, A):
    from pangene_amd import capi
    P = ar.planted(G, A, G * 10007 + A)
    n_sel = 0
    for r, c, sign in SETTINGS:
        if r == 0.0 and G > 300:
            continue  # every eligible pair: the list, not the arithmetic, would be what is tested
        pairs, phi = capi.pan_assoc(ora, P, r, c, sign)
        want, cnt = ar.select(P, r, c, sign)
        assert pairs.shape == want.shape and np.array_equal(pairs, want), (r, c, sign)
        assert np.array_equal(phi, ar.phi(want, cnt, A))
        n_sel += len(want)
    if G >= 127 and A >= 31:
        assert n_sel > 0  # the planted modules


@pytest.mark.parametrize("gfa", GFAS, ids=[os.path.relpath(g, GOLD) for g in GFAS])
def test_fixture_files(built, gfa):
    genes, P = ar.read_gfa(gfa)
    for args, kw in (([], {}), (["-r", "0.5", "-c", "1"], dict(min_phi=0.5, min_count=1)), (["-r", "0.9", "-s", "neg"], dict(min_phi=0.9, sign="neg")),
                     (["-r", "0.95", "-s", "pos", "-c", "3"], dict(min_phi=0.95, sign="pos", min_count=3))):
        want = ar.text(genes, P, **kw)
        if want.count(b"\n") > 200000:
            continue
        rc, out, err = run_cli(["assoc"] + args + [gfa])
        assert rc == 0, err
        assert out == want, " ".join(args)


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", ["C4", "bact20", "fuzz0"])
def test_in_memory_route_equals_file_route(built, tmp_path, name):
    """`pangene --assoc *.paf` (pg_write_assoc on the graph in memory) prints what `pangene *.paf > g.gfa; pangene assoc g.gfa` prints"""
    files = _paf_dir(name)
    rc, gfa, _ = run_cli(files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    rc1, a, _ = run_cli(["--assoc"] + files)
    rc2, b, _ = run_cli(["assoc", str(tmp_path / "g.gfa")])
    assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(HEADER)
    rc1, a, _ = run_cli(["--assoc=0.4", "--assoc-min-count=1", "--assoc-sign=neg"] + files)
    rc2, b, _ = run_cli(["assoc", "-r", "0.4", "-c", "1", "-s", "neg", str(tmp_path / "g.gfa")])
    assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(HEADER)


def test_python_run_equals_command_line(ora):
    from pangene_amd import capi
    files = _paf_dir("C4")
    assert capi.run(ora, files, ["--assoc"]) == run_cli(["--assoc"] + files)[1]
    assert capi.run(ora, files, ["--assoc=0.3", "--assoc-min-count=1"]) == run_cli(["--assoc=0.3", "--assoc-min-count=1"] + files)[1]


def test_refusals(built, ora, tmp_path):
    from pangene_amd import capi
    files = _paf_dir("C4")
    rc, out, err = run_cli(["--gpus", "2", "--assoc"] + files)
    assert rc == 1 and out == b"" and b"--assoc" in err
    for extra in (["--matrix"], ["--call"], ["--matrix=count"], ["--curves"], ["--dist"]):
        rc, out, err = run_cli(["--assoc"] + extra + files)
        assert rc == 1 and out == b"" and b"--assoc" in err
    for bad in (["--assoc=1.5"], ["--assoc=-0.1"], ["--assoc=x"], ["--assoc", "--assoc-min-count=0"], ["--assoc", "--assoc-sign=up"]):
        rc, out, err = run_cli(bad + files)
        assert rc == 1 and out == b""
    g = os.path.join(GOLD, "C4.gfa.gz")
    for bad in (["-r", "1.01"], ["-r", "-0.5"], ["-r", "abc"], ["-c", "0"], ["-s", "up"], ["-x", "-1"]):
        rc, out, _ = run_cli(["assoc"] + bad + [g])
        assert rc == 1 and out == b""
    # more than -x pairs: 4 identical genes make 6 perfect pairs
    f = tmp_path / "m.gfa"
    f.write_text("".join("S\tg%d\t*\tLN:i:1\n" % i for i in range(4)) +
                 "".join("W\ts%d\t0\tc\t0\t1\t%s\n" % (a, ">g0>g1>g2>g3" if a < 3 else ">x") for a in range(6)))
    rc, out, err = run_cli(["assoc", "-x", "5", str(f)])
    assert rc == 1 and out == b"" and b"6 gene pairs" in err and b"-r" in err and b"-c" in err
    rc, out, err = run_cli(["assoc", "-x", "6", str(f)])
    assert rc == 0 and out.count(b"\n") == 7
    P = np.zeros((4, 6), dtype=bool)
    P[:, :3] = True
    with pytest.raises(RuntimeError):
        capi.pan_assoc(ora, P, max_pair=5)
    assert len(capi.pan_assoc(ora, P, max_pair=6)[0]) == 6
    for kw in (dict(min_phi=1.5), dict(min_phi=-0.1), dict(min_count=0), dict(sign="up")):
        with pytest.raises(ValueError):
            capi.pan_assoc(ora, P, **kw)


def test_usage_and_missing_file(built, tmp_path):
    rc, out, _ = run_cli(["assoc"])
    assert rc == 0 and out.startswith(b"Usage: pangene assoc [options] <in.gfa>\n")
    rc, out, _ = run_cli(["assoc", str(tmp_path / "none.gfa")])
    assert rc == 1 and out == b""
    rc, _, err = run_cli([])
    assert b"pangene assoc [-r FLOAT] [-c INT] [-s pos|neg|both] [-x INT] <in.gfa>" in err and b"--assoc[=FLOAT]" in err
    assert b"--assoc-min-count=INT" in err and b"--assoc-sign=STR" in err


def test_no_assemblies(built, tmp_path):
    g = tmp_path / "s.gfa"
    g.write_text("S\ta\t*\tLN:i:1\nS\tb\t*\tLN:i:1\n")
    rc, out, _ = run_cli(["assoc", str(g)])
    assert rc == 0 and out == HEADER


def test_second_fetch_of_the_python_wrapper(ora):
    """more pairs than the wrapper's first buffer holds: 400 identical genes"""
    from pangene_amd import capi
    P = np.zeros((400, 10), dtype=bool)
    P[:, :4] = True
    pairs, phi = capi.pan_assoc(ora, P)
    assert len(pairs) == 400 * 399 // 2 and np.array_equal(pairs, ar.select(P)[0]) and bool((phi == 1.0).all())


def test_torch_input(ora):
    torch = pytest.importorskip("torch")
    from pangene_amd import capi
    P = ar.planted(300, 40, 4)
    a = capi.pan_assoc(ora, torch.from_numpy(P), 0.6)
    b = capi.pan_assoc(ora, P, 0.6)
    assert len(b[0]) > 0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = capi.pan_assoc(ora, torch.from_numpy(P).to(torch.uint8), 0.6, sign="neg")
    assert np.array_equal(c[0], ar.select(P, 0.6, 2, "neg")[0])


def test_tie_tiles(ora):
    """the matrices of the `threshold` GPU cases (assoc_ref.tie_tiles): every cross pair exactly on the threshold -- selected at p and at
    p - 1 with its s, not at p + 1, under the signs that admit its D; the identical rows always, unless the sign is neg"""
    from pangene_amd import capi
    tiles = ar.tie_tiles()
    assert len(tiles) == 8 and {t[2] for t in tiles} == set(ar.TIE_P) and {t[3] for t in tiles} == {1, -1}
    for label, P, p, side, cross, same in tiles:
        G, A = P.shape
        cnt = P.sum(axis=1, dtype=np.int64)
        s = int((P[0] & P[G // 2 if G == 256 else 1]).sum())
        assert A == 4000 and (cnt == 2000).all() and s == 1000 + side * p
        assert 10 ** 6 * (s * A - 2000 * 2000) ** 2 == p * p * (2000 * 2000) ** 2
        for at in (p, p + 1, p - 1):
            assert ar.permille(at / 1000.0) == at
            for sign in ar.SIGNS:
                want, _ = ar.select(P, at / 1000.0, 2, sign)
                assert len(want) == ar.tie_count(p, side, cross, same, at, sign), (label, at, sign)
                got, phi = capi.pan_assoc(ora, P, at / 1000.0, 2, sign)
                assert got.shape == want.shape and np.array_equal(got, want) and np.array_equal(phi, ar.phi(want, cnt, A)), (label, at, sign)
        if side * p > 0:
            assert set(ar.select(P, p / 1000.0, 2, "pos")[0][:, 2].tolist()) == {2000, s}


@pytest.mark.parametrize("p,least", [(337, (2, 2, 2, 1)), (801, (0, 2, 2, 0))])
def test_band_cases(ora, p, least):
    """the cases of the `band337` / `band801` GPU groups (assoc_ref.band_cases) at A = 16 777 215: the search finds pairs on the threshold,
    just above and just below it and with D < 0 (p = 337 alone has at least 2, 2, 2 and 1 of them; no pair sits exactly on 0.801), all
    strictly inside the device's guard band; the checker build decides every one of them as the exact integers do, at p and at p + 1"""
    from fractions import Fraction
    import assoc_direct
    cases = ar.band_cases(p)
    A = ar.MAX_ASM
    for _, a, s, cmp in cases:
        D, V = s * A - a * a, a * (A - a)
        assert 0 <= s <= a and 2 * a - s <= A and abs(Fraction(10 ** 6 * D * D, p * p * V * V) - 1) < Fraction(1, 2 ** 41)
        assert cmp == (10 ** 6 * D * D > p * p * V * V) - (10 ** 6 * D * D < p * p * V * V)
    found = (sum(c[3] == 0 for c in cases), sum(c[3] > 0 for c in cases), sum(c[3] < 0 for c in cases), sum(c[2] * A < c[1] * c[1] for c in cases))
    assert all(f >= l for f, l in zip(found, least)), found
    for _, a, s, cmp in cases:
        assoc_direct.check_band([ora], p, a, s, cmp)


def test_band_expected_is_what_select_gives():
    """the records worked out from (a, s) alone against the restatement itself at 16 777 215 columns, for one pair below the threshold"""
    a, s = 8234022, 7399639
    for at in (800, 801):
        want, cnt = ar.select(ar.band_matrix(a, s) != 0, at / 1000.0, 2)
        pairs, phi = ar.band_expected(a, s, at)
        assert len(want) == (6 if at == 800 else 2) and np.array_equal(want, pairs) and np.array_equal(ar.phi(want, cnt, ar.MAX_ASM), phi)
