"""PERMANOVA (`pangene permanova`, `pangene --permanova`, pg_pan_permanova, pg_pan_permanova_presence) through the checker build: the host
driver linked against the oracle backend, whose table has no pan_permanova entry, so T, A, B and k come from the plain loops of tree.cpp (A
as a double loop over pairs, y_p by indexing an order, G in __int128).  Everything is compared with the numpy / Python-int restatement of
tests/support/permanova_ref.py (A from Y @ W, G in Python ints), the printed F and R2 also with a plain float64 PERMANOVA."""
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
import dist_ref as dr  # noqa: E402
import permanova_ref as pr  # noqa: E402
import tree_ref as tr  # noqa: E402

NAMES = ["C4", "bact20", "human8"]
KINDS = (("gene", "jaccard"), ("adj", "diff"))
OPTION_SETS = [(["-n", "0"], dict(n_perm=0)), (["-n", "37", "-s", "5"], dict(n_perm=37, seed=5)), (["-n", "999"], dict(n_perm=999))]
_fixture_cache = {}


def run_cli(args, exe=CLI):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.returncode, r.stdout, r.stderr


def fixture(name, kind, metric):
    """(gfa, trait file, assembly names, trait names, labels, q, F) of a fixture, computed once"""
    key = (name, kind, metric)
    if key not in _fixture_cache:
        gfa, tf = os.path.join(GOLD, name + ".gfa.gz"), os.path.join(GOLD, "trait", name + ".tsv")
        asm, P = dr.presence(gfa, kind)
        asm = list(asm)
        names, L = pr.read_traits(tf, asm)
        q, F = tr.fixed(dr.shared(P), metric)
        _fixture_cache[key] = (gfa, tf, asm, names, L, q, F)
    return _fixture_cache[key]


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    return oracle_host.load()


@pytest.mark.parametrize("name", NAMES)
def test_fixture_files(built, name):
    """N, n1, Fbits, n_ge, p_perm and the whole text against the restatement, for both kinds of items and the three option sets"""
    n_line = 0
    for kind, metric in KINDS:
        gfa, tf, asm, names, L, q, F = fixture(name, kind, metric)
        for args, kw in OPTION_SETS:
            rc, out, err = run_cli(["permanova", "-t", tf, "-T", kind, "-m", metric] + args + [gfa])
            assert rc == 0, err
            got = pr.parse(out)
            want = [r for r in (dict(pr.one(q, l, F, **kw), Trait=nm) for nm, l in zip(names, L)) if not r["skip"]]
            n = kw["n_perm"]
            assert [(g["Trait"], g["N"], g["n1"], g["n0"], g["Fbits"], g["n_ge"], g["p_perm"]) for g in got] == \
                [(w["Trait"], w["N"], w["n1"], w["N"] - w["n1"], w["Fe"], w["k"] if n else None, "%.6f" % ((w["k"] + 1.0) / (n + 1.0)) if n else "NA") for w in want], (kind, args)
            assert out == pr.text(names, L, q, F, **kw), (kind, args)
            n_line += len(got)
    assert n_line > 0


def _line(name, kind, metric, trait, n_perm=999):
    gfa, tf = fixture(name, kind, metric)[:2]
    rc, out, err = run_cli(["permanova", "-t", tf, "-T", kind, "-m", metric, "-n", str(n_perm), gfa])
    assert rc == 0, err
    return [g for g in pr.parse(out) if g["Trait"] == trait][0]


def test_independent_pins():
    """Figures of a scratch restatement written apart from permanova_ref.py: seed 11, n = 999"""
    g = _line("C4", "gene", "jaccard", "human")
    assert (g["N"], g["n1"], g["F"], g["n_ge"]) == (33, 26, "4.676868", 58)
    g = _line("bact20", "gene", "jaccard", "even")
    assert (g["N"], g["n1"], g["F"], g["n_ge"]) == (19, 10, "0.825469", 821)
    g = _line("human8", "adj", "diff", "hap2")
    assert (g["N"], g["n1"], g["F"], g["n_ge"]) == (8, 4, "1.071572", 333)
    g = _line("bact20", "adj", "diff", "even")
    assert (g["Fbits"], g["n_ge"]) == (17, 945)


def test_scaling_of_the_fixtures():
    """s of the fixtures: 0 for the jaccard cases and for human8 and C4 adj/diff; bact20 adj/diff has 3 for even and resistant, 2 for early"""
    for name in NAMES:
        for kind, metric in KINDS:
            _, _, _, names, L, q, F = fixture(name, kind, metric)
            for nm, l in zip(names, L):
                r = pr.one(q, l, F, n_perm=0)
                if r["skip"]:
                    continue
                s = F - r["Fe"]
                want = {"even": 3, "resistant": 3, "early": 2}.get(nm, 0) if (name, kind) == ("bact20", "adj") else 0
                assert s == want, (name, kind, nm, s)


@pytest.mark.parametrize("name", NAMES)
def test_float_check(built, name):
    """F and R2 against Anderson's sums of squared distances over group sizes in plain float64 over e / 2^Fe: 1e-9 relative (the double
    sums over at most N^2 = 1 089 terms err below 1e-12).  The printed values carry six and four decimals, so they are compared at that."""
    for kind, metric in KINDS:
        gfa, tf, asm, names, L, q, F = fixture(name, kind, metric)
        rc, out, err = run_cli(["permanova", "-t", tf, "-T", kind, "-m", metric, "-n", "0", gfa])
        assert rc == 0, err
        printed = {g["Trait"]: g for g in pr.parse(out)}
        for nm, l in zip(names, L):
            r = pr.one(q, l, F, n_perm=0)
            if r["skip"]:
                continue
            cols = np.nonzero(l >= 0)[0]
            s = F - r["Fe"]
            d = (q[np.ix_(cols, cols)] >> s).astype(np.float64) / 2.0 ** r["Fe"]
            f64, r2_64 = pr.float_permanova(d, l[cols] > 0)
            _, _, f, r2 = pr.stats(r)
            print("%s %s %s: F %.17g against %.17g, R2 %.17g against %.17g" % (name, kind, nm, f, f64, r2, r2_64))
            assert abs(f - f64) <= 1e-9 * abs(f64) and abs(r2 - r2_64) <= 1e-9 * abs(r2_64)
            assert printed[nm]["F"] == "%.6f" % f and printed[nm]["R2"] == "%.4f" % r2


def _groups(N, seed, n1=None):
    rng = np.random.default_rng(seed)
    y = np.zeros(N, dtype=np.int8)
    y[rng.permutation(N)[:n1 if n1 else N // 2]] = 1
    return y


@pytest.mark.parametrize("N", [3, 5, 33, 64, 100])
def test_pan_permanova_against_the_restatement(ora, N):
    from pangene_amd import capi
    for seed in (1, 2):
        q = pr.random_matrix(N, 10 * N + seed, hi=1 << (10 + 9 * seed))
        L = np.stack([_groups(N, seed), _groups(N, seed + 7, 1), np.where(np.arange(N) % 3 == 0, -1, _groups(N, seed + 9))]).astype(np.int8)
        for n, s in ((0, 11), (61, 3)):
            assert pr.same(capi.pan_permanova(ora, q, L, n_perm=n, seed=s), pr.pan_permanova(q, L, 20, n, s)), (N, seed, n)


def test_swapping_the_labels(ora):
    """0 and 1 exchanged: every column stays but n1 and n0 (SSW is symmetric in the groups; G changes, its order does not)"""
    from pangene_amd import capi
    q, y = pr.planted(41, 3)
    y = y.astype(np.int8)
    y[[5, 9]] = -1
    a = capi.pan_permanova(ora, q, y, n_perm=200)
    b = capi.pan_permanova(ora, q, np.where(y < 0, -1, 1 - y).astype(np.int8), n_perm=200)
    assert a["N"] == b["N"] and a["n1"] + b["n1"] == a["N"] and a["T"] == b["T"] and a["k"] == b["k"] and a["Fe"] == b["Fe"]
    ra, rb = ({k: int(v[0]) for k, v in x.items()} for x in (a, b))
    assert pr.stats(ra) == pr.stats(rb)


def test_reordering_the_assemblies(ora):
    """the assemblies reordered together with the matrix: T, A, B and so F stay (the permutations do not: they act on positions)"""
    from pangene_amd import capi
    q, y = pr.planted(37, 5)
    o = np.random.default_rng(1).permutation(37)
    a = capi.pan_permanova(ora, q, y.astype(np.int8), n_perm=0)
    b = capi.pan_permanova(ora, q[np.ix_(o, o)], y[o].astype(np.int8), n_perm=0)
    assert all(a[k] == b[k] for k in ("N", "n1", "Fe", "T", "A", "B"))


def test_degenerate_inputs(built, tmp_path, ora):
    """all off-diagonal distances equal: G is the same for every labelling, k = n; an all-zero submatrix, N < 3 and an empty group print the
    note and no line; two identical blocks give SSW = 0, inf and n_ge >= the permutations that reproduce the split"""
    from pangene_amd import capi
    N = 12
    flat = (1 << 15) * (1 - np.eye(N, dtype=np.int64))
    y = _groups(N, 4)
    got = capi.pan_permanova(ora, flat, y, n_perm=50)
    assert int(got["k"][0]) == 50 and pr.same(got, pr.pan_permanova(flat, y, 20, 50))
    two = np.full(N, -1, dtype=np.int8)
    two[:2] = (0, 1)
    L = np.stack([y, np.zeros(N, dtype=np.int8), np.ones(N, dtype=np.int8), two])
    got = capi.pan_permanova(ora, np.zeros((N, N), dtype=np.int64), L)
    assert (got["k"] == -1).all() and list(got["N"]) == [N, N, N, 2]
    # two blocks: distance 0 inside, d between
    blocks = np.array([0] * 5 + [1] * 4, dtype=np.int8)
    q = (1 << 18) * (blocks[:, None] != blocks[None, :]).astype(np.int64)
    n = 300
    got = capi.pan_permanova(ora, q, blocks, n_perm=n)
    want = pr.pan_permanova(q, blocks, 20, n)
    assert pr.same(got, want)
    r = {k: int(v[0]) for k, v in got.items()}
    assert pr.stats(r)[1] == 0.0 and pr.stats(r)[2] == float("inf")
    import trait_ref
    Y = trait_ref.perm_labels(blocks.astype(np.uint8), n)
    again = int(((Y == blocks).all(axis=1) | (Y == 1 - blocks).all(axis=1)).sum())
    assert r["k"] == again  # SSW = 0 only for the split itself: with n0 != n1 only the same labelling reproduces it


def test_degenerate_text(built, tmp_path):
    gfa, tf, asm, names, L, q, F = fixture("bact20", "gene", "jaccard")
    t = tmp_path / "t.tsv"
    t.write_text("asm\tnone\ttwo\tok\n" + "".join("%s\t0\t%s\t%d\n" % (a, "1" if i < 2 else "NA", i % 2) for i, a in enumerate(asm)))
    rc, out, err = run_cli(["permanova", "-t", str(t), "-n", "10", gfa])
    assert rc == 0 and err.count(b"Note: trait") == 2 and b"none" in err and b"two" in err
    assert [g["Trait"] for g in pr.parse(out)] == ["ok"]


def test_magnitude_and_the_128_bit_compare(ora):
    """entries of 2^29 - 1 at N = 129: the definition gives s = 6 ((2^24 - 1)^2 129 128 is just above 2^62, so 5 does not do), A is near 2^60
    and N A beyond 2^63, so G needs its 128 bits"""
    from pangene_amd import capi
    N = 129
    rng = np.random.default_rng(5)
    q = pr.random_matrix(N, 5, hi=1 << 20)
    y = _groups(N, 6, 120)
    on = np.nonzero(y)[0]
    q[np.ix_(on, on)] = pr.IN_MAX - rng.integers(0, 1 << 12, size=(len(on), len(on)))
    q = np.triu(q, 1) + np.triu(q, 1).T
    want = pr.pan_permanova(q, y, 20, 40)
    assert q.max() == pr.IN_MAX and pr.shift_of(q.max(), N) == 6 and int(want["A"][0]) > 1 << 59 and N * int(want["A"][0]) > 1 << 63
    assert pr.same(capi.pan_permanova(ora, q, y, n_perm=40), want)


def test_the_boundary_of_s(ora):
    """m just below and at the value where (m >> s)^2 N (N - 1) reaches 2^62, for s = 0 and s = 1"""
    from pangene_amd import capi
    import math
    N = 1025  # N (N - 1) = 1 049 600: e < 2 096 128.9..., below 2^29
    lim = math.isqrt(((1 << 62) - 1) // (N * (N - 1)))
    assert lim ** 2 * N * (N - 1) < 1 << 62 <= (lim + 1) ** 2 * N * (N - 1)
    y = _groups(N, 2)
    base = pr.random_matrix(N, 3, hi=1 << 10)
    for m, s in ((lim, 0), (lim + 1, 1), (2 * lim + 1, 1), (2 * lim + 2, 2)):
        q = base.copy()
        q[0, 1] = q[1, 0] = m
        assert pr.shift_of(m, N) == s
        want = pr.pan_permanova(q, y, 20, 3)
        assert int(want["Fe"][0]) == 20 - s
        assert pr.same(capi.pan_permanova(ora, q, y, n_perm=3), want), m


@pytest.mark.parametrize("D", [1, 2, 3, 4, 5, 6, 7, 8])
def test_digit_planes(ora, D):
    """matrices whose w needs exactly D planes (the checker does not split w; the restatement's digits must put it together again)"""
    from pangene_amd import capi
    N = 8 if D == 8 else 40
    q = pr.digit_matrix(N, D, D)
    w = pr.weights(q, 0)
    assert pr.shift_of(q.max(), N) == 0 and pr.planes_of(int(w.max())) == D
    dg = pr.digits(w, D)
    assert sum(int(d.max()) <= 127 and int(d.min()) >= -128 for d in dg) == D and (sum(d << (8 * k) for k, d in enumerate(dg)) == w).all()
    y = _groups(N, D)
    assert pr.same(capi.pan_permanova(ora, q, y, n_perm=20), pr.pan_permanova(q, y, 20, 20))


def test_presence_route(ora):
    from pangene_amd import capi
    P = tr.lineage_presence(400, 30, 2)
    y = _groups(30, 1)
    for metric in ("jaccard", "diff"):
        q, F = tr.fixed(dr.shared(P), metric)
        got, f = capi.pan_permanova_presence(ora, P, y, metric=metric, n_perm=30)
        assert f == F and pr.same(got, pr.pan_permanova(q, y, F, 30))


def test_argument_and_range_errors(ora):
    from pangene_amd import capi
    q = pr.random_matrix(6, 1)
    y = _groups(6, 1)
    for bad in (q + np.eye(6, dtype=np.int64), q + np.triu(np.ones((6, 6), dtype=np.int64), 1), -q):
        with pytest.raises(RuntimeError, match="status -3"):
            capi.pan_permanova(ora, bad, y)
    big = q.copy()
    big[2, 3] = big[3, 2] = 1 << 29
    with pytest.raises(RuntimeError, match="status -2"):
        capi.pan_permanova(ora, big, y)
    big[2, 3] = big[3, 2] = (1 << 29) - 1
    assert pr.same(capi.pan_permanova(ora, big, y, n_perm=5), pr.pan_permanova(big, y, 20, 5))
    with pytest.raises(RuntimeError, match="status -3"):
        capi.pan_permanova(ora, q, y, frac_bits=31)
    o = capi.permanova_opt(ora)
    out = np.zeros(7, dtype=np.int64)
    q32, p32, p8, p64 = np.ascontiguousarray(q, dtype=np.int32), C.POINTER(C.c_int32), C.POINTER(C.c_int8), C.POINTER(C.c_int64)
    assert ora.pg_pan_permanova(q32.ctypes.data_as(p32), 6, y.ctypes.data_as(p8), 1, None, out.ctypes.data_as(p64)) == -3
    assert ora.pg_pan_permanova(q32.ctypes.data_as(p32), 6, None, 1, C.byref(o), out.ctypes.data_as(p64)) == -3
    assert ora.pg_pan_permanova(q32.ctypes.data_as(p32), 6, y.ctypes.data_as(p8), 1, C.byref(o), None) == -3
    assert ora.pg_pan_permanova(q32.ctypes.data_as(p32), -1, y.ctypes.data_as(p8), 1, C.byref(o), out.ctypes.data_as(p64)) == -3
    o.n_perm = -1
    assert ora.pg_pan_permanova(q32.ctypes.data_as(p32), 6, y.ctypes.data_as(p8), 1, C.byref(o), out.ctypes.data_as(p64)) == -3
    o = capi.permanova_opt(ora)
    o.metric = 1  # shared
    assert ora.pg_pan_permanova(q32.ctypes.data_as(p32), 6, y.ctypes.data_as(p8), 1, C.byref(o), out.ctypes.data_as(p64)) == -3


def test_more_columns_than_the_limit(ora):
    """N = 16 385 columns with a value: PGA_ERR_RANGE from both builds, before the matrix is looked at any further"""
    from pangene_amd import capi
    n = pr.LIMIT_N + 1
    q = np.zeros((n, n), dtype=np.int32)
    y = np.zeros(n, dtype=np.int8)
    y[::2] = 1
    with pytest.raises(RuntimeError, match="status -2"):
        capi.pan_permanova(ora, q, y, n_perm=1)
    y[0] = -1  # 16 384 columns: inside the limit (all distances zero: not tested)
    assert int(capi.pan_permanova(ora, q, y, n_perm=1)["k"][0]) == -1


def test_sizeof_and_defaults(ora):
    from pangene_amd import capi
    import re
    hdr = open(os.path.join(ROOT, "include", "pangene_amd.h")).read()
    assert int(re.search(r"sizeof\(pg_permanova_opt_t\) is (\d+)", hdr).group(1)) == C.sizeof(capi.pg_permanova_opt_t) == 20
    o = capi.pg_permanova_opt_t()
    C.memset(C.byref(o), 0xff, C.sizeof(o))
    ora.pg_permanova_opt_init(C.byref(o))
    assert (o.type, o.metric, o.n_perm, o.seed, o.frac_bits) == (0, 0, 1000, 11, 20)


def test_refusals(built, tmp_path):
    gfa, tf = fixture("C4", "gene", "jaccard")[:2]
    d = os.path.join(GOLD, "C4")
    pafs = sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)
    for args, word in ((["permanova", "-t", tf, "-m", "shared", gfa], b"-m"), (["permanova", gfa], b"-t FILE"), (["permanova", "-t", tf, "-n", "-1", gfa], b"-n"),
                       (["permanova", "-t", tf, "-T", "walk", gfa], b"-T"),
                       (["--gpus", "2", "--permanova=" + tf] + pafs, b"--permanova"),
                       (["--permanova=" + tf, "--permanova-metric=shared"] + pafs, b"--permanova-metric"),
                       (["--permanova-perm=5"] + pafs, b"need --permanova"), (["--permanova-seed=5"] + pafs, b"need --permanova"),
                       (["--permanova-type=adj"] + pafs, b"need --permanova"), (["--permanova-metric=diff"] + pafs, b"need --permanova")) + \
            tuple((["--permanova=" + tf, other] + pafs, b"cannot be combined") for other in
                  ("--matrix", "--call", "--curves", "--dist", "--assoc", "--trait=" + tf, "--qtrait=" + tf, "--tree", "--cluster=2")):
        rc, out, err = run_cli(args)
        assert rc == 1 and out == b"" and word in err, (args[:3], err)


def test_trait_file_errors(built, tmp_path):
    """trait's errors with their line number"""
    gfa, tf, asm = fixture("human8", "gene", "jaccard")[:3]
    for body, word in (("asm\tt\n%s\t2\n" % asm[0], b"line 2: value 2 is not"), ("asm\tt\nnobody\t1\n", b"line 2: no assembly named"),
                       ("asm\tt\n%s\t1\n%s\t0\n" % (asm[0], asm[0]), b"line 3: assembly"), ("asm\tt\n%s\t1\t0\n" % asm[0], b"line 2: 3 fields")):
        t = tmp_path / "bad.tsv"
        t.write_text(body)
        rc, out, err = run_cli(["permanova", "-t", str(t), gfa])
        assert rc == 1 and out == b"" and word in err, err
    rc, out, err = run_cli(["permanova", "-t", str(tmp_path / "missing.tsv"), gfa])
    assert rc == 1 and out == b"" and b"cannot open trait file" in err


def test_in_memory_route(built, tmp_path):
    """`pangene --permanova=F *.paf` prints what `pangene permanova -t F` prints for the GFA of the same run"""
    d, tf = os.path.join(GOLD, "human8"), os.path.join(GOLD, "trait", "human8.tsv")
    pafs = sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)
    rc, gfa, _ = run_cli(pafs)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    for mem, fil in ((["--permanova=" + tf], []),
                     (["--permanova=" + tf, "--permanova-type=adj", "--permanova-metric=diff", "--permanova-perm=77", "--permanova-seed=4"], ["-T", "adj", "-m", "diff", "-n", "77", "-s", "4"])):
        rc1, a, _ = run_cli(mem + pafs)
        rc2, b, _ = run_cli(["permanova", "-t", tf] + fil + [str(tmp_path / "g.gfa")])
        assert rc1 == 0 and rc2 == 0 and a == b and a.count(b"\n") > 1, mem


def test_capi_run(ora):
    from pangene_amd import capi
    d, tf = os.path.join(GOLD, "human8"), os.path.join(GOLD, "trait", "human8.tsv")
    pafs = sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)
    a = capi.run(ora, pafs, ["--permanova=" + tf, "--permanova-perm=20"])
    rc, b, _ = run_cli(["--permanova=" + tf, "--permanova-perm=20"] + pafs)
    assert rc == 0 and a == b and a.startswith((pr.HEADER + "\n").encode())
    with pytest.raises(ValueError):
        capi.run(ora, pafs, ["--permanova-perm=20"])
    with pytest.raises(ValueError):
        capi.run(ora, pafs, ["--permanova=" + tf, "--cluster=2"])
