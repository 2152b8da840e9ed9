"""Quantitative traits (`pangene qtrait`, `pangene --qtrait`, pg_pan_qtrait) through the checker build: the host driver linked against the
oracle backend, whose table has no pan_qtrait entry, so the permutations run as the plain host loops of trait.cpp.  Everything is
compared with the numpy restatement of tests/support/qtrait_ref.py: names, line order, the integer columns, U and p_perm as text; auc,
z, p_wilcox and q_bh within 1e-3 relative of what the restatement prints -- both sides through the column's format, because the
tolerance is about the four printed digits: an auc of 0.03125 prints as 0.0312 or 0.0313, which no implementation could bring within
1e-3 relative of the unrounded number."""
import gzip
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
import dist_ref  # noqa: E402
import qtrait_ref as qr  # noqa: E402
import trait_ref as tr  # noqa: E402

NAMES = ["C4", "bact20", "human8"]
HEADER = (qr.HEADER + "\n").encode()
OPTION_SETS = [([], {}), (["-n", "0"], dict(n_perm=0)), (["-n", "37", "-s", "5", "-c", "2"], dict(n_perm=37, seed=5, min_count=2)),
               (["-n", "3000", "-p", "0.07"], dict(n_perm=3000, max_p=0.07))]
FLOAT_COLS = (("auc", 5, "%.4f"), ("z", 6, "%.4f"), ("p_wilcox", 7, "%.3e"), ("q_bh", 8, "%.3e"))


def run_cli(args, exe=CLI):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    return oracle_host.load()


def load(name):
    gfa = os.path.join(GOLD, name + ".gfa.gz")
    genes, P = ar.read_gfa(gfa)
    asm = list(dist_ref.presence(gfa, "gene")[0])
    return gfa, genes, asm, P


def compare(out, want_rows):
    """a printed table against the restatement's rows, as the module docstring says"""
    got = qr.parse(out)
    assert len(got) == len(want_rows)
    for g, w in zip(got, want_rows):
        assert (g["Trait"], g["Gene"], g["N"], g["nG"], g["U"], g["n_ge"], g["p_perm"]) == (w[0], w[1], w[2], w[3], w[4], w[9], w[10]), (g, w)
        for key, i, fmt in FLOAT_COLS:
            printed = float(fmt % w[i])
            assert abs(g[key] - printed) <= 1e-3 * abs(printed), (key, g, w)


def _write(path, txt):
    path.write_text(txt)
    return path


@pytest.mark.parametrize("name", NAMES)
def test_fixture_files(built, name):
    gfa, genes, asm, P = load(name)
    tf = os.path.join(GOLD, "qtrait", name + ".tsv")
    names, V = qr.read_file(tf, asm)
    assert names == ["planted", "ties", "binary"]
    n_line = 0
    for args, kw in OPTION_SETS:
        if "max_p" in kw:  # the cutoff must not sit on a p: no restatement p within 1e-6 relative of it
            assert all(abs(w[7] - kw["max_p"]) > 1e-6 * kw["max_p"] for w in qr.table(genes, asm, P, names, V, n_perm=0))
        want = qr.table(genes, asm, P, names, V, **kw)
        rc, out, err = run_cli(["qtrait", "-t", tf] + args + [gfa])
        assert rc == 0 and out.startswith(HEADER), err
        compare(out, want)
        n_line += len(want)
    assert n_line > 0


@pytest.mark.parametrize("name", NAMES)
def test_binary_trait_gives_what_trait_gives(built, tmp_path, name):
    """on 0 / 1 values c2 is N - t and -t, D = s N - a t: n_ge and p_perm are those of pangene trait on the same labels"""
    gfa, genes, asm, P = load(name)
    names, V = qr.read_file(os.path.join(GOLD, "qtrait", name + ".tsv"), asm)
    b = V[names.index("binary")]
    assert set(np.unique(b)) == {0.0, 1.0}
    L = b.astype(np.int8)[None, :]
    fq = _write(tmp_path / "q.tsv", qr.trait_file(asm, ["binary"], [[str(int(x)) for x in b]]))
    ft = _write(tmp_path / "t.tsv", tr.trait_file(asm, ["binary"], L))
    for n, s in ((200, 11), (61, 7)):
        rc1, a, _ = run_cli(["qtrait", "-t", str(fq), "-n", str(n), "-s", str(s), "-c", "2", gfa])
        rc2, c, _ = run_cli(["trait", "-t", str(ft), "-n", str(n), "-s", str(s), "-c", "2", gfa])
        assert rc1 == 0 and rc2 == 0
        qa, ta = qr.parse(a), tr.parse(c)
        assert len(qa) == len(ta) > 0
        assert [(x["Gene"], x["N"], x["nG"], x["n_ge"], x["p_perm"]) for x in qa] == [(x["Gene"], x["N"], x["nG"], str(x["n_ge"]), x["p_perm"]) for x in ta]


def test_negated_values_negate_d(ora):
    from pangene_amd import capi
    P = ar.planted(300, 90, 5)
    rng = np.random.default_rng(8)
    V = np.stack([rng.normal(size=90), np.round(rng.normal(size=90) * 2.0)])
    V[1, rng.random(90) < 0.1] = np.nan
    a = capi.pan_qtrait(ora, P, V, n_perm=150, seed=3)
    b = capi.pan_qtrait(ora, P, -V, n_perm=150, seed=3)
    assert np.array_equal(a["D"], -b["D"]) and np.array_equal(a["k"], b["k"]) and np.array_equal(a["a"], b["a"]) and np.abs(a["D"]).sum() > 0
    assert int(a["k"].sum()) > 0


def test_against_scipy(built):
    """U and p_wilcox of every printed line of one fixture against scipy's asymptotic Mann-Whitney test without continuity correction"""
    stats = pytest.importorskip("scipy.stats")
    gfa, genes, asm, P = load("bact20")
    tf = os.path.join(GOLD, "qtrait", "bact20.tsv")
    names, V = qr.read_file(tf, asm)
    rc, out, _ = run_cli(["qtrait", "-t", tf, "-n", "0", gfa])
    assert rc == 0
    rows = qr.parse(out)
    assert rows
    at = {g: i for i, g in enumerate(genes)}
    for r in rows:
        v = V[names.index(r["Trait"])]
        ok = ~np.isnan(v)
        carriers, others = v[ok & P[at[r["Gene"]]]], v[ok & ~P[at[r["Gene"]]]]
        res = stats.mannwhitneyu(carriers, others, use_continuity=False, method="asymptotic")
        assert r["U"] == "%.1f" % res.statistic, r
        assert abs(r["p_wilcox"] - float("%.3e" % res.pvalue)) <= 1e-3 * res.pvalue, (r, res)


def test_gzipped_trait_file_comments_and_blank_lines(built, tmp_path):
    gfa, genes, asm, P = load("C4")
    txt = open(os.path.join(GOLD, "qtrait", "C4.tsv")).read()
    rc, a, _ = run_cli(["qtrait", "-t", os.path.join(GOLD, "qtrait", "C4.tsv"), "-n", "20", gfa])
    lines = txt.split("\n")
    lines[2:2] = ["# a comment", ""]
    with gzip.open(tmp_path / "z.tsv.gz", "wt") as f:
        f.write("\n".join(lines))
    rc2, b, _ = run_cli(["qtrait", "-t", str(tmp_path / "z.tsv.gz"), "-n", "20", gfa])
    assert rc == 0 and rc2 == 0 and a == b and a.count(b"\n") > 1


def test_trait_file_errors(built, tmp_path):
    """a name the matrix does not have, a repeated name, a wrong field count, and every value that is no finite number: status 1, nothing
    on stdout, the line number"""
    gfa, genes, asm, P = load("C4")
    assert len(asm) >= 3
    good = ["asm\tx\ty"] + ["%s\t%d.5\t-%de-1" % (a, i, i) for i, a in enumerate(asm)]
    cases = []
    bad = list(good); bad[2] = "nobody\t1\t0"; cases.append((bad, 3))
    bad = list(good); bad[3] = bad[1]; cases.append((bad, 4))
    bad = list(good); bad[2] = bad[2] + "\t1"; cases.append((bad, 3))
    bad = list(good); bad[1] = asm[0] + "\t1"; cases.append((bad, 2))
    for v in ("nan", "NaN", "inf", "-inf", "1e999", "-1e999", "1.5x", "1 2", "-", "yes", "1,5", "--1"):
        bad = list(good); bad[3] = asm[2] + "\t" + v + "\t0"; cases.append((bad, 4))
    bad = list(good); bad[2:2] = ["# note", ""]; bad[5] = asm[2] + "\t0\tinfinity"; cases.append((bad, 6))
    for lines, ln in cases:
        f = _write(tmp_path / "t.tsv", "\n".join(lines) + "\n")
        rc, out, err = run_cli(["qtrait", "-t", str(f), "-n", "5", gfa])
        assert rc == 1 and out == b"" and (b"line %d" % ln) in err, (lines, err)
    f = _write(tmp_path / "ok.tsv", "\n".join(good) + "\n")
    rc, out, _ = run_cli(["qtrait", "-t", str(f), "-n", "5", gfa])
    assert rc == 0 and out.startswith(HEADER)
    rc, out, err = run_cli(["qtrait", "-t", str(tmp_path / "none.tsv"), gfa])
    assert rc == 1 and out == b""
    rc, out, err = run_cli(["qtrait", "-n", "5", gfa])
    assert rc == 1 and out == b"" and b"-t" in err
    for bad in (["-n", "-1"], ["-n", "x"], ["-n", "2147483647"], ["-c", "0"], ["-p", "-1"], ["-p", "x"]):
        rc, out, _ = run_cli(["qtrait", "-t", str(f)] + bad + [gfa])
        assert rc == 1 and out == b""
    rc, out, _ = run_cli(["qtrait", "-t", str(f), str(tmp_path / "none.gfa")])
    assert rc == 1 and out == b""


def test_degenerate_traits(built, tmp_path):
    """all values equal (-0.0 equals 0.0), one value only, missing everywhere: a note each on stderr and no lines; the good trait prints"""
    gfa, genes, asm, P = load("bact20")
    A = len(asm)
    fields = [["0.0" if c % 2 else "-0.0" for c in range(A)], ["3.5" if c == 4 else "NA" for c in range(A)], ["NA"] * A,
              ["%d.25" % (c % 7) for c in range(A)]]
    names = ["flat", "single", "nothing", "good"]
    lines = ["assembly\t" + "\t".join(names)] + [asm[c] + "\t" + "\t".join(fields[t][c] for t in range(4)) for c in range(A)]
    f = _write(tmp_path / "t.tsv", "\n".join(lines) + "\n")
    rc, out, err = run_cli(["qtrait", "-t", str(f), "-n", "10", gfa])
    assert rc == 0 and out.startswith(HEADER)
    rows = qr.parse(out)
    assert rows and {r["Trait"] for r in rows} == {"good"}
    assert all(b"trait " + n.encode() in err for n in names[:3]) and b"trait good" not in err
    V = np.array([[np.nan if x == "NA" else float(x) for x in row] for row in fields])
    compare(out, qr.table(genes, asm, P, names, V, n_perm=10))


def test_assembly_the_file_does_not_name_is_missing(built, tmp_path):
    gfa, genes, asm, P = load("bact20")
    V = np.random.default_rng(9).normal(size=(1, len(asm)))
    V[0, :3] = np.nan
    txt = qr.trait_file(asm, ["t"], [["NA" if np.isnan(x) else repr(float(x)) for x in V[0]]])
    assert all(not l.startswith(asm[0] + "\t") for l in txt.split("\n"))
    rc, out, _ = run_cli(["qtrait", "-t", str(_write(tmp_path / "t.tsv", txt)), "-n", "50", gfa])
    assert rc == 0
    want = qr.table(genes, asm, P, ["t"], V, n_perm=50)
    assert want and want[0][2] == len(asm) - 3
    compare(out, want)


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", ["C4", "bact20"])
def test_in_memory_route_equals_file_route(built, tmp_path, name):
    """`pangene --qtrait=F *.paf` (pg_write_qtrait on the graph in memory) prints what `pangene *.paf > g.gfa; pangene qtrait -t F g.gfa` prints"""
    files, f = _paf_dir(name), os.path.join(GOLD, "qtrait", name + ".tsv")
    rc, gfa, _ = run_cli(files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    rc1, a, _ = run_cli(["--qtrait=" + f] + files)
    rc2, b, _ = run_cli(["qtrait", "-t", f, str(tmp_path / "g.gfa")])
    assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(HEADER) and a.count(b"\n") > 1
    rc1, a, _ = run_cli(["--qtrait=" + f, "--qtrait-perm=33", "--qtrait-seed=4"] + files)
    rc2, b, _ = run_cli(["qtrait", "-t", f, "-n", "33", "-s", "4", str(tmp_path / "g.gfa")])
    assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(HEADER)


def test_python_run_equals_command_line(ora):
    from pangene_amd import capi
    files, f = _paf_dir("C4"), os.path.join(GOLD, "qtrait", "C4.tsv")
    assert capi.run(ora, files, ["--qtrait=" + f, "--qtrait-perm=12"]) == run_cli(["--qtrait=" + f, "--qtrait-perm=12"] + files)[1]


def test_refusals_and_usage(built, tmp_path):
    files = _paf_dir("C4")
    f = str(_write(tmp_path / "t.tsv", "a\tx\n"))
    rc, out, err = run_cli(["--gpus", "2", "--qtrait=" + f] + files)
    assert rc == 1 and out == b"" and b"--qtrait" in err
    for extra in (["--matrix"], ["--call"], ["--matrix=count"], ["--curves"], ["--dist"], ["--assoc"], ["--trait=" + f], ["--tree"]):
        rc, out, err = run_cli(["--qtrait=" + f] + extra + files)
        assert rc == 1 and out == b"" and b"--qtrait" in err, extra
    for alone in (["--qtrait-perm=5"], ["--qtrait-seed=5"]):
        rc, out, err = run_cli(alone + files)
        assert rc == 1 and out == b"" and b"--qtrait" in err
    rc, out, _ = run_cli(["--qtrait=" + f, "--qtrait-perm=-3"] + files)
    assert rc == 1 and out == b""
    rc, out, _ = run_cli(["qtrait"])
    assert rc == 0 and out.startswith(b"Usage: pangene qtrait -t FILE [options] <in.gfa>\n")
    rc, _, err = run_cli([])
    assert b"pangene qtrait -t FILE [-n INT] [-s INT] [-c INT] [-p FLOAT] <in.gfa>" in err
    assert b"--qtrait=FILE" in err and b"--qtrait-perm=INT" in err and b"--qtrait-seed=INT" in err


def test_option_struct_size(ora):
    import ctypes as C
    from pangene_amd import capi
    assert C.sizeof(capi.pg_qtrait_opt_t) == 24
    o = capi.qtrait_opt(ora)
    assert (o.n_perm, o.seed, o.min_count, o.max_p) == (1000, 11, 1, 1.0)
    # the library writes the struct it was compiled with: a guard word behind 24 bytes stays untouched by pg_qtrait_opt_init
    buf = (C.c_uint8 * 32)(*([0xAB] * 32))
    ora.pg_qtrait_opt_init(C.cast(buf, C.c_void_p))
    assert bytes(buf[24:]) == b"\xab" * 8 and bytes(buf[:4]) == (1000).to_bytes(4, "little") and bytes(buf[12:16]) == b"\0" * 4


def make_values(A, seed):
    """(5, A) float64: continuous, heavy ties with NaN, 0 / 1, all equal, missing everywhere"""
    rng = np.random.default_rng(seed)
    V = np.full((5, A), np.nan)
    V[0] = rng.normal(size=A)
    V[1] = rng.integers(-2, 3, size=A)
    V[1, rng.random(A) < 0.3] = np.nan
    V[2] = rng.integers(0, 2, size=A)
    V[3] = 4.0
    return V


SHAPES = [(0, 5), (7, 1), (50, 2), (129, 31), (130, 32), (257, 33), (300, 100), (1, 64)]


@pytest.mark.parametrize("G,A", SHAPES, ids=["G%d-A%d" % s for s in SHAPES])
def test_pan_qtrait_random(ora, G, A):
    from pangene_amd import capi
    P = ar.planted(G, A, G * 7919 + A)
    V = make_values(A, G + A)
    for kw in (dict(n_perm=60), dict(n_perm=0), dict(n_perm=45, seed=3, min_count=2)):
        got = capi.pan_qtrait(ora, P, V, **kw)
        want = qr.pan_qtrait(P, V, **kw)
        for key in ("N", "a", "D", "k"):
            assert got[key].dtype == np.int32 and got[key].shape == (5, G) and np.array_equal(got[key], want[key]), (key, kw)
    one = capi.pan_qtrait(ora, P, V[0], n_perm=10)
    assert one["k"].shape == (1, G) and np.array_equal(one["k"], qr.pan_qtrait(P, V[0], n_perm=10)["k"])


def test_pan_qtrait_arguments(ora):
    torch = pytest.importorskip("torch")
    from pangene_amd import capi
    P = ar.planted(200, 40, 4)
    V = make_values(40, 1)
    a = capi.pan_qtrait(ora, torch.from_numpy(P), torch.from_numpy(V), n_perm=30)
    b = capi.pan_qtrait(ora, P, V, n_perm=30)
    assert all(np.array_equal(a[k], b[k]) for k in a) and int(b["k"].sum()) > 0
    for kw in (dict(n_perm=-1), dict(n_perm=2 ** 31 - 1), dict(min_count=0)):
        with pytest.raises(ValueError):
            capi.pan_qtrait(ora, P, V, **kw)
    with pytest.raises(ValueError):
        capi.pan_qtrait(ora, P, V[:, :39])
    W = V.copy()
    W[0, 3] = np.inf
    with pytest.raises(ValueError):
        capi.pan_qtrait(ora, P, W)


def test_ranks_by_sorting_are_the_ranks():
    for seed, ties in ((1, False), (2, True), (3, True)):
        rng = np.random.default_rng(seed)
        v = rng.normal(size=301)
        if ties:
            v = np.round(v * seed)
            v[:3] = (0.0, -0.0, 0.0)
        assert np.array_equal(qr.ranks_sorted(v), qr.ranks(v)[0])


def test_limit_inputs(ora):
    """the inputs of the `limit` GPU cases (qtrait_ref.limit_inputs) meet their own conditions -- hi = +-125 and lo = -128 and 127, the
    ends of the two signed-byte planes (an odd c2 has an odd lo, so the two ends of lo need both parities of N), the largest |D| of
    the definition, three tie groups -- and the checker build gives what the restatement gives.  (The
    checker build reads values, not ranks: the values are the ranks themselves.)"""
    from pangene_amd import capi
    for label, B, c2 in qr.limit_inputs():
        N = len(c2)
        lo, hi = qr.digits(c2)
        assert np.array_equal(256 * hi + lo, c2) and int(c2.sum()) == 0 and int(np.abs(c2).max()) <= qr.LIMIT_N - 1, label
        if "ties" not in label:
            # every value of the parity of N - 1: the odd ones reach lo = 127 (and -127), the even ones lo = -128 (and 126)
            assert sorted(c2.tolist()) == list(range(-(N - 1), N, 2))
            assert (int(hi.max()), int(hi.min()), int(lo.min()), int(lo.max())) == ((125, -125, -127, 127) if N == qr.LIMIT_N else (125, -125, -128, 126))
        else:
            assert len(set(c2.tolist())) == 3 and np.array_equal(c2, qr.ranks_sorted(c2))
        a, D, k, el, first = qr.counts(B, c2, qr.LIMIT_PERM, d_rows=qr.LIMIT_PERM)
        if N == qr.LIMIT_N:
            assert int(D[0]) == N * N // 4 == -int(D[1]) and int(a[0]) == N // 2 and 2 ** 27 < N * N // 4 < 2 ** 30
        assert int(a[3]) == 0 and int(a[4]) == N and not first[:, 3:5].any() and int(k.sum()) > 0 and int(k[0]) == 0, label
        got = capi.pan_qtrait(ora, B, c2.astype(np.float64), n_perm=qr.LIMIT_PERM)
        assert np.array_equal(got["a"][0], np.where(el, a, -1)) and np.array_equal(got["D"][0], np.where(el, D, 0)), label
        assert np.array_equal(got["k"][0], k), label
