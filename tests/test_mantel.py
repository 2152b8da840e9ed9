"""The Mantel test (`pangene mantel`, `pangene --mantel`, pg_pan_mantel) through the checker build: the host driver linked against the oracle
backend, whose table has no pan_mantel entry, so Z and the two counts come from the plain loops of tree.cpp (the order from
fisher_yates_order, a double loop over i < j, doubled).  Everything is compared with the numpy / Python-int restatement of
tests/support/mantel_ref.py (Z from b[np.ix_(o, o)], r from `decimal` at 50 digits)."""
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
import mantel_ref as mr  # noqa: E402
import tree_ref as tr  # noqa: E402

NAMES = ["C4", "bact20", "human8"]
# (command-line options, X, Y, the restatement's options): the four option sets of the file route
OPTION_SETS = [([], "gene:jaccard", "adj:jaccard", {}), (["-x", "adj:diff", "-y", "gene:jaccard"], "adj:diff", "gene:jaccard", {}),
               (["-n", "0"], "gene:jaccard", "adj:jaccard", dict(n_perm=0)), (["-n", "37", "-s", "5"], "gene:jaccard", "adj:jaccard", dict(n_perm=37, seed=5))]
_cache = {}


def run_cli(args, exe=CLI):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.returncode, r.stdout, r.stderr


def gfa_of(name):
    return os.path.join(GOLD, name + ".gfa.gz")


def fixed(name, spec):
    """(assembly names, q) of a fixture for gene|adj:jaccard|diff, computed once"""
    if (name, spec) not in _cache:
        kind, metric = spec.split(":")
        asm, P = dr.presence(gfa_of(name), kind)
        _cache[name, spec] = (list(asm), tr.fixed(dr.shared(P), metric)[0])
    return _cache[name, spec]


def pafs_of(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    return oracle_host.load()


@pytest.mark.parametrize("name", NAMES)
def test_file_route(built, name):
    """the whole text against the restatement for the default, swapped matrices, no permutations and another count and seed"""
    for args, x, y, kw in OPTION_SETS:
        rc, out, err = run_cli(["mantel"] + args + [gfa_of(name)])
        assert rc == 0, err
        (asm, qx), (asm_y, qy) = fixed(name, x), fixed(name, y)
        assert asm == asm_y
        assert out == mr.text(x, y, qx, qy, **kw), (args, out)
        got = mr.parse(out)
        assert got is not None and got["N"] == len(asm) and (got["p_greater"] == "NA") == (kw.get("n_perm") == 0)


def test_independent_pins():
    """Figures of a scratch restatement written apart from mantel_ref.py (float64 Pearson correlation of the two upper triangles; the
    counts from a loop over curves_ref.order): seed 11, n = 1000"""
    for name, want in (("C4", (33, "0.6873", 0, 1000)), ("human8", (8, "0.8500", 1, 999))):
        rc, out, err = run_cli(["mantel", gfa_of(name)])
        g = mr.parse(out)
        assert rc == 0 and (g["N"], g["r"], g["n_ge"], g["n_le"]) == want, out


@pytest.mark.parametrize("name", NAMES)
def test_float_check(built, name):
    """r against numpy's float64 Pearson correlation of the off-diagonal entries: within 5e-5 + 1e-9, the %.4f rounding plus float64's
    error over at most 33 x 32 terms"""
    rc, out, err = run_cli(["mantel", "-n", "0", gfa_of(name)])
    (asm, qx), (_, qy) = fixed(name, "gene:jaccard"), fixed(name, "adj:jaccard")
    off = ~np.eye(len(asm), dtype=bool)
    want = np.corrcoef(qx[off].astype(np.float64), qy[off].astype(np.float64))[0, 1]
    assert rc == 0 and abs(float(mr.parse(out)["r"]) - want) <= 5e-5 + 1e-9


def _matrix_case(name, tmp_path, phylip):
    """the adj:diff distances of a fixture as a matrix file: rows and columns shuffled, one assembly left out, one name nobody has added"""
    asm, qy = fixed(name, "adj:diff")
    rng = np.random.default_rng(len(asm) + phylip)
    keep = rng.permutation(len(asm))[:-1]  # the last of the shuffle is missing from the file
    names = [asm[k] for k in keep] + ["nobody#0"]
    S = dr.shared(dr.presence(gfa_of(name), "adj")[1])
    d = dr.metric(S, "diff")[np.ix_(keep, keep)].astype(np.float64)
    d = np.pad(d, ((0, 1), (0, 1)), constant_values=3.0)
    d[-1, -1] = 0.0
    pos = rng.permutation(len(names))  # and "nobody" goes somewhere in the middle
    names, d = [names[k] for k in pos], d[np.ix_(pos, pos)]
    path = tmp_path / ("m.phy" if phylip else "m.tsv")
    path.write_text(mr.matrix_text(names, d, phylip, fmt="%d"))
    return str(path), asm, names


@pytest.mark.parametrize("phylip", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_matrix_file(built, tmp_path, name, phylip):
    """-f FILE in both forms: N is the assemblies both name, in the GFA's order; the two names on one side only get a note each"""
    path, asm, names = _matrix_case(name, tmp_path, phylip)
    fnames, qf, F = mr.read_matrix(path)
    assert fnames == names and 0 <= F <= 20
    _, qx = fixed(name, "gene:jaccard")
    a, b = mr.matched(asm, qx, fnames, qf)
    assert a.shape[0] == len(asm) - 1
    rc, out, err = run_cli(["mantel", "-f", path, "-n", "99", gfa_of(name)])
    assert rc == 0, err
    assert out == mr.text("gene:jaccard", "file", a, b, n_perm=99), out
    missing = [n for n in asm if n not in names]
    assert len(missing) == 1 and err.count(b"Note: assembly") == 2
    assert ("Note: assembly %s is in gene:jaccard only" % missing[0]).encode() in err and b"Note: assembly nobody#0 is in file only" in err


def test_matrix_file_scale(built, tmp_path):
    """r does not depend on F: the adj:diff counts and the same counts times 4 096 (F smaller by 12) print the same line; and the text of
    `pangene dist` itself is read back: gene:jaccard against its own six decimals gives r = 1.0000"""
    gfa = gfa_of("bact20")
    asm, _ = fixed("bact20", "gene:jaccard")
    d = dr.metric(dr.shared(dr.presence(gfa, "adj")[1]), "diff")
    (tmp_path / "a.tsv").write_text(mr.matrix_text(asm, d, fmt="%d"))
    (tmp_path / "b.tsv").write_text(mr.matrix_text(asm, d * 4096, fmt="%d"))
    Fa, Fb = mr.read_matrix(str(tmp_path / "a.tsv"))[2], mr.read_matrix(str(tmp_path / "b.tsv"))[2]
    assert Fa - Fb == 12 and Fb >= 0
    outs = []
    for f in ("a.tsv", "b.tsv"):
        rc, out, err = run_cli(["mantel", "-f", str(tmp_path / f), "-n", "30", gfa])
        assert rc == 0 and mr.parse(out) is not None, err
        outs.append(out)
    assert outs[0] == outs[1]
    rc, table, _ = run_cli(["dist", gfa])
    assert rc == 0
    (tmp_path / "c.tsv").write_bytes(table)
    rc, out, err = run_cli(["mantel", "-f", str(tmp_path / "c.tsv"), "-n", "50", gfa])
    g = mr.parse(out)
    assert rc == 0 and g["r"] == "1.0000" and g["Y"] == "file" and g["n_le"] == 50


def test_matrix_file_errors(built, tmp_path):
    """the reader's errors name the file and the line"""
    gfa = gfa_of("human8")
    a, b, c = fixed("human8", "gene:jaccard")[0][:3]
    for body, word in (("Asm\t%s\t%s\n%s\t0\t1\n" % (a, b, a), b"line 2: the matrix is not square: 1 rows, 2 columns"),
                       ("Asm\t%s\t%s\n%s\t0\t1\t2\n%s\t1\t0\n" % (a, b, a, b), b"line 2: the matrix is not square: 3 values in a row, 2 columns"),
                       ("2\n%s 0 1\n%s 1 0\n%s 1 1\n" % (a, b, c), b"line 4: the matrix is not square: more than 2 rows"),
                       ("Asm\t%s\t%s\n%s\t0\tx\n%s\t1\t0\n" % (a, b, a, b), b"line 2: value x is not a finite number >= 0"),
                       ("Asm\t%s\t%s\n%s\t0\t-1\n%s\t-1\t0\n" % (a, b, a, b), b"line 2: value -1 is not a finite number >= 0"),
                       ("Asm\t%s\t%s\n%s\t0\tnan\n%s\t1\t0\n" % (a, b, a, b), b"line 2: value nan is not"), ("2\n%s 0 inf\n%s 1 0\n" % (a, b), b"line 2: value inf is not"),
                       ("2\n%s 0 1e\n%s 1 0\n" % (a, b), b"line 2: value 1e is not"),
                       ("Asm\t%s\t%s\n%s\t0\t1\n%s\t1\t0.5\n" % (a, b, a, b), b"line 3: the diagonal value 0.5 is not 0"),
                       ("Asm\t%s\t%s\n%s\t0\t1\n%s\t2\t0\n" % (a, b, a, b), b"line 3: the matrix is not symmetric"),
                       ("Asm\t%s\t%s\n%s\t0\t1\n%s\t1\t0\n" % (a, b, b, a), b"line 2: row"), ("2\n%s 0 1\n%s 1 0\n" % (a, a), b"line 3: assembly"),
                       ("2\n%s 0 1e9\n%s 1e9 0\n" % (a, b), b"does not fit 29 bits"), ("x y\n", b"line 1: neither an Asm header line nor a count"), ("\n\n", b"no header line")):
        t = tmp_path / "bad.txt"
        t.write_text(body)
        rc, out, err = run_cli(["mantel", "-f", str(t), gfa])
        assert rc == 1 and out == b"" and word in err and str(t).encode() in err, (body, err)
    rc, out, err = run_cli(["mantel", "-f", str(tmp_path / "missing.tsv"), gfa])
    assert rc == 1 and out == b"" and b"cannot open matrix file" in err
    # symmetric after the conversion is what counts: 1 and 1 + 2^-22 both become 2^20 at F = 20
    (tmp_path / "ok.txt").write_text("3\n%s 0 1 2\n%s 1.0000002 0 4\n%s 2 4 0\n" % (a, b, c))
    rc, out, err = run_cli(["mantel", "-f", str(tmp_path / "ok.txt"), "-n", "0", gfa])
    assert rc == 0 and mr.parse(out)["N"] == 3, err


def test_refusals(built):
    gfa, pafs = gfa_of("C4"), pafs_of("C4")
    for args, word in ((["mantel", "-x", "gene", gfa], b"-x"), (["mantel", "-x", "gene:shared", gfa], b"-x"), (["mantel", "-y", "walk:diff", gfa], b"-y"),
                       (["mantel", "-y", "adj:diff", "-f", gfa, gfa], b"-y cannot be combined with -f"), (["mantel", "-n", "-1", gfa], b"-n"),
                       (["mantel", "-n", "2147483647", gfa], b"-n"),
                       (["--gpus", "2", "--mantel"] + pafs, b"--mantel"), (["--mantel", "--mantel-x=gene:shared"] + pafs, b"--mantel-x"),
                       (["--mantel", "--mantel-y=adj"] + pafs, b"--mantel-y"), (["--mantel", "--mantel-perm=-1"] + pafs, b"--mantel-perm"),
                       (["--mantel=" + gfa, "--mantel-y=adj:diff"] + pafs, b"--mantel-y cannot be combined with --mantel=FILE"),
                       (["--mantel-perm=5"] + pafs, b"need --mantel"), (["--mantel-seed=5"] + pafs, b"need --mantel"), (["--mantel-x=adj:diff"] + pafs, b"need --mantel"),
                       (["--mantel-y=adj:diff"] + pafs, b"need --mantel")) + \
            tuple((["--mantel", other] + pafs, b"cannot be combined") for other in
                  ("--matrix", "--call", "--curves", "--dist", "--assoc", "--trait=" + gfa, "--qtrait=" + gfa, "--tree", "--cluster=2", "--permanova=" + gfa)):
        rc, out, err = run_cli(args)
        assert rc == 1 and out == b"" and word in err, (args[:3], err)
    rc, out, err = run_cli(["mantel", os.path.join(GOLD, "no_such.gfa")])
    assert rc == 1 and out == b"" and b"cannot open" in err


def test_degenerate_inputs(built, tmp_path, ora):
    """N < 3 and a constant matrix: a note on stderr, the header only, exit 0; pg_pan_mantel reports the sums, Z = 0 and -1 for the counts"""
    from pangene_amd import capi
    gfa = gfa_of("human8")
    asm = fixed("human8", "gene:jaccard")[0]
    (tmp_path / "two.txt").write_text("2\n%s 0 1\n%s 1 0\n" % (asm[0], asm[1]))
    rc, out, err = run_cli(["mantel", "-f", str(tmp_path / "two.txt"), gfa])
    assert rc == 0 and out == (mr.HEADER + "\n").encode() and b"fewer than 3 assemblies" in err
    flat = 2.5 * (1 - np.eye(len(asm)))
    (tmp_path / "flat.txt").write_text(mr.matrix_text(asm, flat, fmt="%.1f"))
    rc, out, err = run_cli(["mantel", "-f", str(tmp_path / "flat.txt"), gfa])
    assert rc == 0 and out == (mr.HEADER + "\n").encode() and b"a matrix has one value only" in err
    q = mr.random_matrix(6, 1)
    for n in (0, 1, 2):
        got = capi.pan_mantel(ora, q[:n, :n], q[:n, :n], n_perm=5)
        assert mr.same(got, mr.pan_mantel(q[:n, :n], q[:n, :n], 5)) and (got["N"], got["Z"], got["n_ge"], got["n_le"]) == (n, 0, -1, -1)
    const = 7 * (1 - np.eye(6, dtype=np.int64))
    for qx, qy in ((q, const), (const, q), (np.zeros((6, 6), dtype=np.int64), q)):
        got = capi.pan_mantel(ora, qx, qy, n_perm=5)
        assert mr.same(got, mr.pan_mantel(qx, qy, 5)) and got["n_ge"] == -1 and got["Sa"] == int(qx.sum())


def test_pan_mantel(ora):
    """pg_pan_mantel on matrices no fixture has: a = b gives r = 1.0000 and few permutations at or above Z; b = max - a off the diagonal
    gives r = -1.0000; entries of 2^29 - 1 exercise the shifts (s = 7 at N = 300: (2^29 >> 7)^2 300 299 < 2^62 <= (2^29 >> 6)^2 300 299)"""
    from pangene_amd import capi
    q = mr.random_matrix(40, 3)
    got = capi.pan_mantel(ora, q, q, n_perm=200, seed=3)
    assert mr.same(got, mr.pan_mantel(q, q, 200, 3)) and mr.r_text(got) == "1.0000" and got["n_ge"] == 0 and got["n_le"] == 200
    m = int(q.max())
    inv = (m - q) * (1 - np.eye(40, dtype=np.int64))
    got = capi.pan_mantel(ora, q, inv, n_perm=200, seed=3)
    assert mr.same(got, mr.pan_mantel(q, inv, 200, 3)) and mr.r_text(got) == "-1.0000" and got["n_ge"] == 200 and got["n_le"] == 0
    for N, seed in ((7, 1), (33, 2), (300, 3)):
        qx, qy = mr.random_matrix(N, seed, hi=1 << 29), mr.random_matrix(N, seed + 10, hi=1 << 12)
        qx[0, 1] = qx[1, 0] = mr.IN_MAX
        got = capi.pan_mantel(ora, qx, qy, n_perm=20)
        assert mr.same(got, mr.pan_mantel(qx, qy, 20)) and got["sx"] == mr.shift_of(mr.IN_MAX, N) and got["sy"] == 0 and (N != 300 or got["sx"] == 7)
    import torch
    got = capi.pan_mantel(ora, torch.from_numpy(q.astype(np.int32)), torch.from_numpy(inv.astype(np.int32)), n_perm=10)
    assert mr.same(got, mr.pan_mantel(q, inv, 10))


def test_ties_count_in_both(ora):
    """a two-valued pair of matrices: many Z_p equal Z, and each of them counts in n_ge and in n_le"""
    from pangene_amd import capi
    qx, qy = mr.random_matrix(12, 5, hi=2) << 8, mr.random_matrix(12, 6, hi=2) << 8
    got, want = capi.pan_mantel(ora, qx, qy, n_perm=400), mr.pan_mantel(qx, qy, 400)
    assert mr.same(got, want) and got["n_ge"] + got["n_le"] > 400


def test_pan_mantel_refusals(ora):
    from pangene_amd import capi
    q = mr.random_matrix(6, 1)
    for k, v in (((2, 3), 5), ((1, 1), 1), ((4, 0), -1)):
        bad = q.copy()
        bad[k] = v
        if v < 0:
            bad[k[::-1]] = v
        for pair in ((bad, q), (q, bad)):
            with pytest.raises(RuntimeError, match="status -3"):
                capi.pan_mantel(ora, *pair)
    big = q.copy()
    big[2, 3] = big[3, 2] = 1 << 29
    with pytest.raises(RuntimeError, match="status -2"):
        capi.pan_mantel(ora, q, big)
    with pytest.raises(ValueError):
        capi.pan_mantel(ora, q, q[:5, :5])
    o = capi.mantel_opt(ora)
    out = np.zeros(10, dtype=np.int64)
    q32, p32, p64 = np.ascontiguousarray(q, dtype=np.int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    assert ora.pg_pan_mantel(q32.ctypes.data_as(p32), q32.ctypes.data_as(p32), 6, None, out.ctypes.data_as(p64)) == -3
    assert ora.pg_pan_mantel(q32.ctypes.data_as(p32), None, 6, C.byref(o), out.ctypes.data_as(p64)) == -3
    assert ora.pg_pan_mantel(q32.ctypes.data_as(p32), q32.ctypes.data_as(p32), 6, C.byref(o), None) == -3
    assert ora.pg_pan_mantel(q32.ctypes.data_as(p32), q32.ctypes.data_as(p32), -1, C.byref(o), out.ctypes.data_as(p64)) == -3
    o.n_perm = -1
    assert ora.pg_pan_mantel(q32.ctypes.data_as(p32), q32.ctypes.data_as(p32), 6, C.byref(o), out.ctypes.data_as(p64)) == -3
    o = capi.mantel_opt(ora)
    o.y_metric = 1  # shared
    assert ora.pg_pan_mantel(q32.ctypes.data_as(p32), q32.ctypes.data_as(p32), 6, C.byref(o), out.ctypes.data_as(p64)) == -3
    for spec in ("gene", "gene:shared", "walk:diff", ":"):
        with pytest.raises(ValueError):
            capi.mantel_opt(ora, x=spec)


def test_more_assemblies_than_the_limit(ora):
    """N = 16 385: PGA_ERR_RANGE from the host driver too, before the matrices are looked at"""
    from pangene_amd import capi
    n = mr.LIMIT_N + 1
    q = np.zeros((n, n), dtype=np.int32)
    with pytest.raises(RuntimeError, match="status -2"):
        capi.pan_mantel(ora, q, q, n_perm=1)


def test_sizeof_and_defaults(ora):
    from pangene_amd import capi
    import re
    hdr = open(os.path.join(ROOT, "include", "pangene_amd.h")).read()
    assert int(re.search(r"sizeof\(pg_mantel_opt_t\) is (\d+)", hdr).group(1)) == C.sizeof(capi.pg_mantel_opt_t) == 24
    o = capi.pg_mantel_opt_t()
    C.memset(C.byref(o), 0xff, C.sizeof(o))
    ora.pg_mantel_opt_init(C.byref(o))
    assert (o.x_type, o.x_metric, o.y_type, o.y_metric, o.n_perm, o.seed) == (0, 0, 1, 0, 1000, 11)


def test_usage_text(built):
    rc, out, err = run_cli([])
    text = out + err
    for word in (b"--mantel[=FILE]", b"--mantel-x=STR", b"--mantel-y=STR", b"--mantel-perm=INT", b"--mantel-seed=INT",
                 b"pangene mantel [-x SPEC] [-y SPEC | -f FILE] [-n INT] [-s INT] <in.gfa>"):
        assert word in text, word
    rc, out, err = run_cli(["mantel"])
    assert rc == 0 and out.startswith(b"Usage: pangene mantel") and all(w in out for w in (b"-x SPEC", b"-y SPEC", b"-f FILE", b"-n INT", b"-s INT", b"[1000]", b"[11]"))


def test_in_memory_route(built, tmp_path):
    """`pangene --mantel *.paf` prints what `pangene mantel` prints for the GFA of the same run, with a matrix file too"""
    pafs = pafs_of("human8")
    rc, gfa, _ = run_cli(pafs)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    rc, table, _ = run_cli(["dist", "-t", "adj", "-m", "diff", str(tmp_path / "g.gfa")])
    assert rc == 0
    (tmp_path / "d.tsv").write_bytes(table)
    for mem, fil in ((["--mantel"], []), (["--mantel", "--mantel-x=adj:diff", "--mantel-y=gene:diff", "--mantel-perm=77", "--mantel-seed=4"],
                                          ["-x", "adj:diff", "-y", "gene:diff", "-n", "77", "-s", "4"]),
                     (["--mantel=" + str(tmp_path / "d.tsv"), "--mantel-perm=50"], ["-f", str(tmp_path / "d.tsv"), "-n", "50"])):
        rc1, a, _ = run_cli(mem + pafs)
        rc2, b, _ = run_cli(["mantel"] + fil + [str(tmp_path / "g.gfa")])
        assert rc1 == 0 and rc2 == 0 and a == b and mr.parse(a) is not None, mem


def test_capi_run(ora):
    from pangene_amd import capi
    pafs = pafs_of("human8")
    a = capi.run(ora, pafs, ["--mantel", "--mantel-perm=20"])
    rc, b, _ = run_cli(["--mantel", "--mantel-perm=20"] + pafs)
    assert rc == 0 and a == b and mr.parse(a)["N"] == 8
    for argv in (["--mantel-perm=20"], ["--mantel", "--cluster=2"], ["--mantel", "--mantel-x=gene"], ["--mantel=x.tsv", "--mantel-y=adj:diff"], ["--mantel-bogus=1"]):
        with pytest.raises(ValueError):
            capi.run(ora, pafs, argv)
