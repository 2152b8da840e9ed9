"""The lineage-aware trait test (`pangene trait -L`, `pangene --trait --trait-lineage`, pg_pan_pairs) through the checker build: the host
driver linked against the oracle backend, whose table has no pan_pairs entry, so the tree dynamic programmes run as the plain loops of
trait.cpp.  The counts are compared with the restatement of tests/support/pairs_ref.py (None for infeasible, tuples for values) and, up
to 8 leaves, with its brute force over every set of contrasting leaf pairs; the printed columns with the restatement's bytes (exact
big-integer binomial sums, %.3e).  The eleven columns `pangene trait` printed before are held to the bytes of the same command without
-L, which tests/test_trait.py checks."""
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
import assoc_ref as ar  # noqa: E402
import dist_ref  # noqa: E402
import pairs_ref as pr  # noqa: E402
import trait_ref as tr  # noqa: E402
import tree_ref  # noqa: E402

GFAS = sorted(os.path.join(GOLD, f) for f in os.listdir(GOLD) if f.endswith(".gfa.gz"))
HEADER = (tr.HEADER + "\t" + pr.COLUMNS + "\n").encode()
METHODS = ("nj", "upgma")


def run_cli(args, exe=CLI):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    return oracle_host.load()


def random_records(rng, A, method):
    """records of a random tree over A >= 3 leaves: any two live slots are joined, in either order"""
    live, rec = list(range(A)), []
    while len(live) > (3 if method == "nj" else 1):
        i, j = (int(v) for v in rng.choice(live, size=2, replace=False))
        rec.append((i, j, 0, 0, 0, len(live)))
        live.remove(j)
    if method == "nj":
        x, y, z = (int(v) for v in rng.permutation(live))
        rec.append((x, y, z, 0, 0, 0))
    return np.array(rec, dtype=np.int64).reshape(-1, 6)


def random_labels(rng, T, A):
    """(T, A) int8 with missing values; the last row has none missing"""
    L = rng.integers(0, 2, size=(T, A)).astype(np.int8)
    L[rng.random((T, A)) < 0.25] = -1
    L[-1] = rng.integers(0, 2, size=A)
    return L


def shape_of(kids, A):
    """the shape of a tree, leaves unlabelled: a canonical nested tuple"""
    node = [()] * A
    for a, b in kids:
        node.append(tuple(sorted((node[a], node[b]))))
    return node[-1]


@pytest.mark.parametrize("A", range(3, 9))
def test_brute_force_restatement_and_library_agree(ora, A):
    """every tree shape random records give for A leaves, random genes, labels and missing values: brute force == restatement == pg_pan_pairs"""
    from pangene_amd import capi
    rng = np.random.default_rng(100 + A)
    shapes = {m: set() for m in METHODS}
    n_pairs = 0
    for it in range(40):
        for method in METHODS:
            rec = random_records(rng, A, method)
            kids = pr.tree(rec, A, method)
            shapes[method].add(shape_of(kids, A))
            P = rng.random((6, A)) < 0.5
            L = random_labels(rng, 3, A)
            want = pr.counts(P, L, rec, method)
            got = capi.pan_pairs(ora, P, L, rec, method)
            for key in ("pairs", "supp", "opp"):
                assert got[key].dtype == np.int32 and np.array_equal(got[key], want[key]), (key, method, rec.tolist())
            for ti in range(3):
                for g in range(6):
                    b = pr.brute(kids, pr.types(P[g], L[ti]))
                    assert b == (want["pairs"][ti, g], want["supp"][ti, g], want["opp"][ti, g]), (method, rec.tolist(), P[g], L[ti])
                    n_pairs += b[0]
    # rooted shapes of A leaves: 1, 2, 3, 6, 11, 23 (Wedderburn-Etherington); the draws reach them all up to 6 leaves and most beyond
    assert len(shapes["upgma"]) >= {3: 1, 4: 2, 5: 3, 6: 6, 7: 9, 8: 14}[A] and n_pairs > 0


@pytest.mark.parametrize("A", (3, 4, 6, 8))
def test_trifurcation_reading_changes_nothing(ora, A):
    """(x, y, z) read as ((x, y), z), ((x, z), y) or ((y, z), x): the same counts, in the restatement and through the library"""
    from pangene_amd import capi
    rng = np.random.default_rng(7 * A)
    for it in range(20):
        rec = random_records(rng, A, "nj")
        P = rng.random((8, A)) < 0.5
        L = random_labels(rng, 3, A)
        first = pr.counts(P, L, rec, "nj", 0)
        for k in (1, 2):
            other = pr.counts(P, L, rec, "nj", k)
            assert all(np.array_equal(first[key], other[key]) for key in first)
        x, y, z = rec[-1, :3]
        for perm in ((x, z, y), (y, z, x), (z, y, x)):
            r2 = rec.copy()
            r2[-1, :3] = perm
            got = capi.pan_pairs(ora, P, L, r2, "nj")
            assert all(np.array_equal(first[key], got[key]) for key in first)


def pruned(rec, A, keep):
    """upgma-shaped records with the leaves outside `keep` cut off: (records over the kept leaves renumbered 0 .., kept leaves)"""
    kept = [x for x in range(A) if keep[x]]
    slot = [kept.index(x) if keep[x] else None for x in range(A)]
    out = []
    for i, j in rec[:, :2].tolist():
        if slot[i] is not None and slot[j] is not None:
            out.append((slot[i], slot[j], 0, 0, 0, 0))
        elif slot[j] is not None:
            slot[i] = slot[j]
        slot[j] = None
    return np.array(out, dtype=np.int64).reshape(-1, 6), kept


@pytest.mark.parametrize("A", (4, 7, 8, 30))
def test_missing_leaves_equal_the_pruned_tree(ora, A):
    from pangene_amd import capi
    rng = np.random.default_rng(A)
    for it in range(15):
        rec = random_records(rng, A, "upgma")
        P = rng.random((10, A)) < 0.5
        L = rng.integers(0, 2, size=(1, A)).astype(np.int8)
        L[0, rng.random(A) < 0.4] = -1
        rec2, kept = pruned(rec, A, L[0] >= 0)
        whole = capi.pan_pairs(ora, P, L, rec, "upgma")
        small = capi.pan_pairs(ora, P[:, kept], L[:, kept], rec2 if len(kept) >= 3 else None, "upgma")
        want = pr.counts(P[:, kept], L[:, kept], rec2, "upgma")
        for key in whole:
            assert np.array_equal(whole[key], small[key]) and np.array_equal(whole[key], want[key]), (key, rec.tolist(), L.tolist())


def test_trees_of_the_library_and_few_leaves(ora):
    """the records pg_pan_tree returns, both methods, 40 leaves; and one and two leaves, which need no records"""
    from pangene_amd import capi
    P = tree_ref.lineage_presence(120, 40, 3, flip=0.1)
    L = random_labels(np.random.default_rng(1), 4, 40)
    L[0] = -1  # a row without any value
    L[1] = 1   # and a constant one
    for method in METHODS:
        rec, _ = capi.pan_tree(ora, P, "jaccard", method)
        assert np.array_equal(rec, pr.records(P, method))
        got, want = capi.pan_pairs(ora, P, L, rec, method), pr.counts(P, L, rec, method)
        assert all(np.array_equal(got[k], want[k]) for k in got)
        assert not got["pairs"][:2].any() and got["pairs"][2:].max() >= 5
    for A in (1, 2):
        got, want = capi.pan_pairs(ora, P[:, :A], L[:, :A], None, "nj"), pr.counts(P[:, :A], L[:, :A], None, "nj")
        assert all(np.array_equal(got[k], want[k]) for k in got)
    two = capi.pan_pairs(ora, np.array([[1, 0], [1, 1], [0, 1]], dtype=bool), np.array([1, 0]), None, "upgma")
    assert (two["pairs"].tolist(), two["supp"].tolist(), two["opp"].tolist()) == ([[1, 0, 1]], [[1, 0, 0]], [[0, 0, 1]])
    assert capi.pan_pairs(ora, P[:0], L, pr.records(P, "nj"), "nj")["pairs"].shape == (4, 0)


def test_arguments(ora):
    from pangene_amd import capi
    P = tree_ref.lineage_presence(20, 6, 1)
    L = np.ones((1, 6), dtype=np.int8)
    rec = pr.records(P, "upgma")
    o = capi.trait_opt(ora)
    assert o.lineage == 0 and C.sizeof(o) == 32 and capi.trait_opt(ora, lineage="upgma").lineage == 2
    with pytest.raises(ValueError):
        capi.trait_opt(ora, lineage="ml")
    with pytest.raises(ValueError):
        capi.pan_pairs(ora, P, L, rec[:-1], "upgma")  # a record short
    with pytest.raises(ValueError):
        capi.pan_pairs(ora, P, L[:, :5], rec, "upgma")
    for bad in ((0, 0), (0, 6), (-1, 2)):  # a slot joined with itself, out of range
        r2 = rec.copy()
        r2[0, :2] = bad
        with pytest.raises(RuntimeError, match="status -3"):
            capi.pan_pairs(ora, P, L, r2, "upgma")
    r2 = rec.copy()
    r2[-1, :2] = r2[0, :2]  # a slot that has retired
    with pytest.raises(RuntimeError, match="status -3"):
        capi.pan_pairs(ora, P, L, r2, "upgma")
    wide = np.zeros((1, 65536), dtype=bool)
    with pytest.raises(RuntimeError, match="status -2"):
        capi.pan_pairs(ora, wide, np.zeros(65536, dtype=np.int8), pr.caterpillar_records(65536), "upgma")


def read_traits(path, asm):
    """a trait file -> (names, labels (T, A) int8 with -1 = missing)"""
    with open(path) as f:
        lines = [l.rstrip("\n") for l in f if l.strip() and not l.startswith("#")]
    names = lines[0].split("\t")[1:]
    L = np.full((len(names), len(asm)), -1, dtype=np.int8)
    for l in lines[1:]:
        f = l.split("\t")
        for k, v in enumerate(f[1:]):
            L[k, asm.index(f[0])] = -1 if v in ("NA", "") else int(v)
    return names, L


def fixture_traits(gfa, asm, tmp_path):
    """the trait file of the fixture under tests/golden/trait, or -- for a fixture without one -- three made-up traits"""
    path = os.path.join(GOLD, "trait", os.path.basename(gfa).replace(".gfa.gz", ".tsv"))
    if os.path.exists(path):
        names, L = read_traits(path, asm)
        return path, names, L
    rng = np.random.default_rng(len(asm))
    names, L = ["even", "gaps", "rare"], random_labels(rng, 3, len(asm))
    L[2] = 0
    L[2, : min(2, len(asm))] = 1
    f = tmp_path / "traits.tsv"
    f.write_text(tr.trait_file(asm, names, L))
    return str(f), names, L


def check_table(out, plain, want):
    """the lines of -L: the line without -L, then the restatement's five columns"""
    lines, before = out.split(b"\n"), plain.split(b"\n")
    assert lines[0] + b"\n" == HEADER and before[0] == tr.HEADER.encode() and len(lines) == len(before) and lines[-1] == b""
    for l, p in zip(lines[1:-1], before[1:-1]):
        f = l.decode().split("\t")
        assert len(f) == 16 and "\t".join(f[:11]).encode() == p
        assert "\t".join(f[11:]) == want[(f[0], f[1])], l


@pytest.mark.parametrize("gfa", GFAS, ids=[os.path.basename(g) for g in GFAS])
def test_fixture_files(built, tmp_path, gfa):
    genes, P = ar.read_gfa(gfa)
    asm = list(dist_ref.presence(gfa, "gene")[0])
    fn, names, L = fixture_traits(gfa, asm, tmp_path)
    rc, plain, err = run_cli(["trait", "-t", fn, "-n", "10", gfa])
    assert rc == 0, err
    for method in METHODS:
        rc, out, err = run_cli(["trait", "-t", fn, "-n", "10", "-L", method, gfa])
        assert rc == 0, err
        check_table(out, plain, pr.table(genes, P, names, L, method))


def test_exact_tail_prints_the_even_digit():
    """2 / 2^7 = 0.015625 sits half way between two printed values: the exact double prints 1.562e-02, a sum that is one unit off does not"""
    assert pr.columns(1, 7, 7, 0).split("\t")[3:] == ["1.562e-02", "1.562e-02"] and pr.columns(-1, 8, 0, 8).split("\t")[3] == "7.812e-03"


def test_planted_clade(built, tmp_path):
    """a gene and a trait that sit in one clade of bact20's tree: Fisher's p is tiny, the tree has one contrasting pair and p_pair = 1"""
    gfa = os.path.join(GOLD, "bact20.gfa.gz")
    genes, P = ar.read_gfa(gfa)
    asm = list(dist_ref.presence(gfa, "gene")[0])
    A = len(asm)
    kids = pr.tree(pr.records(P, "upgma"), A, "upgma")
    below = [{x} for x in range(A)]
    for a, b in kids:
        below.append(below[a] | below[b])
    clade = min((s for s in below if 5 <= len(s) <= A - 5), key=len)
    y = np.array([1 if x in clade else 0 for x in range(A)], dtype=np.int8)
    # the trait is the clade; the clade as a presence row is "gene" 0 of the restatement
    P2 = np.concatenate([y[None, :] != 0, P])
    got = pr.counts(P2[:1], y, pr.records(P, "upgma"), "upgma")
    assert (int(got["pairs"][0, 0]), int(got["supp"][0, 0]), int(got["opp"][0, 0])) == (1, 1, 0)
    assert tr.fisher(A, len(clade), len(clade), len(clade)) < 1e-3 and pr.p2(1, 1) == 1.0
    f = tmp_path / "t.tsv"
    f.write_text(tr.trait_file(asm, ["clade"], y[None, :]))
    rc, out, _ = run_cli(["trait", "-t", str(f), "-n", "0", "-L", "upgma", gfa])
    assert rc == 0
    check_table(out, run_cli(["trait", "-t", str(f), "-n", "0", gfa])[1], pr.table(genes, P, ["clade"], y[None, :], "upgma"))


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


def test_in_memory_route_and_python_run(ora, tmp_path):
    """`pangene --trait=F --trait-lineage=M *.paf` prints what `pangene trait -t F -L M` prints for the GFA of the same run, and capi.run too"""
    from pangene_amd import capi
    files = _paf_dir("C4")
    rc, gfa, _ = run_cli(files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    f = os.path.join(GOLD, "trait", "C4.tsv")
    for method in METHODS:
        rc1, a, _ = run_cli(["--trait=" + f, "--trait-perm=9", "--trait-lineage=" + method] + files)
        rc2, b, _ = run_cli(["trait", "-t", f, "-n", "9", "-L", method, str(tmp_path / "g.gfa")])
        assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(HEADER) and a.count(b"\n") > 1
        assert capi.run(ora, files, ["--trait=" + f, "--trait-perm=9", "--trait-lineage=" + method]) == a
    with pytest.raises(ValueError):
        capi.run(ora, files, ["--trait=" + f, "--trait-lineage=ml"])
    with pytest.raises(ValueError):
        capi.run(ora, files, ["--trait-lineage=nj"])


def test_without_the_option_nothing_changes(built):
    """no -L: the eleven columns and their header, byte for byte the lines that -L extends"""
    gfa, f = os.path.join(GOLD, "human8.gfa.gz"), os.path.join(GOLD, "trait", "human8.tsv")
    rc, plain, _ = run_cli(["trait", "-t", f, "-n", "25", gfa])
    rc2, out, _ = run_cli(["trait", "-t", f, "-n", "25", "-L", "nj", gfa])
    assert rc == 0 and rc2 == 0 and plain.startswith((tr.HEADER + "\n").encode()) and plain.count(b"\n") > 1
    assert [b"\t".join(l.split(b"\t")[:11]) for l in out.split(b"\n")] == plain.split(b"\n")
    assert all(len(l.split(b"\t")) == 11 for l in plain.split(b"\n")[:-1])


def test_refusals_and_usage(built, tmp_path):
    gfa, f = os.path.join(GOLD, "C4.gfa.gz"), os.path.join(GOLD, "trait", "C4.tsv")
    files = _paf_dir("C4")
    for bad in ("ml", "", "NJ", "nj,upgma"):
        rc, out, err = run_cli(["trait", "-t", f, "-L", bad, gfa])
        assert rc == 1 and out == b"" and b"-L" in err, bad
        rc, out, err = run_cli(["--trait=" + f, "--trait-lineage=" + bad] + files)
        assert rc == 1 and out == b"" and b"--trait-lineage" in err, bad
    rc, out, err = run_cli(["--trait-lineage=nj"] + files)
    assert rc == 1 and out == b"" and b"--trait" in err
    rc, out, err = run_cli(["--gpus", "2", "--trait=" + f, "--trait-lineage=nj"] + files)
    assert rc == 1 and out == b"" and b"--trait" in err
    rc, out, _ = run_cli(["trait"])
    assert rc == 0 and b"-L STR" in out and b"p_pair_worst" in out
    rc, _, err = run_cli([])
    assert b"--trait-lineage=STR" in err and b"-L nj|upgma" in err
