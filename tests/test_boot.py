"""Bootstrap support of the trees (`pangene tree -b`, `pangene --tree --tree-boot`, pg_pan_boot, pg_pan_boot_records) through the checker
build: the host driver linked against the oracle backend, whose table has no pan_boot entry, so every replicate runs as the plain loops
of tree.cpp.  Everything is compared with the numpy restatement of tests/support/boot_ref.py."""
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
import boot_ref as br  # noqa: E402
import dist_ref as dr  # noqa: E402
import tree_ref as tr  # noqa: E402

GFAS = sorted(os.path.join(GOLD, f) for f in os.listdir(GOLD) if f.endswith(".gfa.gz")) + \
    sorted(os.path.join(GOLD, "bubble", f) for f in os.listdir(os.path.join(GOLD, "bubble")) if f.endswith(".gfa"))
ROUTES = (("gene", "jaccard", "nj"), ("adj", "diff", "upgma"))


def run_cli(args, exe=CLI):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    return oracle_host.load()


def write_gfa(P, path):
    """a GFA whose gene presence matrix is P (M, A): one segment per item, one walk per assembly"""
    M, A = P.shape
    lines = ["S\tg%d\t*\tLN:i:1" % m for m in range(M)]
    for a in range(A):
        steps = "".join(">g%d" % m for m in range(M) if P[m, a])
        lines.append("W\ts%d\t0\tc\t0\t%d\t%s" % (a, max(int(P[:, a].sum()), 1), steps or "*"))
    path.write_text("\n".join(lines) + "\n")
    return str(path)


@pytest.mark.parametrize("gfa", GFAS, ids=[os.path.relpath(g, GOLD) for g in GFAS])
def test_fixture_files(built, gfa):
    for kind, metric, method in ROUTES:
        names, P = dr.presence(gfa, kind)
        args = ["tree", "-t", kind, "-m", metric, "-a", method, "-b", "5", "-s", "7", gfa]
        rc, out, err = run_cli(args)
        assert rc == 0, err
        assert out == br.text(names, P, metric, method, 5, 7), " ".join(args)
        rc, out0, _ = run_cli(["tree", "-t", kind, "-m", metric, "-a", method, "-b", "0", "-s", "7", gfa])
        assert rc == 0 and out0 == tr.text(names, dr.shared(P), metric, method)  # -b 0: the plain tree, byte for byte


# (A, method) -> (items, seed, share of exact copies): lineage-structured matrices whose replicates are full of tied minima
CASES = {
    (3, "nj"): (40, 1, 0.5), (3, "upgma"): (40, 2, 0.5), (4, "nj"): (40, 1, 0.5), (4, "upgma"): (40, 2, 0.5),
    (5, "nj"): (40, 1, 0.5), (5, "upgma"): (40, 2, 0.5), (17, "nj"): (200, 1, 0.3), (17, "upgma"): (200, 1, 0.3),
    (64, "nj"): (500, 1, 0.15), (64, "upgma"): (500, 1, 0.15), (65, "nj"): (500, 1, 0.15), (65, "upgma"): (500, 1, 0.15),
}


@pytest.mark.parametrize("A,method", sorted(CASES), ids=["A%d-%s" % c for c in sorted(CASES)])
def test_replicates_and_support_against_the_restatement(ora, A, method):
    from pangene_amd import capi
    M, seed, dup = CASES[(A, method)]
    P = tr.lineage_presence(M, A, seed, dup=dup)
    metric = "jaccard" if A % 2 else "diff"
    stats = {}
    want = br.records(P, metric, method, 7, 1, 3, stats)
    if not (A == 3 and method == "nj"):  # (three leaves under nj: the closing record alone, no minimum is ever taken)
        assert stats["n_tied"] >= 1, "no replicate has a tied minimum: pick another seed"
    got = capi.pan_boot_records(ora, P, metric, method, seed=7, first=1, n=3)
    assert got.dtype == np.int64 and got.shape == want.shape and np.array_equal(got, want)
    rec, F, count = capi.pan_boot(ora, P, metric, method, n_boot=3, seed=7)
    rec_w, F_w, count_w = br.support(P, metric, method, 3, 7)
    assert F == F_w and np.array_equal(rec, rec_w) and count.dtype == np.int32 and np.array_equal(count, count_w)
    assert np.array_equal(rec, capi.pan_tree(ora, P, metric, method)[0])


def test_exact_properties(ora):
    from pangene_amd import capi
    P = tr.lineage_presence(120, 9, 3, dup=0.2)
    B = 6
    for metric in tr.METRICS:
        for method in tr.METHODS:
            rec, _, count = capi.pan_boot(ora, P, metric, method, n_boot=B, seed=5)
            assert count[-1] == B and count.min() >= 0 and count.max() <= B
            # replicate b is the same whichever chunk it is in
            whole = capi.pan_boot_records(ora, P, metric, method, seed=5, first=1, n=B)
            for k in range(B):
                assert np.array_equal(capi.pan_boot_records(ora, P, metric, method, seed=5, first=1 + k, n=1)[0], whole[k])
            assert np.array_equal(capi.pan_boot_records(ora, P, metric, method, seed=5, first=3, n=2), whole[2:4])
            assert capi.pan_boot_records(ora, P, metric, method, seed=5, first=4, n=0).shape == (0, len(rec), 6)
            assert not np.array_equal(capi.pan_boot_records(ora, P, metric, method, seed=6, first=1, n=1)[0], whole[0])  # the seed matters
            # one item: every replicate draws it M = 1 times and is the reference itself
            one = P[:1]
            rec1, _, count1 = capi.pan_boot(ora, one, metric, method, n_boot=B, seed=5)
            assert count1.tolist() == [B] * len(rec1)
            # no item: no draws, every replicate equals the reference tree
            none = P[:0]
            ref0 = capi.pan_tree(ora, none, metric, method)[0]
            assert np.array_equal(capi.pan_boot_records(ora, none, metric, method, seed=5, first=1, n=2), np.stack([ref0, ref0]))
            assert capi.pan_boot(ora, none, metric, method, n_boot=B, seed=5)[2].tolist() == [B] * len(ref0)
            # no replicates: nothing is supported, and the closing entry is B = 0
            assert capi.pan_boot(ora, P, metric, method, n_boot=0, seed=5)[2].tolist() == [0] * len(rec)


def test_argument_and_range_refusals(ora, built):
    from pangene_amd import capi
    P = tr.lineage_presence(40, 5, 1)
    with pytest.raises(RuntimeError, match="status -3"):  # PGA_ERR_ARG
        capi.pan_boot(ora, P, n_boot=-1)
    with pytest.raises(RuntimeError, match="status -3"):
        capi.pan_boot_records(ora, P, first=0, n=1)
    with pytest.raises(RuntimeError, match="status -3"):
        capi.pan_boot_records(ora, P, first=1, n=-1)
    with pytest.raises(RuntimeError, match="status -3"):
        capi.pan_boot_records(ora, P, first=2 ** 31 - 1, n=2)
    with pytest.raises(RuntimeError, match="status -3"):
        capi.pan_boot(ora, P[:, :2], n_boot=2)  # fewer than three assemblies
    with pytest.raises(ValueError):
        capi.pan_boot(ora, P, "shared")
    with pytest.raises(ValueError):
        capi.pan_boot_records(ora, P, "shared")
    with pytest.raises(ValueError):
        capi.tree_opt(ora, n_boot=-1)
    with pytest.raises(RuntimeError, match="status -2"):  # PGA_ERR_RANGE: more assemblies than a label holds
        capi.pan_boot_records(ora, np.ones((1, 65536), dtype=bool), first=1, n=1)
    g = os.path.join(GOLD, "C4.gfa.gz")
    for bad in (["-b", "-1"], ["-b", "x"], ["-b", "2147483648"]):
        rc, out, err = run_cli(["tree"] + bad + [g])
        assert rc == 1 and out == b"" and b"-b" in err
    files = _paf_dir("C4")
    rc, out, err = run_cli(["--tree", "--tree-boot=-1"] + files)
    assert rc == 1 and out == b"" and b"--tree-boot" in err
    rc, out, err = run_cli(["--gpus", "2", "--tree", "--tree-boot=4"] + files)
    assert rc == 1 and out == b"" and b"--tree" in err


def test_seed_is_validated_alike_on_both_fronts(built):
    """-s / --tree-seed take a whole number in [0, 2^32 - 1] and nothing else, on the command line and in capi's argument reader"""
    from pangene_amd import capi
    g = os.path.join(GOLD, "C4.gfa.gz")
    files = _paf_dir("C4")
    for bad in ("x", "-1", "4294967296", "7x", "", " 7", "99999999999999999999999"):
        rc, out, err = run_cli(["tree", "-b", "2", "-s", bad, g])
        assert rc == 1 and out == b"" and b"-s" in err, bad
        rc, out, err = run_cli(["--tree", "--tree-boot=2", "--tree-seed=" + bad] + files)
        assert rc == 1 and out == b"" and b"--tree-seed" in err, bad
        with pytest.raises(ValueError):
            capi._tree_boot_args(["--tree-seed=" + bad])
    rc, top, _ = run_cli(["tree", "-b", "2", "-s", "4294967295", g])
    rc2, top2, _ = run_cli(["--tree", "--tree-boot=2", "--tree-seed=4294967295"] + files)
    assert rc == 0 and rc2 == 0 and top.endswith(b";\n") and top2.endswith(b";\n")
    assert capi._tree_boot_args(["--tree-boot=2", "--tree-seed=4294967295"]) == (2, 4294967295)


def test_options_struct(ora):
    from pangene_amd import capi
    o = capi.pg_tree_opt_t()
    o.n_boot, o.seed = 7, 7
    ora.pg_tree_opt_init(C.byref(o))
    assert (o.n_boot, o.seed) == (0, 0) and C.sizeof(o) == 20
    o = capi.tree_opt(ora, "adj", "diff", "upgma", n_boot=5, seed=2 ** 32 + 9)
    assert (o.type, o.metric, o.method, o.n_boot, o.seed) == (1, 2, 1, 5, 9)


def _mixed(seed):
    """six assemblies over 24 items, two noisy lineages: splits with little support"""
    rng = np.random.default_rng(seed)
    base = rng.random((24, 2)) < 0.5
    return np.stack([base[:, rng.integers(0, 2)] ^ (rng.random(24) < 0.25) for _ in range(6)], axis=1)


# count / B = 1/8 (12.5 -> 13), 1/2 (50) and 199/200 (99.5 -> 100): (seed of the matrix and of the draws, B, count, label)
@pytest.mark.parametrize("seed,B,cnt,label", [(3, 8, 1, b")13:"), (0, 2, 1, b")50:"), (340, 200, 199, b")100:")], ids=["1of8", "1of2", "199of200"])
def test_percent_rounds_half_up(ora, tmp_path, seed, B, cnt, label):
    from pangene_amd import capi
    assert (br.percent(1, 8), br.percent(1, 2), br.percent(199, 200), br.percent(0, 7), br.percent(7, 7)) == (13, 50, 100, 0, 100)
    g = write_gfa(_mixed(seed), tmp_path / "m.gfa")
    names, P = dr.presence(g, "gene")
    rec, F, count = br.support(P, "jaccard", "nj", B, seed)
    assert cnt in count[:-1].tolist(), "the restatement no longer meets this ratio: pick another seed"
    assert np.array_equal(capi.pan_boot(ora, P, "jaccard", "nj", n_boot=B, seed=seed)[2], count)
    rc, out, err = run_cli(["tree", "-b", str(B), "-s", str(seed), g])
    assert rc == 0, err
    assert out == br.text(names, P, "jaccard", "nj", B, seed) and label in out
    assert out.count(b")") == len(names) - 2 and out.endswith(b");\n")  # the trifurcation carries no label


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", ["C4", "bact20"])
def test_in_memory_route_equals_file_route(built, tmp_path, name):
    files = _paf_dir(name)
    rc, gfa, _ = run_cli(files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    for kind, metric, method in ROUTES:
        rc1, a, _ = run_cli(["--tree=" + kind, "--tree-metric=" + metric, "--tree-method=" + method, "--tree-boot=4", "--tree-seed=3"] + files)
        rc2, b, _ = run_cli(["tree", "-t", kind, "-m", metric, "-a", method, "-b", "4", "-s", "3", str(tmp_path / "g.gfa")])
        names, P = dr.presence(str(tmp_path / "g.gfa"), kind)
        assert rc1 == 0 and rc2 == 0 and a == b == br.text(names, P, metric, method, 4, 3), kind
    rc, plain, _ = run_cli(["--tree", "--tree-boot=0"] + files)
    assert rc == 0 and plain == run_cli(["--tree"] + files)[1]


def test_python_run_equals_command_line(ora):
    from pangene_amd import capi
    files = _paf_dir("C4")
    args = ["--tree=adj", "--tree-method=upgma", "--tree-boot=3", "--tree-seed=2"]
    out = capi.run(ora, files, args)
    assert out == run_cli(args + files)[1] and out != capi.run(ora, files, args[:2])


def test_usage(built):
    rc, out, _ = run_cli(["tree"])
    assert rc == 0 and b"-b INT" in out and b"-s INT" in out and b"bootstrap" in out
    rc, _, err = run_cli([])
    assert b"[-b INT] [-s INT] <in.gfa>" in err and b"--tree-boot=INT" in err and b"--tree-seed=INT" in err
