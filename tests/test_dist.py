"""Pairwise distances of the assemblies (`pangene dist`, `pangene --dist`, pg_pan_shared, pg_pan_dist) through the checker build: the
host driver linked against the oracle backend, whose table has no pan_shared entry, so the counting runs as the plain host loops of
dist.cpp.  Everything is compared with the numpy restatement of tests/support/dist_ref.py."""
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

GFAS = sorted(os.path.join(GOLD, f) for f in os.listdir(GOLD) if f.endswith(".gfa.gz")) + \
    sorted(os.path.join(GOLD, "bubble", f) for f in os.listdir(os.path.join(GOLD, "bubble")) if f.endswith(".gfa"))

HAND_GFA = "S\tg1\t*\tLN:i:1\nS\tg2\t*\tLN:i:1\nS\tg3\t*\tLN:i:1\n" \
    "W\ts1\t0\tc1\t0\t3\t>g1>g2>g3\nW\ts2\t0\tc1\t0\t3\t>g1>g2<g3\nW\ts3\t0\tc1\t0\t3\t<g3<g2<g1\n"


def run_cli(args, exe=CLI):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    return oracle_host.load()


def parse_text(b):
    rows = b.decode().rstrip("\n").split("\n")
    body = rows[1:]
    names = [r.split("\t")[0] for r in body]
    vals = [r.split("\t")[1:] for r in body]
    return names, vals


def test_hand_worked_presence(ora):
    """items 0-3: a = {0, 1, 2}, b = {1, 2, 3}, c = {}"""
    from pangene_amd import capi
    P = np.zeros((4, 3), dtype=bool)
    P[[0, 1, 2], 0] = True
    P[[1, 2, 3], 1] = True
    S = capi.pan_shared(ora, P)
    assert S.dtype == np.int32 and S.tolist() == [[3, 2, 0], [2, 3, 0], [0, 0, 0]]
    J = capi.pan_dist(ora, P)
    assert J.dtype == np.float64
    assert "%.6f" % J[0, 1] == "0.500000" and "%.6f" % J[0, 2] == "1.000000" and "%.6f" % J[2, 2] == "0.000000"
    D = capi.pan_dist(ora, P, "diff")
    assert D.dtype == np.int64 and D[0, 1] == 2 and D[0, 2] == 3 and D[2, 2] == 0
    assert capi.pan_dist(ora, P, "shared").tolist() == S.tolist()


def test_hand_written_gfa(built, tmp_path):
    g = tmp_path / "h.gfa"
    g.write_text(HAND_GFA)
    rc, out, _ = run_cli(["dist", str(g)])
    assert rc == 0
    names, vals = parse_text(out)
    assert names == ["s1#0", "s2#0", "s3#0"] and all(v == "0.000000" for r in vals for v in r)
    rc, out, _ = run_cli(["dist", "-t", "adj", str(g)])
    assert rc == 0
    _, vals = parse_text(out)
    assert vals[0][2] == vals[2][0] == "0.000000"  # the reversed walk traverses the same adjacencies
    assert vals[0][1] == "0.666667"  # {g1g2, g2g3} against {g1g2, g2g3'}: 1 shared of 3
    rc, out, _ = run_cli(["dist", "-t", "adj", "-m", "shared", "-p", str(g)])
    assert rc == 0 and out == b"3\ns1#0\t2\t1\t2\ns2#0\t1\t2\t1\ns3#0\t2\t1\t2\n"


SHAPES = [(a, m) for a in (0, 1, 2, 63, 64, 65, 127, 128, 129, 257) for m in (0, 1, 31, 32, 33, 4097)]


@pytest.mark.parametrize("A,M", SHAPES, ids=["A%d-M%d" % s for s in SHAPES])
def test_random_shapes(ora, A, M):
    from pangene_amd import capi
    rng = np.random.default_rng(A * 10007 + M)
    P = rng.random((M, A)) < rng.random((1, A)) if M and A else np.zeros((M, A), dtype=bool)
    S = capi.pan_shared(ora, P)
    want = dr.shared(P)
    assert S.shape == (A, A) and np.array_equal(S, want)
    for m in dr.METRICS:
        got = capi.pan_dist(ora, P, m)
        ref = dr.metric(want, m)
        assert got.dtype == ref.dtype and np.array_equal(got, ref), m


@pytest.mark.parametrize("gfa", GFAS, ids=[os.path.relpath(g, GOLD) for g in GFAS])
def test_fixture_files(built, gfa):
    rc, mat, _ = run_cli(["gfa2matrix", gfa])
    assert rc == 0
    names, P, _ = dr.read_gfa(gfa)
    assert mat.split(b"\n", 1)[0] == ("Gene\t" + "\t".join(names)).encode()  # the columns gfa2matrix prints
    for kind in ("gene", "adj"):
        names, P = dr.presence(gfa, kind)
        S = dr.shared(P)
        for m in dr.METRICS:
            for p in (False, True):
                args = ["dist", "-t", kind, "-m", m] + (["-p"] if p else []) + [gfa]
                rc, out, err = run_cli(args)
                assert rc == 0, err
                assert out == dr.text(names, S, m, p), " ".join(args)


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", ["C4", "bact20", "fuzz0"])
def test_in_memory_route_equals_file_route(built, tmp_path, name):
    """`pangene --dist *.paf` (pg_write_dist on the graph in memory) prints what `pangene *.paf > g.gfa; pangene dist g.gfa` prints"""
    files = _paf_dir(name)
    rc, gfa, _ = run_cli(files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    for kind in ("gene", "adj"):
        rc1, a, _ = run_cli(["--dist=" + kind, "--dist-metric=diff"] + files)
        rc2, b, _ = run_cli(["dist", "-t", kind, "-m", "diff", str(tmp_path / "g.gfa")])
        assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(b"Asm\t"), kind
    rc, d, _ = run_cli(["--dist"] + files)
    assert rc == 0 and d == run_cli(["dist", str(tmp_path / "g.gfa")])[1]


def test_python_run_equals_command_line(ora):
    from pangene_amd import capi
    files = _paf_dir("C4")
    assert capi.run(ora, files, ["--dist=adj"]) == run_cli(["--dist=adj"] + files)[1]


def test_refusals(built):
    files = _paf_dir("C4")
    rc, out, err = run_cli(["--gpus", "2", "--dist"] + files)
    assert rc == 1 and out == b"" and b"--dist" in err
    for extra in (["--matrix"], ["--call"], ["--matrix=count"], ["--curves"]):
        rc, out, err = run_cli(["--dist"] + extra + files)
        assert rc == 1 and out == b"" and b"--dist" in err
    for bad in (["--dist=genes"], ["--dist", "--dist-metric=cosine"]):
        rc, out, err = run_cli(bad + files)
        assert rc == 1 and out == b""
    g = os.path.join(GOLD, "C4.gfa.gz")
    for bad in (["-t", "x"], ["-m", "cosine"]):
        rc, out, _ = run_cli(["dist"] + bad + [g])
        assert rc == 1 and out == b""


def test_usage_and_missing_file(built, tmp_path):
    rc, out, _ = run_cli(["dist"])
    assert rc == 0 and out.startswith(b"Usage: pangene dist [options] <in.gfa>\n")
    rc, out, _ = run_cli(["dist", str(tmp_path / "none.gfa")])
    assert rc == 1 and out == b""
    rc, _, err = run_cli([])
    assert b"pangene dist [-t gene|adj]" in err and b"--dist[=STR]" in err


def test_no_assemblies(built, tmp_path):
    g = tmp_path / "s.gfa"
    g.write_text("S\ta\t*\tLN:i:1\nS\tb\t*\tLN:i:1\n")
    rc, out, _ = run_cli(["dist", str(g)])
    assert rc == 0 and out == b"Asm\n"
    rc, out, _ = run_cli(["dist", "-p", str(g)])
    assert rc == 0 and out == b"0\n"


def test_torch_input(ora):
    torch = pytest.importorskip("torch")
    from pangene_amd import capi
    P = np.random.default_rng(4).random((300, 40)) < 0.3
    assert np.array_equal(capi.pan_shared(ora, torch.from_numpy(P)), capi.pan_shared(ora, P))
    assert np.array_equal(capi.pan_dist(ora, torch.from_numpy(P).to(torch.uint8), "diff"), capi.pan_dist(ora, P, "diff"))
