"""Pangenome accumulation curves (`pangene curves`, `pangene --curves`, pg_pan_curves) through the checker build: the host driver linked
against the oracle backend, whose table has no pan_curves entry, so the counting runs as the plain host loops of curves.cpp.  Everything
is compared with the numpy restatement of tests/support/curves_ref.py (cumulative presence over the columns of each order)."""
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
import curves_ref as cr  # noqa: E402

GFAS = sorted(os.path.join(GOLD, f) for f in os.listdir(GOLD) if f.endswith(".gfa.gz")) + \
    sorted(os.path.join(GOLD, "bubble", f) for f in os.listdir(os.path.join(GOLD, "bubble")) if f.endswith(".gfa"))


def run_cli(args, exe=CLI):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    return oracle_host.load()


def test_hand_worked_example(ora):
    """G = 4, A = 5 under the input order: a core gene, a gene of column 0 only, one of columns 1 and 3, one of column 4"""
    from pangene_amd import capi
    P = np.array([[1, 1, 1, 1, 1], [1, 0, 0, 0, 0], [0, 1, 0, 1, 0], [0, 0, 0, 0, 1]], dtype=bool)
    got = capi.pan_curves(ora, P, n_perm=1)
    assert got.shape == (4, 1, 5)
    assert got[0, 0].tolist() == [2, 3, 3, 3, 4]  # pan
    assert got[1, 0].tolist() == [2, 1, 1, 1, 1]  # core
    assert got[2, 0].tolist() == [2, 1, 0, 0, 1]  # new
    assert got[3, 0].tolist() == [2, 2, 2, 1, 2]  # unique


def test_generator_is_the_spec():
    """order 0 is the identity, the others are permutations that depend on the seed and the order's number"""
    assert cr.order(7, 0) == list(range(7))
    assert sorted(cr.order(50, 3)) == list(range(50))
    assert cr.order(50, 3) != cr.order(50, 4) and cr.order(50, 3, 11) != cr.order(50, 3, 12)
    assert cr.order(1, 5) == [0] and cr.order(0, 5) == []


SHAPES = [(0, 0, 3), (0, 6, 2), (5, 0, 2), (1, 1, 1), (9, 1, 4), (13, 2, 3), (40, 31, 1), (40, 32, 5), (40, 33, 5), (300, 50, 7),
          (120, 97, 6), (8, 400, 3)]


@pytest.mark.parametrize("G,A,n", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_pan_curves_matches_restatement(ora, G, A, n):
    from pangene_amd import capi
    rng = np.random.default_rng(G * 1000 + A)
    P = rng.random((G, A)) < rng.random((G, 1)) ** 2 if G else np.zeros((0, A), dtype=bool)
    got = capi.pan_curves(ora, P, n_perm=n, seed=5)
    assert got.shape == (4, n, A)
    assert np.array_equal(got, cr.curves(P, n, 5))


def test_u_shaped_matrix(ora):
    from pangene_amd import capi
    P = cr.u_shaped(500, 150, 3)
    assert np.array_equal(capi.pan_curves(ora, P, n_perm=4, seed=9), cr.curves(P, 4, 9))


def test_torch_input(ora):
    torch = pytest.importorskip("torch")
    from pangene_amd import capi
    P = cr.u_shaped(60, 20, 4)
    assert np.array_equal(capi.pan_curves(ora, torch.from_numpy(P), n_perm=3), capi.pan_curves(ora, P, n_perm=3))


def check_invariants(out, G):
    pan, core, new, uniq = out.astype(np.int64)
    A = out.shape[2]
    if A == 0:
        return
    assert (np.diff(pan, axis=1) >= 0).all() and (np.diff(core, axis=1) <= 0).all()
    assert (new.sum(1) == pan[:, -1]).all()
    assert (uniq <= pan).all() and (core <= pan).all() and (pan <= G).all() and (out >= 0).all()
    assert (pan[:, 0] == core[:, 0]).all() and (pan[:, 0] == uniq[:, 0]).all()


def test_invariants(ora):
    from pangene_amd import capi
    for G, A, seed in [(400, 60, 1), (50, 3, 2), (10, 200, 3)]:
        P = cr.u_shaped(G, A, seed)
        check_invariants(capi.pan_curves(ora, P, n_perm=6, seed=seed), G)


@pytest.mark.parametrize("gfa", GFAS, ids=[os.path.relpath(g, GOLD) for g in GFAS])
def test_file_route_equals_restatement_of_gfa2matrix(built, gfa):
    rc, mat, _ = run_cli(["gfa2matrix", gfa])
    assert rc == 0
    P = cr.parse_matrix(mat)
    rc, out, _ = run_cli(["curves", gfa])
    assert rc == 0
    want = cr.curves(P, 10, 11)
    assert out == cr.text(want)
    check_invariants(want, P.shape[0])
    rc, out, _ = run_cli(["curves", "-n", "3", "-s", "77", gfa])
    assert rc == 0 and out == cr.text(cr.curves(P, 3, 77))


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", ["C4", "bact20", "fuzz0"])
def test_in_memory_route_equals_file_route(built, tmp_path, name):
    """`pangene --curves *.paf` (pg_write_curves on the graph in memory) prints what `pangene *.paf > g.gfa; pangene curves g.gfa` prints"""
    files = _paf_dir(name)
    rc, gfa, _ = run_cli(files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    rc1, a, _ = run_cli(["--curves=4", "--curves-seed=3"] + files)
    rc2, b, _ = run_cli(["curves", "-n", "4", "-s", "3", str(tmp_path / "g.gfa")])
    assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(b"Stat\tPerm\t1")
    rc, d, _ = run_cli(["--curves"] + files)
    assert rc == 0 and d == run_cli(["curves", str(tmp_path / "g.gfa")])[1]


def test_python_run_equals_command_line(ora):
    from pangene_amd import capi
    files = _paf_dir("C4")
    assert capi.run(ora, files, ["--curves=3"]) == run_cli(["--curves=3"] + files)[1]


def test_refusals(built):
    files = _paf_dir("C4")
    rc, out, err = run_cli(["--gpus", "2", "--curves"] + files)
    assert rc == 1 and out == b"" and b"--curves" in err
    for extra in (["--matrix"], ["--call"], ["--matrix=count"]):
        rc, out, err = run_cli(["--curves"] + extra + files)
        assert rc == 1 and out == b"" and b"--curves" in err
    rc, out, err = run_cli(["curves", "-n", "0", os.path.join(GOLD, "C4.gfa.gz")])
    assert rc == 1 and out == b""


def test_usage_and_missing_file(built, tmp_path):
    rc, out, _ = run_cli(["curves"])
    assert rc == 0 and out.startswith(b"Usage: pangene curves [options] <in.gfa>\n")
    rc, out, _ = run_cli(["curves", str(tmp_path / "none.gfa")])
    assert rc == 1 and out == b""


def test_no_assemblies(built, tmp_path):
    """a GFA without W-lines: genes but no columns, so the rows have no values"""
    g = tmp_path / "s.gfa"
    g.write_text("S\ta\t*\tLN:i:1\nS\tb\t*\tLN:i:1\nL\ta\t+\tb\t+\t0M\n")
    rc, out, _ = run_cli(["curves", "-n", "2", str(g)])
    assert rc == 0 and out == b"Stat\tPerm\npan\t0\npan\t1\ncore\t0\ncore\t1\nnew\t0\nnew\t1\nunique\t0\nunique\t1\n"
