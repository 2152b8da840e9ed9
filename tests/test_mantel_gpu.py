"""The Mantel test on the MI355X: the orders of a batch come from k_mantel_order, Z_p of every permutation from the gather kernel k_mantel_z
(the permuted row of b staged in LDS, one 64-bit atomicAdd per workgroup) and the two counts from k_mantel_stat (pga_pan_mantel,
k_mantel.hpp).  The product must print the bytes the checker build prints (oracle backend: no pan_mantel entry, so the host loops of
tree.cpp -- a second implementation; r and the text are host code both share) and the integers of the restatement
(tests/support/mantel_ref.py).  Every step runs in a child process under a timeout of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "mantel_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import dist_ref  # noqa: E402
import mantel_ref as mr  # noqa: E402
import tree_ref  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["C4", "bact20", "human8"]
HEADER = (mr.HEADER + "\n").encode()
OPTION_SETS = [([], "gene:jaccard", "adj:jaccard", {}), (["-x", "adj:diff", "-y", "gene:jaccard"], "adj:diff", "gene:jaccard", {}),
               (["-n", "0"], "gene:jaccard", "adj:jaccard", dict(n_perm=0)), (["-n", "37", "-s", "5"], "gene:jaccard", "adj:jaccard", dict(n_perm=37, seed=5))]


def run(exe, args, timeout=300, env=None):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    if r.returncode != 0:
        sys.stderr.write("%s: exit %d, stderr: %s\n" % (" ".join(args[:4]), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r.returncode, r.stdout, r.stderr


def _fixed(gfa, spec):
    kind, metric = spec.split(":")
    asm, P = dist_ref.presence(gfa, kind)
    return list(asm), tree_ref.fixed(dist_ref.shared(P), metric)[0]


@pytest.mark.parametrize("name", NAMES)
def test_file_route(built, tmp_path, name):
    gfa = os.path.join(GOLD, name + ".gfa.gz")
    q = {spec: _fixed(gfa, spec) for spec in ("gene:jaccard", "adj:jaccard", "adj:diff")}
    for args, x, y, kw in OPTION_SETS:
        cmd = ["mantel"] + args + [gfa]
        rc, out, _ = run(HIP, cmd)
        rc2, out2, _ = run(ORA, cmd)
        assert rc == 0 and rc2 == 0 and out == out2 and out.startswith(HEADER), args
        assert out == mr.text(x, y, q[x][1], q[y][1], **kw), args
    # a matrix file: the adj:diff counts without the last assembly, in PHYLIP
    asm, _ = q["adj:diff"]
    d = dist_ref.metric(dist_ref.shared(dist_ref.presence(gfa, "adj")[1]), "diff")[:-1, :-1]
    (tmp_path / "m.phy").write_text(mr.matrix_text(asm[:-1], d, phylip=True, fmt="%d"))
    cmd = ["mantel", "-f", str(tmp_path / "m.phy"), "-n", "99", gfa]
    rc, out, _ = run(HIP, cmd)
    rc2, out2, _ = run(ORA, cmd)
    fnames, qf, _ = mr.read_matrix(str(tmp_path / "m.phy"))
    a, b = mr.matched(asm, q["gene:jaccard"][1], fnames, qf)
    assert rc == 0 and rc2 == 0 and out == out2 == mr.text("gene:jaccard", "file", a, b, n_perm=99)


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, tmp_path, name):
    """`pangene --mantel *.paf` on the device: what the checker prints, and what `pangene mantel` prints for the GFA of the same run"""
    files = _paf_dir(name)
    rc, gfa, _ = run(HIP, files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    for mem, fil in ((["--mantel"], []),
                     (["--mantel", "--mantel-x=adj:diff", "--mantel-y=gene:diff", "--mantel-perm=333", "--mantel-seed=4"], ["-x", "adj:diff", "-y", "gene:diff", "-n", "333", "-s", "4"])):
        rc1, a, _ = run(HIP, mem + files)
        rc2, b, _ = run(HIP, ["mantel"] + fil + [str(tmp_path / "g.gfa")])
        rc3, c, _ = run(ORA, mem + files)
        assert rc1 == 0 and rc2 == 0 and rc3 == 0 and a == b == c and a.startswith(HEADER) and a.count(b"\n") == 2, mem


def test_refused_when_sharded(built):
    rc, out, err = run(HIP, ["--gpus", "2", "--mantel"] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--mantel" in err


@pytest.mark.parametrize("which", ["maps", "tiles", "classes", "ties", "magnitude", "batches", "limit", "buffers", "range"])
def test_direct_cases(built, which):
    """pga_pan_mantel on matrices no GFA fixture reaches (tests/support/mantel_direct.py): Z, n_ge, n_le and Z_p and the order of every
    permutation of the first batch compared completely with the restatement.  maps: N = 200, every entry of a and of b distinct, 130
    permutations.  tiles: N in {3, 4, 63, 64, 65, 255, 256, 257, 1 023, 1 025} x n in {1, 63, 65}.  classes: the edges of the 16-row block
    of k_mantel_z (N = 16, 17, 18, 33, 34) and of its dynamic LDS beyond 64 KiB (N = 10 912, 10 913).  ties: a constant b gives
    n_ge = n_le = n; a two-valued pair.  magnitude: N = 129, a = b at the largest entry the bound allows (Z above 2^61), and entries of
    2^29 - 1 through pg_pan_mantel (sx = 6).  batches: PANGENE_MANTEL_BATCH=256 in the child, n = 255, 256, 257, 773.  limit: N = 16 384,
    n = 3, the full LDS footprint, against the quadratic form u_o . a . u_o (the one case that takes more than a few seconds: two 1 GiB
    matrices go up).  buffers: growing then shrinking shapes through pg_pan_mantel, cuda tensors, pga_host_trim(0) and again.  range:
    N = 16 385 is PGA_ERR_RANGE before anything is launched."""
    env = dict(os.environ)
    env.pop("PANGENE_MANTEL_BATCH", None)
    if which == "batches":
        env["PANGENE_MANTEL_BATCH"] = "256"
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT, env=env)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]
