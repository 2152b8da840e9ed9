"""Clusters on the MI355X: k-medoids comes from the HIP kernels of k_medoids.hpp (pga_pan_medoids).  The product must print and return
what the numpy restatement (tests/support/cluster_ref.py) and the checker build (oracle backend: no pan_medoids entry, so the host loops
of tree.cpp -- a second implementation; the silhouettes and the text are host code both share) print and return.  Every step runs in a
child process under a timeout of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "cluster_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import cluster_ref as cr  # noqa: E402
import dist_ref as dr  # noqa: E402

pytestmark = pytest.mark.gpu
GFAS = sorted(os.path.join(GOLD, f) for f in os.listdir(GOLD) if f.endswith(".gfa.gz")) + \
    sorted(os.path.join(GOLD, "bubble", f) for f in os.listdir(os.path.join(GOLD, "bubble")) if f.endswith(".gfa"))


def run(exe, args, timeout=120):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write("%s: exit %d, stderr: %s\n" % (" ".join(args[:6]), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("gfa", GFAS, ids=[os.path.relpath(g, GOLD) for g in GFAS])
def test_file_route(built, gfa):
    for kind, metric in (("gene", "jaccard"), ("adj", "diff")):
        names, P = dr.presence(gfa, kind)
        if len(names) < 4:
            pytest.skip("fewer than 4 assemblies")
        rng = "2-%d" % min(4, len(names) - 1)
        args = ["cluster", "-t", kind, "-m", metric, "-k", rng, gfa]
        rc, out, _ = run(HIP, args)
        assert rc == 0 and out == cr.text(names, dr.shared(P), metric, 2, min(4, len(names) - 1)), " ".join(args)
        rc, out2, _ = run(ORA, args)
        assert rc == 0 and out2 == out


def test_a_range_of_k_on_bact20(built):
    """`pangene cluster -k 2-6`: the same bytes from the product, the checker build and the restatement"""
    gfa = os.path.join(GOLD, "bact20.gfa.gz")
    names, P = dr.presence(gfa, "gene")
    rc, out, _ = run(HIP, ["cluster", "-k", "2-6", gfa])
    assert rc == 0 and out == cr.text(names, dr.shared(P), "jaccard", 2, 6)
    assert run(ORA, ["cluster", "-k", "2-6", gfa])[1] == out


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", ["C4", "bact20", "human8"])
def test_in_memory_route(built, tmp_path, name):
    """`pangene --cluster *.paf` on the device: what the checker prints, and what `pangene cluster` prints for the GFA of the same run"""
    files = _paf_dir(name)
    rc, gfa, _ = run(HIP, files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    rng = "2-%d" % min(4, len(dr.presence(str(tmp_path / "g.gfa"), "gene")[0]) - 1)
    for kind, metric in (("gene", "jaccard"), ("adj", "diff")):
        opts = ["--cluster=" + rng, "--cluster-type=" + kind, "--cluster-metric=" + metric]
        rc1, a, _ = run(HIP, opts + files)
        rc2, b, _ = run(HIP, ["cluster", "-t", kind, "-m", metric, "-k", rng, str(tmp_path / "g.gfa")])
        rc3, c, _ = run(ORA, opts + files)
        assert rc1 == 0 and rc2 == 0 and rc3 == 0 and a == b == c and a.startswith(b"#K\t"), kind


def test_refused_when_sharded(built):
    rc, out, err = run(HIP, ["--gpus", "2", "--cluster=2"] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--cluster" in err


@pytest.mark.parametrize("which", ["sizes", "large", "uneven", "ties", "chunks", "cached", "magnitude"])
def test_direct_cases(built, which):
    """pg_pan_medoids on matrices no GFA fixture reaches (tests/support/cluster_direct.py): sizes across a wave and the tiles of
    candidates against the restatement; 1 025 columns and k = 1 024 against the checker build; one huge cluster with one row a chunk;
    all-equal distances and copies of columns; the iteration chunks at 1, 8 and 3; growing and shrinking sizes on the cached buffers;
    entries in the upper half of the range at 257 to 1 281 columns, where every sum needs 64 bits (magnitude)"""
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=180, cwd=ROOT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]
