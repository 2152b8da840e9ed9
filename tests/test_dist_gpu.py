"""Pairwise distances on the MI355X: the shared-item counts come from the HIP kernel of k_dist.hpp (pga_pan_shared).  The product must
print and return what the numpy restatement (tests/support/dist_ref.py) and the checker build (oracle backend: no pan_shared entry,
so the host loops of dist.cpp -- a second implementation) print and return.  Every step runs in a child process under a timeout of
its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "dist_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import dist_ref as dr  # noqa: E402

pytestmark = pytest.mark.gpu
GFAS = sorted(os.path.join(GOLD, f) for f in os.listdir(GOLD) if f.endswith(".gfa.gz")) + \
    sorted(os.path.join(GOLD, "bubble", f) for f in os.listdir(os.path.join(GOLD, "bubble")) if f.endswith(".gfa"))


def run(exe, args, timeout=300):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write("%s: exit %d, stderr: %s\n" % (" ".join(args[:4]), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("gfa", GFAS, ids=[os.path.relpath(g, GOLD) for g in GFAS])
def test_file_route(built, gfa):
    for kind in ("gene", "adj"):
        names, P = dr.presence(gfa, kind)
        S = dr.shared(P)
        for m in dr.METRICS:
            args = ["dist", "-t", kind, "-m", m, gfa]
            rc, out, _ = run(HIP, args)
            assert rc == 0 and out == dr.text(names, S, m), " ".join(args)
            rc, out2, _ = run(ORA, args)
            assert rc == 0 and out2 == out
    names, P = dr.presence(gfa, "gene")
    rc, out, _ = run(HIP, ["dist", "-p", gfa])
    assert rc == 0 and out == dr.text(names, dr.shared(P), "jaccard", True)


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", ["C4", "bact20", "human8"])
def test_in_memory_route(built, tmp_path, name):
    """`pangene --dist *.paf` on the device: what the checker prints, and what `pangene dist` prints for the GFA of the same run"""
    files = _paf_dir(name)
    rc, gfa, _ = run(HIP, files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    for kind in ("gene", "adj"):
        rc1, a, _ = run(HIP, ["--dist=" + kind, "--dist-metric=shared"] + files)
        rc2, b, _ = run(HIP, ["dist", "-t", kind, "-m", "shared", str(tmp_path / "g.gfa")])
        rc3, c, _ = run(ORA, ["--dist=" + kind, "--dist-metric=shared"] + files)
        assert rc1 == 0 and rc2 == 0 and rc3 == 0 and a == b == c and a.startswith(b"Asm\t"), kind


def test_refused_when_sharded(built):
    rc, out, err = run(HIP, ["--gpus", "2", "--dist"] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--dist" in err


@pytest.mark.parametrize("which", ["large", "sizes", "edges"])
def test_direct_cases(built, which):
    """pg_pan_shared on matrices no GFA fixture reaches (A = 12 003, M = 70 001; split K at A = 200) and on a run of growing and
    shrinking sizes that reuse the cached buffers (tests/support/dist_direct.py)"""
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900, cwd=ROOT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]
