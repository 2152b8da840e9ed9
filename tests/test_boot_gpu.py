"""Bootstrap support of the trees on the MI355X: the replicates come from the HIP kernels of k_boot.hpp and the batched joins of
k_join.hpp (pga_pan_boot).  The product must print and return what the numpy restatement (tests/support/boot_ref.py) and the checker
build (oracle backend: no pan_boot entry, so the host loops of tree.cpp -- a second implementation) print and return.  Every step runs
in a child process under a timeout of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "boot_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import boot_ref as br  # noqa: E402
import dist_ref as dr  # noqa: E402

pytestmark = pytest.mark.gpu
GFAS = sorted(os.path.join(GOLD, f) for f in os.listdir(GOLD) if f.endswith(".gfa.gz")) + \
    sorted(os.path.join(GOLD, "bubble", f) for f in os.listdir(os.path.join(GOLD, "bubble")) if f.endswith(".gfa"))
ROUTES = (("gene", "jaccard", "nj"), ("adj", "diff", "upgma"))


def run(exe, args, timeout=300):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write("%s: exit %d, stderr: %s\n" % (" ".join(args[:4]), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("gfa", GFAS, ids=[os.path.relpath(g, GOLD) for g in GFAS])
def test_file_route(built, gfa):
    for kind, metric, method in ROUTES:
        names, P = dr.presence(gfa, kind)
        args = ["tree", "-t", kind, "-m", metric, "-a", method, "-b", "5", "-s", "7", gfa]
        rc, out, _ = run(HIP, args)
        assert rc == 0 and out == br.text(names, P, metric, method, 5, 7), " ".join(args)
        rc, out2, _ = run(ORA, args)
        assert rc == 0 and out2 == out


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", ["C4", "bact20", "human8"])
def test_in_memory_route(built, tmp_path, name):
    """`pangene --tree --tree-boot=4 *.paf` on the device: what the checker prints, and what `pangene tree -b 4` prints for the GFA of the same run"""
    files = _paf_dir(name)
    rc, gfa, _ = run(HIP, files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    for kind, method in (("gene", "nj"), ("adj", "upgma")):
        rc1, a, _ = run(HIP, ["--tree=" + kind, "--tree-method=" + method, "--tree-boot=4", "--tree-seed=3"] + files)
        rc2, b, _ = run(HIP, ["tree", "-t", kind, "-a", method, "-b", "4", "-s", "3", str(tmp_path / "g.gfa")])
        rc3, c, _ = run(ORA, ["--tree=" + kind, "--tree-method=" + method, "--tree-boot=4", "--tree-seed=3"] + files)
        assert rc1 == 0 and rc2 == 0 and rc3 == 0 and a == b == c and a.endswith(b";\n"), kind
        rc4, plain, _ = run(HIP, ["--tree=" + kind, "--tree-method=" + method] + files)
        assert rc4 == 0 and plain != a and plain.count(b")") == a.count(b")")


def test_refused_when_sharded(built):
    rc, out, err = run(HIP, ["--gpus", "2", "--tree", "--tree-boot=4"] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--tree" in err


@pytest.mark.parametrize("which", ["draws", "resample", "wide", "groups", "joins", "large", "chunks", "parts", "metrics", "buffers", "counts"])
def test_direct_cases(built, which):
    """pga_pan_boot, pg_pan_boot and pg_pan_boot_records on matrices no GFA fixture reaches: the draws hook against Python integers; item
    counts across a word's boundaries, the global-memory path of the resampling and a full row; rows of several workgroups of words with 4
    and with 32 assemblies to a workgroup of the resampling; several replicate groups inside one call; the batched joins
    across the kernels' wave, tile and workgroup boundaries against the restatement and 1 025 against the checker build; chunks of 3, 3, 1
    and of one; a search whose workgroups stride over several tiles; both metrics with replicates whose F differs from the reference's;
    growing and shrinking sizes on the cached buffers; and the support counts (tests/support/boot_direct.py)"""
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]
