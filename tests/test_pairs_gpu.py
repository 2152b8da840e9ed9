"""The lineage-aware trait test on the MI355X: the tree dynamic programmes come from the HIP kernel of k_pairs.hpp (pga_pan_pairs).  The
product must print and return what the restatement (tests/support/pairs_ref.py) and the checker build (oracle backend: no pan_pairs
entry, so the host loops of trait.cpp -- a second implementation) print and return.  Every step runs in a child process under a timeout
of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "pairs_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import assoc_ref as ar  # noqa: E402
import dist_ref as dr  # noqa: E402
import pairs_ref as pr  # noqa: E402
import test_pairs as tp  # noqa: E402

pytestmark = pytest.mark.gpu
GFAS = tp.GFAS
METHODS = ("nj", "upgma")


def run(exe, args, timeout=300):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write("%s: exit %d, stderr: %s\n" % (" ".join(args[:4]), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("gfa", GFAS, ids=[os.path.basename(g) for g in GFAS])
def test_file_route(built, tmp_path, gfa):
    genes, P = ar.read_gfa(gfa)
    asm = list(dr.presence(gfa, "gene")[0])
    fn, names, L = tp.fixture_traits(gfa, asm, tmp_path)
    rc, plain, _ = run(HIP, ["trait", "-t", fn, "-n", "10", gfa])
    assert rc == 0
    for method in METHODS:
        args = ["trait", "-t", fn, "-n", "10", "-L", method, gfa]
        rc, out, _ = run(HIP, args)
        assert rc == 0
        tp.check_table(out, plain, pr.table(genes, P, names, L, method))
        rc, out2, _ = run(ORA, args)
        assert rc == 0 and [l.split(b"\t")[11:] for l in out2.split(b"\n")] == [l.split(b"\t")[11:] for l in out.split(b"\n")]


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", ["C4", "bact20", "human8"])
def test_in_memory_route(built, tmp_path, name):
    """`pangene --trait=F --trait-lineage=M *.paf` on the device: the pair columns the checker prints, and the bytes `pangene trait -L M`
    prints for the GFA of the same run"""
    files = _paf_dir(name)
    f = os.path.join(GOLD, "trait", name + ".tsv")
    rc, gfa, _ = run(HIP, files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    for method in METHODS:
        opts = ["--trait=" + f, "--trait-perm=9", "--trait-lineage=" + method]
        rc1, a, _ = run(HIP, opts + files)
        rc2, b, _ = run(HIP, ["trait", "-t", f, "-n", "9", "-L", method, str(tmp_path / "g.gfa")])
        rc3, c, _ = run(ORA, opts + files)
        assert rc1 == 0 and rc2 == 0 and rc3 == 0 and a == b and a.startswith(tp.HEADER) and a.count(b"\n") > 1
        assert [l.split(b"\t")[11:] for l in c.split(b"\n")] == [l.split(b"\t")[11:] for l in a.split(b"\n")]
        assert [l.split(b"\t")[:6] for l in c.split(b"\n")] == [l.split(b"\t")[:6] for l in a.split(b"\n")]


def test_refused_when_sharded(built):
    f = os.path.join(GOLD, "trait", "C4.tsv")
    rc, out, err = run(HIP, ["--gpus", "2", "--trait=" + f, "--trait-lineage=nj"] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--trait" in err
    rc, out, err = run(HIP, ["trait", "-t", f, "-L", "ml", os.path.join(GOLD, "C4.gfa.gz")])
    assert rc == 1 and out == b"" and b"-L" in err


@pytest.mark.parametrize("which", ["sizes", "rows", "shapes", "deep", "buffers", "heavier", "refused"])
def test_direct_cases(built, which):
    """pga_pan_pairs and pg_pan_pairs on trees no GFA fixture reaches: gene counts around a word, a wave and a workgroup of 128 lanes; 1, 2
    and 5 label rows with a row without values and rows of one type; a caterpillar of 200 leaves (a stack of 2) and balanced trees of
    2^1 .. 2^8 leaves (stacks of 2 .. 9); 64 genes on balanced trees of 4 095 and 65 535 leaves with alternating types, where pairs reaches
    32 767 and the stack its limit of 16 (against the checker build; the smaller one against the restatement too); sizes growing and
    shrinking on the cached buffers; records whose heavier child is slot i in some joins and slot j in others; and the programs and sizes
    the entry refuses (tests/support/pairs_direct.py)"""
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]
