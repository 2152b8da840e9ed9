"""Gene associations on the MI355X: the pairs are counted and selected by the HIP kernels of k_assoc.hpp (pga_pan_assoc).  The product
must print and return what the numpy restatement (tests/support/assoc_ref.py, exact integers) and the checker build (oracle backend:
no pan_assoc entry, so the host loops of assoc.cpp -- a second implementation) print and return.  Every step runs in a child process
under a timeout of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "assoc_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import assoc_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu
GFAS = sorted(os.path.join(GOLD, f) for f in os.listdir(GOLD) if f.endswith(".gfa.gz")) + \
    sorted(os.path.join(GOLD, "bubble", f) for f in os.listdir(os.path.join(GOLD, "bubble")) if f.endswith(".gfa"))
HEADER = b"GeneA\tGeneB\tnA\tnB\tnAB\tphi\n"


def run(exe, args, timeout=300, env=None):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    if r.returncode != 0:
        sys.stderr.write("%s: exit %d, stderr: %s\n" % (" ".join(args[:4]), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("gfa", GFAS, ids=[os.path.relpath(g, GOLD) for g in GFAS])
def test_file_route(built, gfa):
    genes, P = ar.read_gfa(gfa)
    for args, kw in (([], {}), (["-r", "0.5", "-c", "1"], dict(min_phi=0.5, min_count=1)), (["-r", "0.9", "-s", "neg"], dict(min_phi=0.9, sign="neg")),
                     (["-r", "0.95", "-s", "pos", "-c", "3"], dict(min_phi=0.95, sign="pos", min_count=3))):
        want = ar.text(genes, P, **kw)
        if want.count(b"\n") > 200000:
            continue
        rc, out, _ = run(HIP, ["assoc"] + args + [gfa])
        assert rc == 0 and out == want, " ".join(args)
        rc, out2, _ = run(ORA, ["assoc"] + args + [gfa])
        assert rc == 0 and out2 == out
    # the second run of the pairs kernel: a starting capacity of one record
    rc, out, _ = run(HIP, ["assoc", "-r", "0.5", "-c", "1", gfa], env=dict(os.environ, PANGENE_ASSOC_CAP="1"))
    assert rc == 0 and out == ar.text(genes, P, min_phi=0.5, min_count=1)


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", ["C4", "bact20", "human8"])
def test_in_memory_route(built, tmp_path, name):
    """`pangene --assoc *.paf` on the device: what the checker prints, and what `pangene assoc` prints for the GFA of the same run"""
    files = _paf_dir(name)
    rc, gfa, _ = run(HIP, files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    for mem, fil in ((["--assoc"], []), (["--assoc=0.4", "--assoc-min-count=1", "--assoc-sign=neg"], ["-r", "0.4", "-c", "1", "-s", "neg"])):
        rc1, a, _ = run(HIP, mem + files)
        rc2, b, _ = run(HIP, ["assoc"] + fil + [str(tmp_path / "g.gfa")])
        rc3, c, _ = run(ORA, mem + files)
        assert rc1 == 0 and rc2 == 0 and rc3 == 0 and a == b == c and a.startswith(HEADER), mem


def test_refused_when_sharded(built):
    rc, out, err = run(HIP, ["--gpus", "2", "--assoc"] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--assoc" in err


def test_too_many_pairs(built, tmp_path):
    """more than -x pairs on the device: status 1, nothing on stdout, the number that passed on stderr"""
    f = tmp_path / "m.gfa"
    f.write_text("".join("S\tg%d\t*\tLN:i:1\n" % i for i in range(4)) +
                 "".join("W\ts%d\t0\tc\t0\t1\t%s\n" % (a, ">g0>g1>g2>g3" if a < 3 else ">x") for a in range(6)))
    rc, out, err = run(HIP, ["assoc", "-x", "5", str(f)])
    assert rc == 1 and out == b"" and b"6 gene pairs" in err
    rc, out, _ = run(HIP, ["assoc", "-x", "6", str(f)])
    assert rc == 0 and out.count(b"\n") == 7


@pytest.mark.parametrize("which", ["large", "wide", "sizes", "edges", "threshold", "band337", "band801"])
def test_direct_cases(built, which):
    """pg_pan_assoc on matrices no GFA fixture reaches, compared completely with the checker build and the restatement
    (tests/support/assoc_direct.py): G = 20 003 x A = 1 001 with planted modules, the forced second run and a cuda tensor (large);
    G = 70 001 and G = 1 000 003 rows, beyond the row limit of pan_shared (wide); growing and shrinking sizes that reuse the cached
    buffers, one of them with 6.7 M selected pairs (sizes); every slot of an off-diagonal and of a diagonal tile exactly on the threshold, one
    permille below and above it, on either side of D = 0 and under every sign, and the exact small cases of tests/test_assoc.py
    (threshold); every pair the search of assoc_ref.band_search finds inside the guard band at A = 16 777 215, on, above and below the
    threshold, at p and p + 1 (band337, band801)"""
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900, cwd=ROOT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]
