"""Quantitative traits on the MI355X: the permuted value rows are made by k_qtrait_perm and multiplied with the gene rows by the int8
MFMA kernel k_qtrait_count (pga_pan_qtrait, k_qtrait.hpp).  The product must print the bytes the checker build prints (oracle backend:
no pan_qtrait entry, so the host loops of trait.cpp -- a second implementation; U, auc, z, p_wilcox and q_bh are host code both share)
and the integers of the numpy restatement (tests/support/qtrait_ref.py).  Every step runs in a child process under a timeout of its
own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "qtrait_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import assoc_ref as ar  # noqa: E402
import dist_ref  # noqa: E402
import qtrait_ref as qr  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["C4", "bact20", "human8"]
HEADER = (qr.HEADER + "\n").encode()
OPTION_SETS = [([], {}), (["-n", "0"], dict(n_perm=0)), (["-n", "37", "-s", "5", "-c", "2"], dict(n_perm=37, seed=5, min_count=2)),
               (["-n", "3000", "-p", "0.07"], dict(n_perm=3000, max_p=0.07))]


def run(exe, args, timeout=300, env=None):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    if r.returncode != 0:
        sys.stderr.write("%s: exit %d, stderr: %s\n" % (" ".join(args[:4]), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("name", NAMES)
def test_file_route(built, name):
    gfa, tf = os.path.join(GOLD, name + ".gfa.gz"), os.path.join(GOLD, "qtrait", name + ".tsv")
    genes, P = ar.read_gfa(gfa)
    asm = list(dist_ref.presence(gfa, "gene")[0])
    names, V = qr.read_file(tf, asm)
    n_line = 0
    for args, kw in OPTION_SETS:
        rc, out, _ = run(HIP, ["qtrait", "-t", tf] + args + [gfa])
        rc2, out2, _ = run(ORA, ["qtrait", "-t", tf] + args + [gfa])
        assert rc == 0 and rc2 == 0 and out == out2 and out.startswith(HEADER), " ".join(args)
        want = qr.table(genes, asm, P, names, V, **kw)
        got = qr.parse(out)
        assert [(g["Trait"], g["Gene"], g["N"], g["nG"], g["U"], g["n_ge"], g["p_perm"]) for g in got] == \
            [(w[0], w[1], w[2], w[3], w[4], w[9], w[10]) for w in want], " ".join(args)
        n_line += len(got)
    assert n_line > 0


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, tmp_path, name):
    """`pangene --qtrait=F *.paf` on the device: what the checker prints, and what `pangene qtrait -t F` prints for the GFA of the same run"""
    files, tf = _paf_dir(name), os.path.join(GOLD, "qtrait", name + ".tsv")
    rc, gfa, _ = run(HIP, files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    for mem, fil in ((["--qtrait=" + tf], []), (["--qtrait=" + tf, "--qtrait-perm=333", "--qtrait-seed=4"], ["-n", "333", "-s", "4"])):
        rc1, a, _ = run(HIP, mem + files)
        rc2, b, _ = run(HIP, ["qtrait", "-t", tf] + fil + [str(tmp_path / "g.gfa")])
        rc3, c, _ = run(ORA, mem + files)
        assert rc1 == 0 and rc2 == 0 and rc3 == 0 and a == b == c and a.startswith(HEADER) and a.count(b"\n") > 1, mem


def test_refused_when_sharded(built):
    rc, out, err = run(HIP, ["--gpus", "2", "--qtrait=" + os.path.join(GOLD, "qtrait", "C4.tsv")] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--qtrait" in err


@pytest.mark.parametrize("which", ["identity", "tiles", "digits", "rows", "batches", "large", "buffers", "range", "limit"])
def test_direct_cases(built, which):
    """pga_pan_qtrait on matrices no GFA fixture reaches (tests/support/qtrait_direct.py), a, D and k compared completely with the
    restatement.  identity: G = N = 200, gene g in column g alone, distinct values: d_rows[p][g] == perm_rows[p][g] for 130 permutations,
    the check of the MFMA's lane maps.  tiles: G in {1, 127, 128, 129, 300} x N in {2, 3, 63, 64, 65, 255, 256, 257, 1 000} x n in
    {1, 127, 129}, d_rows completely for N in {65, 257, 1 000}.  digits: N = 1 000 without ties (|c2| up to 999, both bytes live), with
    three tie groups, N = 100 (hi = 0: the kernel without the hi plane), rows of all ones (D_p = 0 for every p), empty rows.  rows:
    perm_rows for N = 31, 64, 256 (LDS form), 257 and 4 200 (global form) against c2[order(N, p, seed)], which pins the device's 64-bit
    %.  batches: PANGENE_QTRAIT_BATCH=256 in the child, n = 255, 256, 257, 773.  large: G = 20 003 x N = 1 001 with a planted trait,
    n = 2 000.  buffers: growing then shrinking shapes, cuda tensors, pga_host_trim(0) and again.  range: N = 32 001 is PGA_ERR_RANGE
    before anything is launched.  limit: N = 32 000 and 31 999 without ties (hi = +-125, lo = 127 and -128, |D| = N^2 / 4) and 31 999 with
    three tie groups, G = 130, n = 130, perm_rows and d_rows completely."""
    env = dict(os.environ)
    env.pop("PANGENE_QTRAIT_BATCH", None)
    if which == "batches":
        env["PANGENE_QTRAIT_BATCH"] = "256"
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT, env=env)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]
