"""Gene-trait association on the MI355X: the permuted label rows are made and counted by the HIP kernels of k_trait.hpp
(pga_pan_trait).  The product must print the bytes the checker build prints (oracle backend: no pan_trait entry, so the host loops of
trait.cpp -- a second implementation; phi, p_fisher and q_bh are host code both share) and the integers of the numpy restatement
(tests/support/trait_ref.py).  Every step runs in a child process under a timeout of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "trait_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import assoc_ref as ar  # noqa: E402
import dist_ref  # noqa: E402
import trait_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["C4", "bact20", "human8"]
HEADER = (tr.HEADER + "\n").encode()
OPTION_SETS = [([], {}), (["-n", "0"], dict(n_perm=0)), (["-n", "37", "-s", "5", "-c", "2"], dict(n_perm=37, seed=5, min_count=2)),
               (["-n", "3000", "-p", "0.07"], dict(n_perm=3000, max_p=0.07))]


def run(exe, args, timeout=300, env=None):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    if r.returncode != 0:
        sys.stderr.write("%s: exit %d, stderr: %s\n" % (" ".join(args[:4]), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r.returncode, r.stdout, r.stderr


def read_traits(path, asm):
    """(trait names, labels (T, A) int8) of a trait fixture"""
    import numpy as np
    lines = [l for l in open(path).read().split("\n")]
    names = lines[0].split("\t")[1:]
    L = np.full((len(names), len(asm)), -1, dtype=np.int8)
    for l in lines[1:]:
        if not l or l[0] == "#":
            continue
        f = l.split("\t")
        L[:, asm.index(f[0])] = [-1 if v in ("NA", "") else int(v) for v in f[1:]]
    return names, L


@pytest.mark.parametrize("name", NAMES)
def test_file_route(built, name):
    gfa, tf = os.path.join(GOLD, name + ".gfa.gz"), os.path.join(GOLD, "trait", name + ".tsv")
    genes, P = ar.read_gfa(gfa)
    asm = list(dist_ref.presence(gfa, "gene")[0])
    names, L = read_traits(tf, asm)
    n_line = 0
    for args, kw in OPTION_SETS:
        rc, out, _ = run(HIP, ["trait", "-t", tf] + args + [gfa])
        rc2, out2, _ = run(ORA, ["trait", "-t", tf] + args + [gfa])
        assert rc == 0 and rc2 == 0 and out == out2 and out.startswith(HEADER), " ".join(args)
        if "max_p" in kw:  # the cutoff must not sit on a p: no restatement p within 1e-6 relative of it
            assert all(abs(w[7] - kw["max_p"]) > 1e-6 * kw["max_p"] for w in tr.table(genes, asm, P, names, L, n_perm=0))
        want = tr.table(genes, asm, P, names, L, **kw)
        got = tr.parse(out)
        assert [(g["Trait"], g["Gene"], g["N"], g["nT"], g["nG"], g["nTG"], "NA" if g["n_ge"] is None else str(g["n_ge"]), g["p_perm"]) for g in got] == \
            [w[:6] + w[9:] for w in want], " ".join(args)
        n_line += len(got)
    assert n_line > 0


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, tmp_path, name):
    """`pangene --trait=F *.paf` on the device: what the checker prints, and what `pangene trait -t F` prints for the GFA of the same run"""
    files, tf = _paf_dir(name), os.path.join(GOLD, "trait", name + ".tsv")
    rc, gfa, _ = run(HIP, files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    for mem, fil in ((["--trait=" + tf], []), (["--trait=" + tf, "--trait-perm=333", "--trait-seed=4"], ["-n", "333", "-s", "4"])):
        rc1, a, _ = run(HIP, mem + files)
        rc2, b, _ = run(HIP, ["trait", "-t", tf] + fil + [str(tmp_path / "g.gfa")])
        rc3, c, _ = run(ORA, mem + files)
        assert rc1 == 0 and rc2 == 0 and rc3 == 0 and a == b == c and a.startswith(HEADER) and a.count(b"\n") > 1, mem


def test_refused_when_sharded(built):
    rc, out, err = run(HIP, ["--gpus", "2", "--trait=" + os.path.join(GOLD, "trait", "C4.tsv")] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--trait" in err


@pytest.mark.parametrize("which", ["large", "batches", "sizes", "rows", "edges", "wide"])
def test_direct_cases(built, which):
    """pg_pan_trait on matrices no GFA fixture reaches, a, s and k compared completely with the restatement
    (tests/support/trait_direct.py): G = 20 003 x A = 1 001 with planted traits, n = 2 000 (large); n = one batch - 1, one batch, one
    batch + 1 and three batches + 5, the batch read from the library (batches); N = 4 200, past the LDS form of k_trait_perm, then
    growing and shrinking shapes that reuse the cached buffers, cuda tensors among them (sizes); the permuted label rows of the first
    batch themselves for N = 31, 64, 1 000 and 4 200 against y[order(N, p, seed)], which pins the device's 64-bit % (rows; the rows
    come through the tests-only perm_rows pointer of pga_trait_in_t); N = 70 001 and 70 000 with t = 35 000, where the products of
    the thresholds pass 2^31, with the label row itself, D = 0 and every row on equality, and the 70 permuted rows themselves (wide)"""
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900, cwd=ROOT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]
