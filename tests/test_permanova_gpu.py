"""PERMANOVA on the MI355X: the squared distances become signed-byte digit planes (k_perma_prep), the permuted label rows come from
k_trait_perm, A_p = y_p . W . y_p of every permutation from the int8 MFMA kernel k_perma_quad and the 128-bit compare from k_perma_stat
(pga_pan_permanova, k_permanova.hpp).  The product must print the bytes the checker build prints (oracle backend: no pan_permanova entry, so
the host loops of tree.cpp -- a second implementation; the statistics and the text are host code both share) and the integers of the
restatement (tests/support/permanova_ref.py).  Every step runs in a child process under a timeout of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "permanova_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import dist_ref  # noqa: E402
import permanova_ref as pr  # noqa: E402
import tree_ref  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["C4", "bact20", "human8"]
HEADER = (pr.HEADER + "\n").encode()
KINDS = (("gene", "jaccard"), ("adj", "diff"))
OPTION_SETS = [([], {}), (["-n", "0"], dict(n_perm=0)), (["-n", "37", "-s", "5"], dict(n_perm=37, seed=5)), (["-n", "999"], dict(n_perm=999))]


def run(exe, args, timeout=300, env=None):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    if r.returncode != 0:
        sys.stderr.write("%s: exit %d, stderr: %s\n" % (" ".join(args[:4]), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("name", NAMES)
def test_file_route(built, name):
    gfa, tf = os.path.join(GOLD, name + ".gfa.gz"), os.path.join(GOLD, "trait", name + ".tsv")
    n_line = 0
    for kind, metric in KINDS:
        asm, P = dist_ref.presence(gfa, kind)
        names, L = pr.read_traits(tf, list(asm))
        q, F = tree_ref.fixed(dist_ref.shared(P), metric)
        for args, kw in OPTION_SETS:
            cmd = ["permanova", "-t", tf, "-T", kind, "-m", metric] + args + [gfa]
            rc, out, _ = run(HIP, cmd)
            rc2, out2, _ = run(ORA, cmd)
            assert rc == 0 and rc2 == 0 and out == out2 and out.startswith(HEADER), (kind, args)
            assert out == pr.text(names, L, q, F, **kw), (kind, args)
            n_line += out.count(b"\n") - 1
    assert n_line > 0


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, tmp_path, name):
    """`pangene --permanova=F *.paf` on the device: what the checker prints, and what `pangene permanova -t F` prints for the GFA of the same run"""
    files, tf = _paf_dir(name), os.path.join(GOLD, "trait", name + ".tsv")
    rc, gfa, _ = run(HIP, files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    for mem, fil in ((["--permanova=" + tf], []),
                     (["--permanova=" + tf, "--permanova-type=adj", "--permanova-metric=diff", "--permanova-perm=333", "--permanova-seed=4"],
                      ["-T", "adj", "-m", "diff", "-n", "333", "-s", "4"])):
        rc1, a, _ = run(HIP, mem + files)
        rc2, b, _ = run(HIP, ["permanova", "-t", tf] + fil + [str(tmp_path / "g.gfa")])
        rc3, c, _ = run(ORA, mem + files)
        assert rc1 == 0 and rc2 == 0 and rc3 == 0 and a == b == c and a.startswith(HEADER) and a.count(b"\n") > 1, mem


def test_refused_when_sharded(built):
    rc, out, err = run(HIP, ["--gpus", "2", "--permanova=" + os.path.join(GOLD, "trait", "C4.tsv")] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--permanova" in err


@pytest.mark.parametrize("which", ["maps", "tiles", "digits", "ties", "magnitude", "batches", "large", "buffers", "range"])
def test_direct_cases(built, which):
    """pga_pan_permanova on matrices no GFA fixture reaches (tests/support/permanova_direct.py): T, A, B, k and A_p, B_p and the label row of
    every permutation of the first batch compared completely with the restatement.  maps: N = 200, all w distinct (w_ij = (1 + i N + j)^2
    mirrored), 130 permutations: the lane maps, the mask and the symmetry doubling.  tiles: N in {3, 63, 64, 65, 127, 128, 129, 255, 257,
    300} x n in {1, 127, 129}.  digits: D = 1, 2, 3, 5, 8 planes with the digits -128 and 127 where a plane can hold them, and an all-zero
    middle plane.  ties: few distinct distances, so many G_p = G_obs; an all-equal matrix gives k = n.  magnitude: entries of 2^29 - 1 at
    N = 129 (s = 6, N A beyond 2^63: the 128-bit compare).  batches: PANGENE_PERMA_BATCH=256 in the child, n = 255, 256, 257, 773.  large:
    N = 1 001, n = 300, planted and random groups.  buffers: growing then shrinking shapes through pg_pan_permanova, cuda tensors,
    pga_host_trim(0) and again.  range: N = 16 385 is PGA_ERR_RANGE before anything is launched."""
    env = dict(os.environ)
    env.pop("PANGENE_PERMA_BATCH", None)
    if which == "batches":
        env["PANGENE_PERMA_BATCH"] = "256"
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT, env=env)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]
