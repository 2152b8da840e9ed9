"""Phylogenetic signal on the MI355X: the orders, the classes x permutations up passes and the counts come from the HIP kernels of
k_phylosig.hpp (pga_pan_phylosig).  The product must print the bytes the checker build prints (oracle backend: no pan_phylosig entry, so
the host loops of pan_phylosig.hpp -- a second implementation) and return what the restatement (tests/support/phylosig_ref.py) returns.
Every step runs in a child process under a timeout of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "phylosig_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import phylosig_ref as ps  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["C4", "bact20", "human8"]


def run(exe, args, timeout=60):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write("%s: exit %d, stderr: %s\n" % (" ".join(args[:4]), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r.returncode, r.stdout, r.stderr


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


def direct(which, env=None):
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=ROOT, env=env)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]


@pytest.mark.parametrize("name", NAMES)
def test_file_route(built, name):
    """pg_phylosig_file on the device prints the checker's bytes, and the restatement's, for the five option sets and -p 0.05 (one child
    process: the device comes up once)"""
    direct("file:" + name)


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, name):
    """`--phylosig ...` over the PAF files on the device (capi.run, pg_write_phylosig): the bytes pg_phylosig_file prints for the GFA of
    the same run, in the product and in the checker build, for the five option sets and -p 0.05"""
    direct("memory:" + name)


def test_command_line(built):
    """the product's command line itself: `pangene phylosig` and `pangene --phylosig` print what the checker's command line prints"""
    gfa = os.path.join(GOLD, "bact20.gfa.gz")
    args = ["phylosig", "-a", "nj", "-g", "2", "-n", "300", gfa]
    rc1, a, _ = run(HIP, args)
    rc2, b, _ = run(ORA, args)
    assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(ps.HEADER) and a.count(b"\n") > 2
    args = ["--phylosig=200", "--phylosig-min=1", "--phylosig-seed=3"] + _paf_dir("bact20")
    rc1, a, _ = run(HIP, args)
    rc2, b, _ = run(ORA, args)
    assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(ps.HEADER) and a.count(b"\n") > 2


def test_refused_when_sharded(built):
    rc, out, err = run(HIP, ["--gpus", "2", "--phylosig"] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--phylosig" in err
    rc, out, err = run(HIP, ["phylosig", "-g", "256", os.path.join(GOLD, "C4.gfa.gz")])
    assert rc == 1 and out == b"" and b"-g" in err


@pytest.mark.parametrize("which", ["shapes", "trees", "deep", "costs", "counts", "batches", "buffers", "refused", "range"])
def test_direct_cases(built, which):
    """pga_pan_phylosig and pg_pan_phylosig against the restatement -- every word of the first batch's orders and costs, n_le, n_ge and
    sum -- on shapes no GFA fixture reaches: 1 .. 257 permutations (the wave, the workgroup of 128 lanes) x 1 .. 9 classes (the remainder
    of the classes a lane carries, for 1, 2 and 4 of them) x 2 .. 257 leaves (the 32-op program word, the orders in LDS up to 256 leaves
    and in the scratch buffer beyond) x 1 .. 1 000 items; a caterpillar of 300 leaves (a stack of 2) and balanced trees of 2^1 .. 2^10
    leaves (stacks of 2 .. 11); one balanced tree of 32 768 leaves, 128 permutations x 8 classes, the stack limit of 16 with the full LDS
    footprint; five cost pairs on 65 leaves; 257 real items over 65 leaves with 200 permutations, where the restatement must first have
    met cost < obs, == obs and > obs; PANGENE_PHYLOSIG_BATCH=64 with 63 .. 200 permutations, so that counts and sums add across batches;
    sizes growing and shrinking on the cached buffers with pga_host_trim(0) in between; a program that needs 17 entries, malformed
    programs, a leaf list that is no permutation, classes that do not ascend or leave 1 .. n_leaf - 1 and an item's class out of range,
    turned away before any launch; and the sizes and costs out of range (tests/support/phylosig_direct.py)"""
    direct(which, dict(os.environ, PANGENE_PHYLOSIG_BATCH="64") if which == "batches" else None)
