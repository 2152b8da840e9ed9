"""Gene gain and loss on the MI355X: the two passes and the node totals come from the HIP kernels of k_gainloss.hpp (pga_pan_gainloss).
The product must print the bytes the checker build prints (oracle backend: no pan_gainloss entry, so the host loops of pan_gainloss.hpp
-- a second implementation) and return what the restatement (tests/support/gainloss_ref.py) returns.  Every step runs in a child
process under a timeout of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "gainloss_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import gainloss_ref as gr  # noqa: E402

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
    """pg_gainloss_file on the device prints the checker's bytes, and the restatement's, for the five option sets (one child process:
    the device comes up once)"""
    direct("file:" + name)


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, name):
    """`--gainloss ...` over the PAF files on the device (capi.run, pg_write_gainloss): the bytes pg_gainloss_file prints for the GFA of
    the same run, in the product and in the checker build, for the five option sets"""
    direct("memory:" + name)


def test_command_line(built):
    """the product's command line itself: `pangene gainloss` and `pangene --gainloss` print what the checker's command line prints"""
    gfa = os.path.join(GOLD, "C4.gfa.gz")
    args = ["gainloss", "-o", "node", "-a", "nj", "-g", "2", gfa]
    rc1, a, _ = run(HIP, args)
    rc2, b, _ = run(ORA, args)
    assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(gr.NODE_HEADER) and a.count(b"\n") > 2
    args = ["--gainloss", "--gainloss-resolve=early"] + _paf_dir("C4")
    rc1, a, _ = run(HIP, args)
    rc2, b, _ = run(ORA, args)
    assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(gr.GENE_HEADER) and a.count(b"\n") > 2


def test_refused_when_sharded(built):
    rc, out, err = run(HIP, ["--gpus", "2", "--gainloss"] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--gainloss" in err
    rc, out, err = run(HIP, ["gainloss", "-g", "256", os.path.join(GOLD, "C4.gfa.gz")])
    assert rc == 1 and out == b"" and b"-g" in err


@pytest.mark.parametrize("which", ["shapes", "trees", "deep", "refused", "ties", "chunks", "buffers", "range"])
def test_direct_cases(built, which):
    """pga_pan_gainloss and pg_pan_gainloss against the restatement -- gene, node and every word of the state rows -- on shapes no GFA
    fixture reaches: 1 .. 4 097 items (the ballot word, the workgroup of 128 lanes) over 1 .. 65 leaves (the 32-op program word, the 32-leaf
    gather); a caterpillar of 300 leaves (a stack of 2) and balanced trees of 2^1 .. 2^10 leaves (stacks of 2 .. 11); one balanced tree of
    32 768 leaves x 65 items, the stack limit of 16 with the full LDS footprint; a program that needs 17 entries, malformed programs and a
    par that contradicts the program, turned away before any launch; five cost pairs x both tie rules on 257 items over 65 leaves, where
    the restatement must have met each of the three ties; PANGENE_GAINLOSS_CHUNK=1024 with 1 023 .. 3 000 items, so that the node totals add
    across chunks; sizes growing and shrinking on the cached buffers with pga_host_trim(0) in between; and the sizes and costs out of
    range (tests/support/gainloss_direct.py)"""
    direct(which, dict(os.environ, PANGENE_GAINLOSS_CHUNK="1024") if which == "chunks" else None)
