"""Co-evolution on the MI355X: the reconstruction, the event rows, the pair counts and the selection come from the HIP kernels of
k_gainloss.hpp and k_coevo.hpp (pga_pan_coevo).  The product must print the bytes the checker build prints (oracle backend: no pan_coevo
entry, so the host loops of pan_coevo.hpp -- a second implementation) and return what the restatement (tests/support/coevo_ref.py)
returns.  Every step runs in a child process under a timeout of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "coevo_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import coevo_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["C4", "bact20", "human8", "dense"]


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
    """pg_coevo_file on the device prints the checker's bytes, and the restatement's rows, for the defaults and the five option sets (one
    child process: the device comes up once)"""
    direct("file:" + name)


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, name):
    """`--coevo ...` over the PAF files on the device (capi.run, pg_write_coevo): the bytes pg_coevo_file prints for the GFA of the same
    run, in the product and in the checker build, for the defaults and the five option sets"""
    direct("memory:" + name)


def test_command_line(built):
    """the product's command line itself: `pangene coevo` and `pangene --coevo` print what the checker's command line prints"""
    gfa = os.path.join(GOLD, "bact20.gfa.gz")
    args = ["coevo", "-a", "nj", "-s", "neg", gfa]
    rc1, a, _ = run(HIP, args)
    rc2, b, _ = run(ORA, args)
    assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(cr.HEADER) and a.count(b"\n") == 10
    args = ["--coevo=0.5", "--coevo-type=adj", "--coevo-min=1"] + _paf_dir("C4")
    rc1, a, _ = run(HIP, args)
    rc2, b, _ = run(ORA, args)
    assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(cr.HEADER) and a.count(b"\n") > 1


def test_refused_when_sharded_and_too_many(built):
    rc, out, err = run(HIP, ["--gpus", "2", "--coevo"] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--coevo" in err
    rc, out, err = run(HIP, ["coevo", "-g", "256", os.path.join(GOLD, "C4.gfa.gz")])
    assert rc == 1 and out == b"" and b"-g" in err
    rc, out, err = run(HIP, ["coevo", "-x", "64", os.path.join(GOLD, "bact20.gfa.gz")])
    assert rc == 1 and out == b"" and b"65 item pairs passed, more than the 64 allowed (-x)" in err


@pytest.mark.parametrize("which", ["shapes", "leaves", "wide", "tiles", "chunks", "cap", "buffers", "refused", "range"])
def test_direct_cases(built, which):
    """pga_pan_coevo and pg_pan_coevo against the restatement -- the events, every pair record and every word of the event rows -- on shapes
    no GFA fixture reaches: 1 .. 4 097 items (the ballot word, the workgroup of 128 lanes); caterpillars and balanced trees of 1, 2, 3, 17,
    33, 34 and 65 leaves (B across 32 and 64 bits) and of 513 and 514 (B = 1 024 and 1 026: the 32-word K chunk of k_ce_pairs and the span of
    k_ce_rows, and one word more); E = 1, 2, 127, 128, 129 and 257 eligible items around the 128 x 128 tile, and 300 scattered over 3 000
    items, so that the places matter; PANGENE_COEVO_CHUNK=1024 with 1 023 .. 3 000 items, so that rows written by different chunks meet in
    one tile; PANGENE_COEVO_CAP=16 with more pairs than that, the second run of k_ce_pairs; sizes growing and shrinking on the cached
    buffers with pga_host_trim(0) in between; malformed programs, a program that needs 17 stack entries, options, costs and sizes out of
    range, turned away before any launch (tests/support/coevo_direct.py)"""
    env = None
    if which == "chunks":
        env = dict(os.environ, PANGENE_COEVO_CHUNK="1024")
    elif which == "cap":
        env = dict(os.environ, PANGENE_COEVO_CAP="16")
    direct(which, env)
