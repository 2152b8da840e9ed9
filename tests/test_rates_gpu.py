"""Gain and loss rates on the MI355X: the likelihoods of every batch of parameter sets and the posteriors come from the HIP kernels of
k_rates.hpp (pga_pan_rates).  Floating point: the product and the checker build (oracle backend: no pan_rates entry, so the plain loops
of pan_rates.hpp -- a second implementation) are each compared with the restatement (tests/support/rates_ref.py) within the bounds that
follow from the arithmetic; they are not compared byte for byte.  Every step runs in a child process under a timeout of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
DIRECT = os.path.join(ROOT, "tests", "support", "rates_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import rates_ref as rr  # noqa: E402

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
    """pg_rates_file on the device and in the checker build, each against the restatement, for the five option sets: three with given
    rates, where every number is compared, and two fits, where lnL is compared at the rates the table prints (one child process: the
    device comes up once)"""
    direct("file:" + name)


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, name):
    """`--rates ...` over the PAF files on the device (capi.run, pg_write_rates) and in the checker build, each against the restatement
    over the GFA of the same run"""
    direct("memory:" + name)


def test_command_line(built, tmp_path):
    """the product's command line itself: `pangene rates` and `pangene --rates` against the restatement"""
    gfa = os.path.join(GOLD, "bact20.gfa.gz")
    kw = rr.OPTION_SETS[1]
    rc, a, _ = run(HIP, ["rates"] + rr.option_args(**kw)[0] + [gfa])
    assert rc == 0 and a.startswith(rr.NODE_HEADER) and rr.check_table(a, gfa, **kw) == ""
    rc, a, _ = run(HIP, ["rates", gfa])
    assert rc == 0 and a.startswith(rr.GENE_HEADER) and a.count(b"\n") > 2 and rr.check_table(a, gfa) == ""
    kw = rr.OPTION_SETS[0]
    rc, a, _ = run(HIP, rr.option_args(**kw)[1] + _paf_dir("C4"))
    rc2, g, _ = run(HIP, _paf_dir("C4"))
    gfa = str(tmp_path / "g.gfa")
    with open(gfa, "wb") as f:
        f.write(g)
    assert rc == 0 and rc2 == 0 and rr.check_table(a, gfa, **kw) == ""


def test_refused(built):
    """--gpus 2 --rates is refused, and so is one rate without the other: status 1, nothing on stdout"""
    rc, out, err = run(HIP, ["--gpus", "2", "--rates"] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--rates" in err
    gfa = os.path.join(GOLD, "C4.gfa.gz")
    for args in (["-g", "1"], ["-l", "2"], ["-g", "0", "-l", "1"], ["-g", "x", "-l", "1"], ["-o", "tree"], ["-c", "-1"]):
        rc, out, err = run(HIP, ["rates"] + args + [gfa])
        assert rc == 1 and out == b"" and err != b"", args


@pytest.mark.parametrize("which", ["shapes", "trees", "deep", "exact", "post", "chunks", "refused", "buffers", "same", "fit"])
def test_direct_cases(built, which):
    """pga_pan_rates and pg_pan_rates against the restatement -- every L with the exponents aligned, gene, node and every entry of the
    posterior rows -- on shapes no GFA fixture reaches: 1 .. 4 097 items (the wave, the workgroup of 128 lanes) over 1 .. 65 leaves (the
    32-op program word, the 32-leaf gather) with 1, 2 and 25 parameter sets; a caterpillar of 300 leaves (a stack of 2) and balanced
    trees of 2^1 .. 2^10 leaves; one balanced tree of 32 768 leaves x 65 items, the stack limit of 16 with the full LDS footprint of both
    kernels; a caterpillar of 1 200 leaves whose every L is exactly 2^-1200, below fp64's range, compared for equality; the posteriors
    against the enumeration over all inner assignments at 7 and 9 leaves; PANGENE_RATES_CHUNK=256 with 255 .. 1 000 items and a trailing
    all-absent item kept out of the node totals; malformed programs, a par that contradicts the program, a stack need of 17, a NaN, a
    negative and an infinite table entry, n_set 0 and 65, turned away before any launch; sizes growing and shrinking on the cached buffers
    with pga_host_trim(0) in between; two calls that return equal bits; and the named cases of the fit, whose lattice paths must
    coincide with the restatement's (tests/support/rates_direct.py)"""
    direct(which, dict(os.environ, PANGENE_RATES_CHUNK="256") if which == "chunks" else None)
