"""Principal coordinates on the MI355X: the products B x come from k_pcoa_mult over the int32 matrix, the Gram-Schmidt passes, the
norms and the Ritz vectors from the other kernels of k_pcoa.hpp (pga_pan_pcoa), the tridiagonal eigenproblem and the restart decisions
from the host between the chunks.  This is floating point: the product is compared with the numpy reference within the tolerances
tests/support/pcoa_ref.py derives from the stopping rule, never with the checker build byte for byte; only two runs of the same build are
(the determinism rule).  Every GPU step runs in a child process under a timeout of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
DIRECT = os.path.join(ROOT, "tests", "support", "pcoa_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pcoa_ref as pc  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ["C4", "bact20", "human8"]


def run(exe, args, timeout=120, env=None):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    return r.returncode, r.stdout, r.stderr


def direct(which, env=None):
    e = dict(os.environ)
    e.pop("PANGENE_PCOA_STEPS", None)
    e.update(env or {})
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=ROOT, env=e)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", NAMES)
def test_file_route(built, name):
    """`pangene pcoa -k 3` of the product on the fixture for gene / adj x jaccard / diff, and pg_pan_pcoa and pg_pan_pcoa_presence on the
    same matrices, against the reference (one child process: the device comes up once)"""
    direct("file:" + name)


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, name):
    """`pangene --pcoa *.paf` prints the bytes `pangene pcoa` prints for the GFA of the same run -- the same build and the same code, so
    this is the determinism rule -- and stands within the bounds"""
    direct("memory:" + name)


def test_refused_when_sharded(built):
    rc, out, err = run(HIP, ["--gpus", "2", "--pcoa"] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--pcoa" in err
    rc, out, err = run(HIP, ["pcoa", "-k", "17", os.path.join(GOLD, "C4.gfa.gz")])
    assert rc == 1 and out == b"" and b"-k" in err


def test_cap_on_the_command_line(built):
    """PANGENE_PCOA_STEPS=2 on bact20, which needs more: status 0, `converged 0`, the residuals in the table and a note on stderr"""
    rc, out, err = run(HIP, ["pcoa", os.path.join(GOLD, "bact20.gfa.gz")], env=dict(os.environ, PANGENE_PCOA_STEPS="2"))
    got = pc.of_text(out)
    assert rc == 0 and b"converged 0" in out and got["steps"] == 2 and got["axes"] == 2 and b"did not converge within 2 vectors" in err
    assert all(r > 1e-6 * got["eig"][0] for r in got["resid"])


def test_notes(built, tmp_path):
    """no distance above zero, and fewer than three assemblies: the # line, a note on stderr, no table"""
    from test_pcoa import check_notes
    check_notes(HIP, tmp_path)


@pytest.mark.parametrize("which", ["maps", "negative", "rank", "multiple", "slow", "cap", "magnitude", "twice", "range"])
def test_direct_cases(built, which):
    """pga_pan_pcoa and pg_pan_pcoa on matrices no GFA fixture reaches (tests/support/pcoa_direct.py).  maps: points in R^3 at N = 3, 4, 63,
    64, 65, 127, 129, 257, 513 and 1 025 -- the four columns of a lane, the 1 024 columns of a workgroup's pass, the four rows of a
    workgroup of k_pcoa_mult, the lanes and waves of the reductions -- with Y = B X for b = 1, 3, 8 columns through x_test against numpy
    within the dot-product bound, then the full result.  negative: twelve points on a line with the squared distance as the distance
    (l_min = -0.316 l_1: a solver that ranks by size fails); the matrix as stated rounds to l_2 = 3.7e-7 l_1, above the cut, so three
    axes come back there, and its exact variant ((i - j) / 16)^2 returns exactly one.  rank: two groups of identical points (one axis,
    at least one restart, finite), all-zero and N = 1, 2.  multiple: the regular simplex of six points, three equal eigenvalues.  slow: a
    random Jaccard matrix whose top three lie within 6 per cent (56 steps; the dropped coordinates' reference gaps are asserted).  cap:
    the same with PANGENE_PCOA_STEPS=6: converged 0 and every residual is |B v - theta v| of the returned vector within 1e-9 l_1.
    magnitude: N = 129, entries up to 2^29 - 1.  twice: bit-identical results twice, after a larger and a smaller call, and after the
    buffers were given back.  range: n = 16 385 and k = 17 and 0 are PGA_ERR_RANGE before any launch; k = N is clamped."""
    direct(which, {"PANGENE_PCOA_STEPS": "6"} if which == "cap" else None)
