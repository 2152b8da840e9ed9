"""Structure-adjusted association on the MI355X: the sums S = X . cols come from k_glm_sums on the fp64 matrix cores, V from k_glm_stat
(pga_pan_glm), the null fits, Z, p, q and lambda from the host code both builds share.  This is floating point: the product is compared
with the numpy restatement within the tolerances of tests/support/glm_ref.py, and with the checker build within the same bounds, never
byte for byte; only two runs of the same build are (the determinism rule).  With integer columns the sums are exact, and there the
product must equal numpy's integer product.  Every GPU step runs in a child process under a timeout of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
DIRECT = os.path.join(ROOT, "tests", "support", "glm_direct.py")

pytestmark = pytest.mark.gpu
NAMES = ["C4", "bact20", "human8"]


def run(exe, args, timeout=120, env=None):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    return r.returncode, r.stdout, r.stderr


def direct(which):
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, cwd=ROOT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", NAMES)
def test_file_route(built, name):
    """`pangene glm -k 0|3` of the product on the fixture with its binary and its quantitative trait file against the restatement"""
    direct("file:" + name)


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, name):
    """`pangene --glm=FILE *.paf` prints the bytes `pangene glm -t FILE` prints for the GFA of the same run -- the same build and the same
    code, so this is the determinism rule -- and stands within the bounds of the restatement"""
    direct("memory:" + name)


def test_refused_on_the_command_line(built):
    tsv = os.path.join(GOLD, "trait", "C4.tsv")
    rc, out, err = run(HIP, ["--gpus", "2", "--glm=" + tsv] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--glm" in err
    rc, out, err = run(HIP, ["glm", "-k", "14", "-t", tsv, os.path.join(GOLD, "C4.gfa.gz")])
    assert rc == 1 and out == b"" and b"-k" in err
    rc, out, err = run(HIP, ["glm", os.path.join(GOLD, "C4.gfa.gz")])
    assert rc == 1 and out == b"" and b"needs -t FILE" in err


@pytest.mark.parametrize("which", ["maps", "sums", "stat", "collinear", "separation", "na", "twice", "range"])
def test_direct_cases(built, which):
    """pga_pan_glm and pg_pan_glm on matrices no GFA fixture reaches (tests/support/glm_direct.py).  maps: columns of small integers
    (|v| <= 8) through sums_test at A = 3, 4, 5, 31, 32, 33, 63, 65, 129, 257, 1 025 and G = 1, 15, 16, 17, 63, 65, 255, 257, 1 000 -- every
    A with two G and every G with two A -- and T = 1, 2, 5: the sums EQUAL numpy's integer product (the f64 result map, the eight steps
    of a word, the tile edges, the trait tiles, the K segments), column 0 is the popcount of the valid bits, and a, U, s_w, V are exact.
    sums: the same shapes with normal columns within 4 A 2^-53 sum |cols_i|.  stat: k = 0, 1, 13 at A = 129, G = 257, both families: U, V,
    s_w against the restatement and against the checker build.  collinear: a covariate equal to a gene's row.  separation: a trait
    equal to the sign of the first covariate, through pg_pan_glm and on the command line (Fit 0, a note, no G lines).  na: dropping the
    assemblies without a value by hand gives the same numbers.  twice: bit-identical results twice, after a larger and a smaller call,
    and after the buffers were given back.  range: n_asm = 16 385, n_cov = 14, 2^24 genes are PGA_ERR_RANGE before any launch; an
    infinite value is PGA_ERR_ARG; no genes and no assemblies."""
    direct(which)
