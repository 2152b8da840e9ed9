"""Trees on the MI355X: the joins come from the HIP kernels of k_join.hpp (pga_pan_join).  The product must print and return what the
numpy restatement (tests/support/tree_ref.py) and the checker build (oracle backend: no pan_join entry, so the host loops of tree.cpp
-- a second implementation) print and return.  Every step runs in a child process under a timeout of its own."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HIP = os.path.join(ROOT, "pangene_amd", "bin", "pangene")
ORA = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
DIRECT = os.path.join(ROOT, "tests", "support", "tree_direct.py")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import dist_ref as dr  # noqa: E402
import tree_ref as tr  # noqa: E402

pytestmark = pytest.mark.gpu
GFAS = sorted(os.path.join(GOLD, f) for f in os.listdir(GOLD) if f.endswith(".gfa.gz")) + \
    sorted(os.path.join(GOLD, "bubble", f) for f in os.listdir(os.path.join(GOLD, "bubble")) if f.endswith(".gfa"))


def run(exe, args, timeout=300):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write("%s: exit %d, stderr: %s\n" % (" ".join(args[:4]), r.returncode, r.stderr.decode(errors="replace")[-2000:]))
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("gfa", GFAS, ids=[os.path.relpath(g, GOLD) for g in GFAS])
def test_file_route(built, gfa):
    for kind, metric in (("gene", "jaccard"), ("adj", "diff")):
        names, P = dr.presence(gfa, kind)
        S = dr.shared(P)
        for method in tr.METHODS:
            args = ["tree", "-t", kind, "-m", metric, "-a", method, gfa]
            rc, out, _ = run(HIP, args)
            assert rc == 0 and out == tr.text(names, S, metric, method), " ".join(args)
            rc, out2, _ = run(ORA, args)
            assert rc == 0 and out2 == out


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", ["C4", "bact20", "human8"])
def test_in_memory_route(built, tmp_path, name):
    """`pangene --tree *.paf` on the device: what the checker prints, and what `pangene tree` prints for the GFA of the same run"""
    files = _paf_dir(name)
    rc, gfa, _ = run(HIP, files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    for kind, method in (("gene", "nj"), ("adj", "upgma")):
        rc1, a, _ = run(HIP, ["--tree=" + kind, "--tree-method=" + method] + files)
        rc2, b, _ = run(HIP, ["tree", "-t", kind, "-a", method, str(tmp_path / "g.gfa")])
        rc3, c, _ = run(ORA, ["--tree=" + kind, "--tree-method=" + method] + files)
        assert rc1 == 0 and rc2 == 0 and rc3 == 0 and a == b == c and a.endswith(b";\n"), kind


def test_refused_when_sharded(built):
    rc, out, err = run(HIP, ["--gpus", "2", "--tree"] + _paf_dir("C4"))
    assert rc == 1 and out == b"" and b"--tree" in err


@pytest.mark.parametrize("which", ["sizes", "large", "cached", "equal", "presence", "parts", "signed"])
def test_direct_cases(built, which):
    """pg_pan_join on matrices no GFA fixture reaches, for both methods: sizes across the kernels' wave, tile and workgroup boundaries
    against the restatement, 1 025 and 2 049 against the checker build, a run of growing and shrinking sizes on the cached buffers,
    all-equal distances, pg_pan_tree from presence bytes, a search whose workgroups stride over several tiles, and (signed) entries of
    either sign up to 2^29 - 1, a run that peaks three below the range limit, and the device's own input flag through pga_pan_join
    (tests/support/tree_direct.py)"""
    r = subprocess.run([sys.executable, DIRECT, which], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and out.rstrip().endswith("ALL OK"), out[-3000:]
