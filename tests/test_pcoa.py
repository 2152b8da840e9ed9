"""Principal coordinates (`pangene pcoa`, `pangene --pcoa`, pg_pan_pcoa) through the checker build: the host driver linked against the
oracle backend, whose table has no pan_pcoa entry, so the eigenpairs come from the second implementation of pan_pcoa.hpp (cyclic Jacobi
on the dense matrix).  Everything is compared with the numpy restatement of tests/support/pcoa_ref.py within the tolerances stated
there; nothing is compared byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.path.join(ROOT, "tests", "_build", "pangene_oraclehost")
sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
sys.path.insert(0, ROOT)
import dist_ref as dr  # noqa: E402
import pcoa_ref as pc  # noqa: E402
import tree_ref as tr  # noqa: E402

NAMES = ["C4", "bact20", "human8"]
SPECS = [("gene", "jaccard"), ("gene", "diff"), ("adj", "jaccard"), ("adj", "diff")]
_cache = {}


def run_cli(args, exe=CLI, env=None):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)
    return r.returncode, r.stdout, r.stderr


def gfa_of(name):
    return os.path.join(GOLD, name + ".gfa.gz")


def fixed(name, kind, metric):
    """(assembly names, q, F, the reference) of a fixture, computed once and left unchanged"""
    if (name, kind, metric) not in _cache:
        asm, P = dr.presence(gfa_of(name), kind)
        q, F = tr.fixed(dr.shared(P), metric)
        _cache[name, kind, metric] = (list(asm), q, F, pc.reference(q, F))
    return _cache[name, kind, metric]


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    return oracle_host.load()


@pytest.mark.parametrize("kind,metric", SPECS)
@pytest.mark.parametrize("name", NAMES)
def test_file_route(built, name, kind, metric):
    """`pangene pcoa -k 3` on the fixtures: eigenvalues, coordinates under the gap rule, residuals, orthogonality, the exact trace,
    Explained and Cumulative, within the bounds of pcoa_ref plus 5e-6 for the text"""
    asm, q, F, ref = fixed(name, kind, metric)
    rc, out, err = run_cli(["pcoa", "-t", kind, "-m", metric, "-k", "3", gfa_of(name)])
    assert rc == 0, err
    got = pc.of_text(out)
    assert got["names"] == asm and got["N"] == len(asm) and got["Fbits"] == F and got["converged"] == 1
    assert pc.parse(out)["head"]["items"] == kind and pc.parse(out)["head"]["metric"] == metric
    bad, compared = pc.check(q, F, got, 3, text=True, ref=ref)
    assert not bad, bad
    tr_ = float(pc.trace_exact(q, F))
    assert np.allclose(got["expl"], got["eig"] / tr_, atol=5.1e-5 + 1e-5) and np.allclose(got["cum"], np.cumsum(got["eig"] / tr_), atol=5.1e-5 + 3e-5)
    w = ref[1]
    if name in ("bact20", "human8") and metric == "jaccard" and kind == "gene":
        assert compared == [0, 1, 2]  # their top three are well separated: every coordinate was compared
    if (name, kind, metric) == ("C4", "gene", "diff"):
        assert got["axes"] == 1  # rank 1: one axis comes back
    if (name, kind, metric) == ("C4", "gene", "jaccard"):
        assert got["axes"] >= 2 and 1 not in compared and w[1] < 1e-4 * w[0]  # nearly rank 1: axis 2 is printed, its coordinates fall under the gap rule


@pytest.mark.parametrize("name", NAMES)
def test_pg_pan_pcoa(ora, name):
    """capi.pan_pcoa and capi.pan_pcoa_presence in the checker build on the fixtures' matrices: the same bounds without the text's share"""
    from pangene_amd import capi
    for kind, metric in SPECS:
        asm, q, F, ref = fixed(name, kind, metric)
        got = capi.pan_pcoa(ora, q, F, 3)
        bad, _ = pc.check(q, F, got, 3, ref=ref)
        assert not bad and got["converged"] == 1, (kind, metric, bad)
    _, P = dr.presence(gfa_of(name), "gene")
    _, q, F, ref = fixed(name, "gene", "jaccard")
    got, F2 = capi.pan_pcoa_presence(ora, np.asarray(P) != 0, "jaccard", 3)
    bad, _ = pc.check(q, F, got, 3, ref=ref)
    assert F2 == F and not bad, bad


def test_negative_eigenvalues_are_no_axes(built):
    """The fixtures are not Euclidean: the reference has eigenvalues well below zero (C4 adj:diff reaches -0.09 l_1), and the axes are the
    algebraically largest ones -- a pick by size would put such a value among the first three of C4 adj:diff or be caught by the bounds"""
    _, q, F, (B, w, v) = fixed("C4", "adj", "diff")
    assert w[-1] < -0.05 * w[0]
    rc, out, err = run_cli(["pcoa", "-t", "adj", "-m", "diff", "-k", "16", gfa_of("C4")])
    got = pc.of_text(out)
    assert rc == 0 and np.all(got["eig"] > 0) and np.all(np.diff(got["eig"]) <= 0)
    bad, _ = pc.check(q, F, got, 16, text=True, ref=(B, w, v))
    assert not bad, bad


def test_at_most_n_minus_one_axes(built):
    """human8 with -k 7: seven is N - 1, the whole centred subspace; what comes back is at most that and passes the bounds"""
    asm, q, F, ref = fixed("human8", "gene", "jaccard")
    rc, out, err = run_cli(["pcoa", "-k", "7", gfa_of("human8")])
    got = pc.of_text(out)
    assert rc == 0 and len(asm) == 8 and got["axes"] <= 7
    bad, _ = pc.check(q, F, got, 7, text=True, ref=ref)
    assert not bad, bad
    rc, out, err = run_cli(["pcoa", "-k", "16", gfa_of("human8")])  # above N - 1: clamped
    assert rc == 0 and pc.of_text(out)["axes"] <= 7


def test_eigenvalues_sum_to_the_exact_trace(ora):
    """The float side against the exact integer trace on bact20: the sum of ALL N - 1 eigenvalues is trace(B) = T / (2 N) 4^-F within
    1e-9 l_1 N.  The interface returns at most 16 axes and bact20 has 19, so the 16 returned values stand in for the reference's first 16
    and the reference's last three complete the sum; the reference's own sum is held to the same bound."""
    from pangene_amd import capi
    _, q, F, (B, w, v) = fixed("bact20", "gene", "jaccard")
    N = len(q)
    got = capi.pan_pcoa(ora, q, F, 16)
    tr_ = float(pc.trace_exact(q, F))
    assert N == 20 and got["axes"] == 16 and got["trace"] == pytest.approx(tr_, rel=2e-15)
    assert abs(w.sum() - tr_) <= 1e-9 * w[0] * N
    assert abs(got["eig"].sum() + w[16:].sum() - got["trace"]) <= 1e-9 * w[0] * N


def test_command_line_messages(built):
    gfa = gfa_of("C4")
    for args, word in ((["-k", "0"], b"-k must be in [1, 16]"), (["-k", "17"], b"-k must be in [1, 16]"), (["-k", "x"], b"-k must be in [1, 16]"),
                       (["-t", "genes"], b"-t must be gene or adj"), (["-m", "shared"], b"-m must be jaccard or diff")):
        rc, out, err = run_cli(["pcoa"] + args + [gfa])
        assert rc == 1 and out == b"" and word in err, (args, err)
    rc, out, err = run_cli(["pcoa"])
    assert rc == 0 and b"Usage: pangene pcoa" in out and b"overstate" in out and b"--pcoa[=INT]" in out
    rc, out, err = run_cli(["pcoa", "/nonexistent.gfa"])
    assert rc == 1 and out == b""
    pafs = sorted(os.path.join(GOLD, "C4", f) for f in os.listdir(os.path.join(GOLD, "C4")) if ".paf" in f)
    for args, word in ((["--pcoa=17"], b"--pcoa must be in [1, 16]"), (["--pcoa-type=x", "--pcoa"], b"--pcoa-type must be gene or adj"),
                       (["--pcoa-metric=jaccard"], b"need --pcoa"), (["--phylosig", "--pcoa"], b"--pcoa cannot be combined with"),
                       (["--gpus", "2", "--pcoa"], b"--pcoa needs every genome in one process")):
        rc, out, err = run_cli(args + pafs)
        assert rc == 1 and out == b"" and word in err, (args, err)


def test_in_memory_route(built):
    """`pangene --pcoa=2 --pcoa-type=adj` over the PAF files prints what `pangene pcoa -k 2 -t adj` prints for the GFA of the same run,
    byte for byte: the same build and the same code"""
    pafs = sorted(os.path.join(GOLD, "human8", f) for f in os.listdir(os.path.join(GOLD, "human8")) if ".paf" in f)
    rc1, a, _ = run_cli(["--pcoa=2", "--pcoa-type=adj"] + pafs)
    rc2, b, _ = run_cli(["pcoa", "-k", "2", "-t", "adj", gfa_of("human8")])
    assert rc1 == 0 and rc2 == 0 and a == b and pc.of_text(a)["axes"] == 2


def test_refused_matrices(ora):
    """capi.pan_pcoa turns away a matrix that is not symmetric or has a diagonal entry (PGA_ERR_ARG, -3), an entry of 2^29 (PGA_ERR_RANGE,
    -2) and an axis count outside 1 .. 16 (-2)"""
    from pangene_amd import capi
    q = np.array([[0, 5, 7], [5, 0, 9], [7, 9, 0]], dtype=np.int32) << 10
    assert capi.pan_pcoa(ora, q, 20, 2)["axes"] == 2
    for change, status in (((0, 1, 6 << 10), "-3"), ((1, 1, 1), "-3"), ((0, 2, -1), "-3"), ((0, 2, 1 << 29), "-2")):
        m = q.copy()
        i, j, v = change
        m[i, j] = v
        if v == 1 << 29 or v == -1:
            m[j, i] = v
        with pytest.raises(RuntimeError, match="status " + status):
            capi.pan_pcoa(ora, m, 20, 2)
    for k in (0, 17):
        with pytest.raises(RuntimeError, match="status -2"):
            capi.pan_pcoa(ora, q, 20, k)


def test_nothing_to_plot(ora, built, tmp_path):
    """fewer than three assemblies, or no distance above zero: no axes, and on the command line a note and no table"""
    from pangene_amd import capi
    for n in (0, 1, 2):
        q = (1 - np.eye(n, dtype=np.int32)) << 20
        assert capi.pan_pcoa(ora, q, 20, 3)["axes"] == 0
    got = capi.pan_pcoa(ora, np.zeros((5, 5), dtype=np.int32), 20, 3)
    assert got["axes"] == 0 and got["trace"] == 0.0
    got, F = capi.pan_pcoa_presence(ora, np.ones((7, 4), dtype=bool), "jaccard", 2)  # four identical assemblies
    assert got["axes"] == 0 and F == 20
    check_notes(CLI, tmp_path)


HAND = "S\tg1\t*\tLN:i:1\nS\tg2\t*\tLN:i:1\nS\tg3\t*\tLN:i:1\n"
WALKS = ["W\ts1\t0\tc1\t0\t3\t>g1>g2>g3\n", "W\ts2\t0\tc1\t0\t3\t>g1>g2<g3\n", "W\ts3\t0\tc1\t0\t3\t<g3<g2<g1\n"]


def check_notes(exe, tmp_path):
    """three assemblies with the same genes: no distance above zero; one and two assemblies: fewer than 3 -- the # line, a note, status 0"""
    for n, note in ((3, b"Note: no distance above zero over the 3 assemblies"), (2, b"Note: fewer than 3 assemblies over the 2 assemblies"),
                    (1, b"Note: fewer than 3 assemblies over the 1 assemblies")):
        g = tmp_path / ("w%d.gfa" % n)
        g.write_text(HAND + "".join(WALKS[:n]))
        rc, out, err = run_cli(["pcoa", str(g)], exe=exe)
        assert rc == 0 and note in err and out.count(b"\n") == 1 and out.startswith(b"#\titems gene\t") and b"\tN %d\t" % n in out, (n, out, err)
