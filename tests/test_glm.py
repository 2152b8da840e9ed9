"""Structure-adjusted association (`pangene glm`, `pangene --glm`, pg_pan_glm) through the checker build: the host driver linked against
the oracle backend, whose table has no pan_glm entry, so the sums come from the second implementation of pan_glm.hpp (the set bits
walked in fp64).  Everything is compared with the numpy restatement of tests/support/glm_ref.py within the tolerances stated there;
nothing is compared byte for byte."""
import math
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
import glm_ref as gr  # noqa: E402
import tree_ref as tr  # noqa: E402

NAMES = ["C4", "bact20", "human8"]
FAMILIES = [("binary", "trait"), ("quant", "qtrait")]
_cache = {}


def run_cli(args, exe=CLI, env=None):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)
    return r.returncode, r.stdout, r.stderr


def gfa_of(name):
    return os.path.join(GOLD, name + ".gfa.gz")


def matrices(gfa):
    """(assembly names, gene names, P (G, A), q, F) of a GFA file"""
    asm, P = dr.presence(gfa, "gene")
    q, F = tr.fixed(dr.shared(P), "jaccard")
    return list(asm), gr.gene_names(gfa), np.asarray(P, dtype=bool), q, F


def fixture(name):
    """the same of a fixture, computed once and left unchanged"""
    if name not in _cache:
        _cache[name] = matrices(gfa_of(name))
    return _cache[name]


def check_fixture(exe, name, family, folder, k, gfa=None, text=None):
    """`pangene glm` of `exe` on a fixture (or on `gfa`, a GFA of the fixture's run; or `text`, what a command printed for it, with its
    stderr) against the restatement: the list of what is wrong, and how many genes were compared"""
    asm, genes, P, q, F = fixture(name) if gfa is None else matrices(gfa)
    tsv = os.path.join(GOLD, folder, name + ".tsv")
    if text is None:
        rc, out, err = run_cli(["glm", "-t", tsv, "-y", family, "-k", str(k), gfa or gfa_of(name)], exe=exe)
        assert rc == 0, err
    else:
        out, err = text
    got = gr.parse(out)
    h = got["head"]
    assert h["items"] == "gene" and h["metric"] == "jaccard" and int(h["A"]) == len(asm) and int(h["Fbits"]) == F and h["family"] == family and int(h["converged"]) == 1
    take, lo, hi = gr.axes(q, F, k) if k else (None, 0, 0)
    n_axes = int(h["axes"])
    assert lo <= n_axes <= hi, (n_axes, lo, hi)
    cov, delta = take(n_axes) if k else (None, 0.0)
    tnames, vals = gr.read_traits(tsv, asm)
    refs = gr.reference(P, vals, cov, family, delta=min(delta, 1e-4))
    if delta > 1e-4:  # the span of the axes is not determined: only what does not hang on them
        for nm, ref in zip(tnames, refs):
            assert (nm in got["traits"]) == (not ref["skip"]) and (ref["skip"] or got["traits"][nm]["N"] == ref["N"])
        return [], 0
    assert got["kind"] == ("Cases" if family == "binary" else "Mean")
    bad = gr.check_text(got, tnames, genes, refs)
    for nm, ref in zip(tnames, refs):
        if not ref["skip"] and ref["clear"] and not ref["fit"]:
            assert ("Note: trait %s:" % nm).encode() in err
        if ref["skip"]:
            assert ("Note: trait %s has" % nm).encode() in err
    return bad, sum(len(ref["tested"]) for ref in refs if ref["fit"])


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    return oracle_host.load()


@pytest.mark.parametrize("k", [0, 3])
@pytest.mark.parametrize("family,folder", FAMILIES)
@pytest.mark.parametrize("name", NAMES)
def test_fixtures(built, name, family, folder, k):
    """`pangene glm -k 0|3` on the fixtures with their binary and quantitative trait files: the T and G lines against the restatement"""
    bad, compared = check_fixture(CLI, name, family, folder, k)
    assert not bad, bad[:10]
    if k == 0:
        assert compared > 0


def random_case(seed, G=120, A=57, k=2, na=6):
    rng = np.random.default_rng(seed)
    P = rng.random((G, A)) < rng.uniform(0.1, 0.9, size=(G, 1))
    cov = rng.standard_normal((A, k))
    yb = (rng.random(A) < 1.0 / (1.0 + np.exp(-(0.3 + 0.8 * cov[:, 0] if k else np.zeros(A))))).astype(np.float64)
    yq = rng.standard_normal(A) + (0.7 * cov[:, 0] if k else 0.0) + 0.9 * P[3]
    for y in (yb, yq):
        y[rng.choice(A, size=na, replace=False)] = np.nan
    return P, cov, yb, yq


def z_of(got, t):
    with np.errstate(divide="ignore", invalid="ignore"):
        return got["U"][t] / np.sqrt(got["V"][t])


def test_k0_binary_identity(ora):
    """without covariates the score test of a binary trait is the chi-square of the 2 x 2 table: Z^2 = N phi^2"""
    from pangene_amd import capi
    P, _, yb, _ = random_case(3, k=0)
    got = capi.pan_glm(ora, P, yb, None, "binary", 2)
    ref = gr.one_trait(P, yb, None, "binary", 2)
    assert got["fit"][0] == 1 and not gr.check_values(got, 0, ref)
    v = np.flatnonzero(~np.isnan(yb))
    N, t = len(v), int(yb[v].sum())
    z = z_of(got, 0)
    for i, g in enumerate(ref["tested"]):
        a, s = int(P[g, v].sum()), int((P[g, v] & (yb[v] > 0)).sum())
        phi2 = (s * N - a * t) ** 2 / (a * (N - a) * t * (N - t))
        assert abs(z[g] ** 2 - N * phi2) <= 2 * abs(z[g]) * ref["ez"][i] + ref["ez"][i] ** 2 + 1e-13 * (1 + N * phi2)
    assert len(ref["tested"]) > 50


def test_k0_quant_identity(ora):
    """without covariates the score test of a quantitative trait is the correlation test: Z^2 = (N - 1) r^2, r the Pearson correlation"""
    from pangene_amd import capi
    P, _, _, yq = random_case(4, k=0)
    got = capi.pan_glm(ora, P, yq, None, "quant", 2)
    ref = gr.one_trait(P, yq, None, "quant", 2)
    assert got["fit"][0] == 1 and not gr.check_values(got, 0, ref)
    v = np.flatnonzero(~np.isnan(yq))
    z = z_of(got, 0)
    for i, g in enumerate(ref["tested"]):
        r = np.corrcoef(P[g, v].astype(np.float64), yq[v])[0, 1]
        want = (len(v) - 1) * r * r
        assert abs(z[g] ** 2 - want) <= 2 * abs(z[g]) * ref["ez"][i] + ref["ez"][i] ** 2 + 1e-13 * (1 + want)
    assert len(ref["tested"]) > 50


@pytest.mark.parametrize("family", ["binary", "quant"])
def test_invariance(ora, family):
    """covariates Z M for a random invertible M, and sign flips, span the same space: the same U and V within the bounds"""
    from pangene_amd import capi
    P, cov, yb, yq = random_case(5, k=3)
    y = yb if family == "binary" else yq
    rng = np.random.default_rng(55)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    M = Q @ np.diag([0.5, 1.0, 2.0]) @ np.linalg.qr(rng.standard_normal((3, 3)))[0]
    base = capi.pan_glm(ora, P, y, cov, family)
    ref = gr.one_trait(P, y, cov, family)
    assert base["fit"][0] == 1 and not gr.check_values(base, 0, ref)
    for other in (cov @ M, cov * np.array([1.0, -1.0, -1.0])):
        got = capi.pan_glm(ora, P, y, other, family)
        ref2 = gr.one_trait(P, y, other, family)
        assert not gr.check_values(got, 0, ref2)
        el = ref["eligible"]
        assert np.array_equal(got["a"], base["a"])
        assert np.all(np.abs(got["U"][0] - base["U"][0])[el] <= (ref["eU"] + ref2["eU"])[el])
        assert np.all(np.abs(got["V"][0] - base["V"][0])[el] <= (ref["eV"] + ref2["eV"])[el])


@pytest.mark.parametrize("family", ["binary", "quant"])
def test_collinear(ora, family):
    """a covariate equal to a gene's own row: that gene is collinear (V <= 1e-8 s_w, here a factor 100 below), the others are tested"""
    from pangene_amd import capi
    P, cov, yb, yq = random_case(6, k=1, na=0)
    y = yb if family == "binary" else yq
    g = 7
    cov = np.hstack([cov, P[g][:, None].astype(np.float64)])
    got = capi.pan_glm(ora, P, y, cov, family)
    ref = gr.one_trait(P, y, cov, family)
    same = np.flatnonzero((P == P[g]).all(axis=1) | (P == ~P[g]).all(axis=1))
    assert ref["collinear"][g] and ref["margin"].all() and ref["clear"] and set(np.flatnonzero(ref["collinear"] & ref["eligible"])) == set(same)
    assert got["fit"][0] == 1 and got["V"][0][g] <= 1e-10 * got["s_w"][0][g] and got["a"][0][g] == P[g].sum()
    assert got["tested"][0] == int(ref["eligible"].sum()) - len(same) and not gr.check_values(got, 0, ref)


def test_separation(ora, built, tmp_path):
    """a binary trait equal to the sign of the first covariate: Fit 0, no values; on the command line a note and no G lines"""
    from pangene_amd import capi
    P, cov, _, _ = random_case(8, k=2, na=0)
    y = (cov[:, 0] > 0).astype(np.float64)
    ref = gr.one_trait(P, y, cov, "binary")
    assert ref["fit"] == 0 and ref["clear"]
    got = capi.pan_glm(ora, P, y, cov, "binary")
    assert got["fit"][0] == 0 and got["tested"][0] == 0 and np.all(got["a"] == -1) and not got["U"].any()
    check_separation_cli(CLI, tmp_path)


def check_separation_cli(exe, tmp_path):
    """the same through the command line: the trait is the sign of the first principal coordinate of bact20"""
    rc, out, err = run_cli(["pcoa", "-k", "1", gfa_of("bact20")], exe=exe)
    assert rc == 0
    pcs = [l.split("\t") for l in out.decode().split("\n") if l.startswith("PC\t") and not l.startswith("PC\tAsm")]
    tsv = tmp_path / "sign.tsv"
    tsv.write_text("asm\tside\n" + "".join("%s\t%d\n" % (f[1], float(f[2]) > 0) for f in pcs))
    rc, out, err = run_cli(["glm", "-t", str(tsv), "-k", "1", gfa_of("bact20")], exe=exe)
    got = gr.parse(out)
    assert rc == 0 and got["traits"]["side"]["fit"] == 0 and got["traits"]["side"]["tested"] == 0 and got["traits"]["side"]["lam"] is None
    assert not got["genes"] and b"Note: trait side:" in err


def test_planted_structure(ora):
    """two clades, 60 noisy clade markers, a trait driven by the clade and one planted gene: one axis of pg_pan_pcoa_presence as the
    covariate more than halves the markers' median |Z|, lambda falls, and the planted gene keeps |Z| > 4"""
    from pangene_amd import capi
    P, y, clade, markers, planted = gr.two_clades(1)
    pc, _ = capi.pan_pcoa_presence(ora, P, "jaccard", 1)
    assert pc["axes"] == 1 and abs(np.corrcoef(pc["coord"][:, 0], clade)[0, 1]) > 0.9
    cov = pc["coord"] / np.sqrt(pc["eig"] / P.shape[1])
    res = []
    for c in (None, cov):
        got = capi.pan_glm(ora, P, y, c, "binary")
        z = z_of(got, 0)
        ok = got["a"][0] >= 0
        assert got["fit"][0] == 1 and got["tested"][0] == ok.sum() and not gr.check_values(got, 0, gr.one_trait(P, y, c, "binary"))
        res.append((np.median(np.abs(z[markers])), np.median(z[ok] ** 2) / gr.CHI2_MEDIAN, abs(z[planted])))
    (m0, l0, p0), (m1, l1, p1) = res
    assert m1 < 0.5 * m0 and l1 < l0 and p0 > 4 and p1 > 4, res


@pytest.mark.parametrize("family", ["binary", "quant"])
def test_na_handling(ora, family):
    """an assembly without a value is a zero row of the columns: dropping those assemblies from the matrix by hand gives the same numbers"""
    from pangene_amd import capi
    P, cov, yb, yq = random_case(9, k=2, na=11)
    y = yb if family == "binary" else yq
    v = np.flatnonzero(~np.isnan(y))
    full = capi.pan_glm(ora, P, y, cov, family, 2)
    cut = capi.pan_glm(ora, P[:, v], y[v], cov[v], family, 2)
    ref, ref2 = gr.one_trait(P, y, cov, family, 2), gr.one_trait(P[:, v], y[v], cov[v], family, 2)
    assert full["N"][0] == len(v) == cut["N"][0] and np.array_equal(full["a"], cut["a"]) and full["tested"][0] == cut["tested"][0]
    assert not gr.check_values(full, 0, ref) and not gr.check_values(cut, 0, ref2)
    el = ref["eligible"]
    assert np.all(np.abs(full["U"][0] - cut["U"][0])[el] <= (ref["eU"] + ref2["eU"])[el]) and np.all(np.abs(full["V"][0] - cut["V"][0])[el] <= (ref["eV"] + ref2["eV"])[el])
    # a trait whose values all sit on NA but two, and one with one value only, are skipped: fit 0, no values
    few = np.full((2, P.shape[1]), np.nan)
    few[0, :4] = [0, 1, 0, 1]
    few[1, :30] = 1.0
    got = capi.pan_glm(ora, P, few, cov, "binary")
    assert list(got["N"]) == [4, 30] and not got["fit"].any() and np.all(got["a"] == -1)


def test_refusals(ora, built):
    from pangene_amd import capi
    gfa, tsv = gfa_of("C4"), os.path.join(GOLD, "trait", "C4.tsv")
    for args, word in ((["-k", "14", "-t", tsv], b"-k must be in [0, 13]"), (["-k", "-1", "-t", tsv], b"-k must be in [0, 13]"), ([], b"pangene glm needs -t FILE"),
                       (["-y", "count", "-t", tsv], b"-y must be binary or quant"), (["-T", "genes", "-t", tsv], b"-T must be gene or adj"),
                       (["-c", "0", "-t", tsv], b"-c must be at least 1")):
        rc, out, err = run_cli(["glm"] + args + [gfa])
        assert rc == 1 and out == b"" and word in err, (args, err)
    rc, out, err = run_cli(["glm"])
    assert rc == 0 and b"Usage: pangene glm" in out and b"one-step" in out and b"--glm=FILE" in out
    rc, out, err = run_cli(["glm", "-t", os.path.join(GOLD, "qtrait", "C4.tsv"), gfa])  # numbers under the binary family
    assert rc == 1 and out == b"" and b"is not 1, 0 or NA" in err
    pafs = sorted(os.path.join(GOLD, "C4", f) for f in os.listdir(os.path.join(GOLD, "C4")) if ".paf" in f)
    for args, word in ((["--gpus", "2", "--glm=" + tsv], b"--glm needs every genome in one process"), (["--glm-axes=2"], b"need --glm=FILE"),
                       (["--glm=" + tsv, "--glm-axes=14"], b"--glm-axes must be in [0, 13]"), (["--pcoa", "--glm=" + tsv], b"--glm cannot be combined with")):
        rc, out, err = run_cli(args + pafs)
        assert rc == 1 and out == b"" and word in err, (args, err)
    P, cov, yb, yq = random_case(10, k=1, na=0)
    with pytest.raises(RuntimeError, match="status -2"):
        capi.pan_glm(ora, np.zeros((1, 16385), dtype=bool), np.zeros(16385), None, "quant")
    with pytest.raises(RuntimeError, match="status -2"):
        capi.pan_glm(ora, P, yq, np.zeros((P.shape[1], 14)), "quant")
    for bad in (np.inf, -np.inf):
        y = yq.copy()
        y[5] = bad
        with pytest.raises(RuntimeError, match="status -3"):
            capi.pan_glm(ora, P, y, cov, "quant")
    c = cov.copy()
    c[3, 0] = np.nan
    with pytest.raises(RuntimeError, match="status -3"):
        capi.pan_glm(ora, P, yq, c, "quant")
    with pytest.raises(RuntimeError, match="status -3"):
        capi.pan_glm(ora, P, yq, cov, "binary")  # values that are not 0 or 1
    with pytest.raises(ValueError):
        capi.glm_opt(ora, n_axis=14)
    assert capi.glm_opt(ora, "quant", 0, "adj", "diff", 5, 2, 0.5).max_p == 0.5


def test_in_memory_route(built):
    """`pangene --glm=FILE` over the PAF files prints what `pangene glm -t FILE` prints for the GFA of the same run, byte for byte: the
    same build and the same code"""
    pafs = sorted(os.path.join(GOLD, "human8", f) for f in os.listdir(os.path.join(GOLD, "human8")) if ".paf" in f)
    tsv = os.path.join(GOLD, "qtrait", "human8.tsv")
    rc1, a, _ = run_cli(["--glm=" + tsv, "--glm-family=quant", "--glm-axes=1", "--glm-type=adj", "--glm-metric=diff", "--glm-seed=5", "--glm-min=2", "--glm-max-p=0.5"] + pafs)
    rc2, b, _ = run_cli(["glm", "-t", tsv, "-y", "quant", "-k", "1", "-T", "adj", "-m", "diff", "-s", "5", "-c", "2", "-p", "0.5", gfa_of("human8")])
    got = gr.parse(a)
    assert rc1 == 0 and rc2 == 0 and a == b and got["head"]["items"] == "adj" and got["head"]["metric"] == "diff" and got["genes"]
    assert all(v["z"] is None or v["p"] <= 0.5 * (1 + 1e-5) for v in got["genes"].values()) and all(min(v["a"], v["N"] - v["a"]) >= 2 for v in got["genes"].values())


def test_transcript_still_replays(built):
    """the recorded command lines of the older analyses print what they printed: glm joins the table without a change to usage() or to
    any message (tests/test_cli_transcript.py replays them; this is its replay through the same module)"""
    import oracle_host
    import test_cli_transcript as tc
    tc.test_the_list_covers_what_it_must()
    tc.test_replay(oracle_host.load())


def test_capi_run_reads_the_options(ora):
    """capi's table of the long options has the same rows as the command line's"""
    from pangene_amd import capi
    a, kw, side, o = capi._analysis_args(["--glm=x.tsv", "--glm-family=quant", "--glm-axes=0", "--glm-min=3", "--glm-max-p=0.01"], ora)
    assert a.name == "glm" and side == "x.tsv" and (o.family, o.n_axis, o.min_count, o.max_p) == (1, 0, 3, 0.01)
    with pytest.raises(ValueError, match="--glm-axes must be in"):
        capi._analysis_args(["--glm=x.tsv", "--glm-axes=14"], ora)
    assert math.isclose(capi.glm_opt(ora).max_p, 1.0)
