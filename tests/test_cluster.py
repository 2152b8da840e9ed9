"""Clusters of the assemblies (`pangene cluster`, `pangene --cluster`, pg_pan_medoids, pg_pan_cluster) through the checker build: the
host driver linked against the oracle backend, whose table has no pan_medoids entry, so k-medoids runs as the plain loops of tree.cpp.
Everything is compared with the numpy restatement of tests/support/cluster_ref.py, whose deltas are differences of two TDs."""
import ctypes as C
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
import cluster_ref as cr  # noqa: E402
import dist_ref as dr  # noqa: E402
import tree_ref as tr  # noqa: E402

GFAS = sorted(os.path.join(GOLD, f) for f in os.listdir(GOLD) if f.endswith(".gfa.gz")) + \
    sorted(os.path.join(GOLD, "bubble", f) for f in os.listdir(os.path.join(GOLD, "bubble")) if f.endswith(".gfa"))


def run_cli(args, exe=CLI):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.returncode, r.stdout, r.stderr


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    return oracle_host.load()


@pytest.mark.parametrize("gfa", GFAS, ids=[os.path.relpath(g, GOLD) for g in GFAS])
def test_fixture_files(built, gfa):
    for kind, metric in (("gene", "jaccard"), ("adj", "diff")):
        names, P = dr.presence(gfa, kind)
        if len(names) < 4:
            pytest.skip("fewer than 4 assemblies")
        S = dr.shared(P)
        args = ["cluster", "-t", kind, "-m", metric]
        rc, out, err = run_cli(args + ["-k", "2", gfa])
        assert rc == 0, err
        assert out == cr.text(names, S, metric, 2), kind
        rc, out, err = run_cli(args + ["-k", "2-4", gfa])
        if len(names) == 4:  # the range leaves [2, 3]: refused, and the range that fits is compared instead
            assert rc == 1 and out == b"" and b"k must be in [2, 3]" in err
            rc, out, err = run_cli(args + ["-k", "2-3", gfa])
            assert rc == 0 and out == cr.text(names, S, metric, 2, 3), kind
        else:
            assert rc == 0, err
            assert out == cr.text(names, S, metric, 2, 4), kind


def _matrix(n, seed):
    """planted for even seeds, without structure and with many ties for odd ones"""
    return cr.planted(n, 4, seed) if seed % 2 == 0 else cr.random_matrix(n, seed, hi=64)


@pytest.mark.parametrize("n", [3, 5, 17, 64, 100])
def test_pan_medoids_against_the_restatement(ora, n):
    from pangene_amd import capi
    swaps = 0
    for k in sorted({2, 3, n - 1} & set(range(2, n))):
        for seed in (0, 1):
            q = _matrix(n, 10 * n + seed)
            want = cr.medoids(q, k)
            assert want["converged"] == 1
            got = capi.pan_medoids(ora, q, k)
            assert cr.same(got, want), (n, k, seed)
            assert got["rec"].shape == (k + got["n_swap"], 3) and got["td"] == cr.td(q.astype(np.int64), list(got["medoid"]))
            swaps += got["n_swap"]
    assert swaps >= 1 or n == 3, "no input of this size needed a swap: pick other seeds"


def test_decomposition_is_exact():
    """removal + acc + plus against the difference of two TDs, on matrices with many tied and zero distances, after BUILD and after
    every swap, whichever of two equally near medoids is taken for the nearest"""
    for n, k, hi, seed in ((12, 2, 4, 1), (30, 5, 3, 2), (30, 29, 6, 3), (41, 7, 2, 4), (25, 4, 1 << 20, 5)):
        q = cr.random_matrix(n, seed, hi).astype(np.int64)
        if seed == 4:  # column 5 a copy of column 9: zero distance between two columns
            q[5], q[:, 5] = q[9].copy(), q[:, 9].copy()
            q[5, 5] = q[5, 9] = q[9, 5] = 0
        r = cr.medoids(q, k)
        M = [int(x) for x in r["rec"][:k, 0]]
        states = [list(M)]
        for x, m, _ in r["rec"][k:]:
            M[M.index(int(m))] = int(x)
            states.append(list(M))
        for M in states:
            cand, ms, want = cr.deltas(q, M)
            for last in (False, True):
                c2, m2, got = cr.decomposition(q, M, last)
                assert np.array_equal(c2, cand) and m2 == ms and np.array_equal(got, want), (n, k, last)


def test_all_equal_distances(ora):
    """every gain and every delta ties: BUILD takes 0, 1, .., k - 1, no swap lowers TD, and every other column goes to medoid 0"""
    from pangene_amd import capi
    for n, k in ((5, 2), (9, 4), (20, 19)):
        q = np.full((n, n), 3 << 18, dtype=np.int32)
        np.fill_diagonal(q, 0)
        got = capi.pan_medoids(ora, q, k)
        assert cr.same(got, cr.medoids(q, k))
        assert got["medoid"].tolist() == list(range(k)) and got["n_swap"] == 0 and got["converged"] == 1
        assert got["label"].tolist() == list(range(k)) + [0] * (n - k) and got["size"].tolist() == [n - k + 1] + [1] * (k - 1)


def test_identical_rows(ora):
    """copies of one assembly at distance 0 of each other: with more medoids than distinct rows some medoids are copies of others, and
    each still labels itself, so no cluster is empty"""
    from pangene_amd import capi
    base = cr.planted(4, 2, 3)
    idx = np.array([0, 0, 0, 1, 1, 2, 3, 3, 0, 1])
    q = base[np.ix_(idx, idx)].astype(np.int32)
    for k in (2, 4, 6, 9):
        got = capi.pan_medoids(ora, q, k)
        assert cr.same(got, cr.medoids(q, k)), k
        assert (got["size"] >= 1).all() and got["label"][got["medoid"]].tolist() == list(range(k))
    P = tr.lineage_presence(300, 12, 2, dup=0.6)
    for metric in tr.METRICS:
        qq, F = tr.fixed(dr.shared(P), metric)
        assert ((qq == 0).sum() - 12) >= 2, "the input has no copies"
        got, F2 = capi.pan_cluster(ora, P, 7, metric)
        assert F2 == F and cr.same(got, cr.medoids(qq, 7)) and (got["size"] >= 1).all()


# an input without structure whose restatement swaps 4 times at k = 5 (the default limit of 1 000 is never near)
SWAPPY = (60, 5, 11)


def test_iteration_limits(ora):
    from pangene_amd import capi
    n, k, seed = SWAPPY
    q = cr.random_matrix(n, seed)
    full = cr.medoids(q, k)
    assert full["converged"] == 1 and full["n_swap"] >= 2, full["n_swap"]
    assert cr.same(capi.pan_medoids(ora, q, k), full)
    got = capi.pan_medoids(ora, q, k, max_iter=0)  # BUILD only
    assert got["n_swap"] == 0 and got["converged"] == 0 and got["rec"].shape == (k, 3) and np.array_equal(got["rec"], full["rec"][:k])
    assert cr.same(got, cr.medoids(q, k, 0))
    got = capi.pan_medoids(ora, q, k, max_iter=1)
    assert got["n_swap"] == 1 and got["converged"] == 0 and cr.same(got, cr.medoids(q, k, 1))
    got = capi.pan_medoids(ora, q, k, max_iter=full["n_swap"])  # every iteration swapped: convergence was never seen
    assert got["converged"] == 0 and np.array_equal(got["rec"], full["rec"])
    assert capi.pan_medoids(ora, q, k, max_iter=full["n_swap"] + 1)["converged"] == 1


def test_not_converged_is_reported(built, tmp_path):
    rc, out, err = run_cli(["cluster", "-k", "2-3", "-i", "0", os.path.join(GOLD, "bact20.gfa.gz")])
    names, P = dr.presence(os.path.join(GOLD, "bact20.gfa.gz"), "gene")
    assert rc == 0 and out == cr.text(names, dr.shared(P), "jaccard", 2, 3, max_iter=0)
    assert err.count(b"did not converge") == 2 and out.splitlines()[1].endswith(b"\t0\t0")


def test_argument_and_range_errors(ora):
    from pangene_amd import capi
    q = cr.random_matrix(6, 1)
    for n, k, it in ((2, 2, 10), (6, 1, 10), (6, 6, 10), (6, 2, -1)):
        with pytest.raises(RuntimeError, match="status -3"):  # PGA_ERR_ARG
            capi.pan_medoids(ora, q[:n, :n], k, it)
    for i, j, v in ((0, 1, -1), (2, 2, 1), (1, 3, 5)):  # negative, diagonal, asymmetric
        bad = q.copy()
        bad[i, j] = v
        if v == -1:
            bad[j, i] = v
        with pytest.raises(RuntimeError, match="status -3"):
            capi.pan_medoids(ora, bad, 2)
    big = q.copy()
    big[0, 1] = big[1, 0] = 1 << 29
    with pytest.raises(RuntimeError, match="status -2"):  # PGA_ERR_RANGE
        capi.pan_medoids(ora, big, 2)
    big[0, 1] = big[1, 0] = (1 << 29) - 1
    assert cr.same(capi.pan_medoids(ora, big, 2), cr.medoids(big, 2))
    wide = np.zeros((1100, 1100), dtype=np.int32)
    with pytest.raises(RuntimeError, match="status -2"):  # k > 1 024
        capi.pan_medoids(ora, wide, 1025)
    with pytest.raises(ValueError):
        capi.pan_cluster(ora, np.ones((5, 4), dtype=bool), 2, "shared")
    with pytest.raises(RuntimeError, match="status -3"):
        capi.pan_cluster(ora, np.ones((5, 2), dtype=bool), 2)


def test_too_many_assemblies_is_a_range_error(ora):
    """n > 65 535 is refused on its size alone: the matrix behind the pointer is never read (one row is all that is there)"""
    row = np.zeros(65536, dtype=np.int32)
    outs = [np.zeros(4, dtype=np.int32) for _ in range(4)] + [np.zeros(4, dtype=np.int64) for _ in range(2)]
    n_rec, n_swap, conv, td = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
    p32, p64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    rc = ora.pg_pan_medoids(row.ctypes.data_as(p32), 65536, 2, 1, *[a.ctypes.data_as(p32) for a in outs[:4]], *[a.ctypes.data_as(p64) for a in outs[4:]], 1,
                            C.byref(n_rec), C.byref(n_swap), C.byref(td), C.byref(conv))
    assert rc == -2


def test_option_struct(ora):
    from pangene_amd import capi
    o = capi.cluster_opt(ora)
    assert (o.type, o.metric, o.k_lo, o.k_hi, o.max_iter) == (0, 0, 2, 2, 1000) and C.sizeof(capi.pg_cluster_opt_t) == 20
    o = capi.cluster_opt(ora, 3, 6, "adj", "diff", 5)
    assert (o.type, o.metric, o.k_lo, o.k_hi, o.max_iter) == (1, 2, 3, 6, 5)
    for kw in ({"k_lo": 1}, {"k_lo": 4, "k_hi": 3}, {"metric": "shared"}, {"max_iter": -1}):
        with pytest.raises(ValueError):
            capi.cluster_opt(ora, **kw)


def _paf_dir(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.mark.parametrize("name", ["C4", "bact20", "human8"])
def test_in_memory_route_equals_file_route(built, tmp_path, name):
    files = _paf_dir(name)
    rc, gfa, _ = run_cli(files)
    assert rc == 0
    (tmp_path / "g.gfa").write_bytes(gfa)
    n = len(dr.presence(str(tmp_path / "g.gfa"), "gene")[0])
    rng = "2-%d" % min(4, n - 1)
    for kind, metric in (("gene", "jaccard"), ("adj", "diff")):
        rc1, a, _ = run_cli(["--cluster=" + rng, "--cluster-type=" + kind, "--cluster-metric=" + metric] + files)
        rc2, b, _ = run_cli(["cluster", "-t", kind, "-m", metric, "-k", rng, str(tmp_path / "g.gfa")])
        assert rc1 == 0 and rc2 == 0 and a == b and a.startswith(b"#K\tk\tTD"), kind
    rc, d, _ = run_cli(["--cluster=2", "--cluster-iter=3"] + files)
    assert rc == 0 and d == run_cli(["cluster", "-k", "2", "-i", "3", str(tmp_path / "g.gfa")])[1]


def test_python_run_equals_command_line(ora):
    from pangene_amd import capi
    files = _paf_dir("bact20")
    args = ["--cluster=2-5", "--cluster-type=adj", "--cluster-metric=diff"]
    assert capi.run(ora, files, args) == run_cli(args + files)[1]
    for bad in (["--cluster=1"], ["--cluster=4-3"], ["--cluster=x"], ["--cluster-iter=5"], ["--cluster=2", "--tree"], ["--cluster=2", "--cluster-metric=shared"],
                ["--cluster"], ["--cluster=2", "--cluster-type"], ["--cluster=2", "--cluster-rows=3"]):
        with pytest.raises(ValueError):
            capi.run(ora, files, bad)
    for k in ("20", "50", "2-50"):  # 20 assemblies: k in [2, 19]
        with pytest.raises(RuntimeError, match="pg_write_cluster"):
            capi.run(ora, files, ["--cluster=" + k])
    assert capi.run(ora, files, ["--cluster=19"]).count(b"\nC\t") == 19


def test_refusals(built, tmp_path):
    files = _paf_dir("C4")
    rc, out, err = run_cli(["--gpus", "2", "--cluster=2"] + files)
    assert rc == 1 and out == b"" and b"--cluster" in err
    for extra in (["--matrix"], ["--call"], ["--curves"], ["--dist"], ["--assoc"], ["--trait=x"], ["--tree"], ["--qtrait=x"]):
        rc, out, err = run_cli(["--cluster=2"] + extra + files)
        assert rc == 1 and out == b"" and b"--cluster" in err, extra
    for alone in (["--cluster-type=adj"], ["--cluster-metric=diff"], ["--cluster-iter=5"]):
        rc, out, err = run_cli(alone + files)
        assert rc == 1 and out == b"" and b"need --cluster" in err
    for bad in (["--cluster=1"], ["--cluster=3-2"], ["--cluster=2-"], ["--cluster=-3"], ["--cluster=2", "--cluster-metric=shared"], ["--cluster=2", "--cluster-type=x"],
                ["--cluster=2", "--cluster-iter=-1"]):
        rc, out, err = run_cli(bad + files)
        assert rc == 1 and out == b"" and err != b"", bad
    n4 = len(dr.presence(os.path.join(GOLD, "C4.gfa.gz"), "gene")[0])
    for k in (str(n4), "50", "2-50", "2-%d" % n4):  # the in-memory route: a k or a range outside [2, assemblies - 1]
        rc, out, err = run_cli(["--cluster=" + k] + files)
        assert rc == 1 and out == b"" and b"k must be in [2, %d]" % (n4 - 1) in err, k
    rc, out, err = run_cli(["--cluster=2"] + files[:2])  # and fewer than 3 assemblies
    assert rc == 1 and out == b"" and b"at least 3 assemblies" in err
    g = os.path.join(GOLD, "bact20.gfa.gz")  # 20 assemblies: k in [2, 19]
    for bad in (["-k", "1"], ["-k", "20"], ["-k", "2-20"], ["-k", "5-4"], ["-k", "0-3"], ["-k", "x"], ["-k", "2", "-m", "shared"], ["-k", "2", "-t", "x"], ["-k", "2", "-i", "-1"], []):
        rc, out, err = run_cli(["cluster"] + bad + [g])
        assert rc == 1 and out == b"" and err != b"", bad
    rc, out, _ = run_cli(["cluster", "-k", "19", g])
    assert rc == 0 and out.count(b"\nC\t") == 19
    hand = "S\tg1\t*\tLN:i:1\nS\tg2\t*\tLN:i:1\nS\tg3\t*\tLN:i:1\n"
    two = tmp_path / "two.gfa"
    two.write_text(hand + "W\ts1\t0\tc1\t0\t3\t>g1>g2>g3\nW\ts2\t1\tc1\t0\t3\t>g1>g2\n")
    rc, out, err = run_cli(["cluster", "-k", "2", str(two)])
    assert rc == 1 and out == b"" and b"at least 3 assemblies" in err
    rc, out, _ = run_cli(["cluster", "-k", "2", str(tmp_path / "none.gfa")])
    assert rc == 1 and out == b""


def test_usage(built):
    rc, out, _ = run_cli(["cluster"])
    assert rc == 0 and out.startswith(b"Usage: pangene cluster -k INT[-INT] [options] <in.gfa>\n") and b"mean silhouette" in out
    rc, _, err = run_cli([])
    assert b"pangene cluster [-t gene|adj]" in err and b"--cluster=INT[-INT]" in err


def test_magnitude_inputs(ora):
    """the matrices of the `magnitude` GPU cases (cluster_ref.magnitude_inputs): entries up to 2^29 - 1, td, sums and gains beyond 2^32, the largest of them beyond 2^35 (2^37 from n = 513 on),
    the swaps the structured ones were built for, a lane's share of one gain beyond 2^31; the checker build gives what the restatement
    gives"""
    from pangene_amd import capi
    inputs = cr.magnitude_inputs()
    assert [(q.shape[0], k) for _, q, k, _ in inputs] == list(cr.MAGNITUDE_RANDOM) + [c[:2] for c in cr.MAGNITUDE_PLANTED]
    for label, q, k, swaps in inputs:
        n = q.shape[0]
        assert n >= 257 and np.array_equal(q, q.T) and not np.diag(q).any() and 1 << 28 < int(q.max()) < cr.LIMIT
        if label == "uniform":
            assert int(q[~np.eye(n, dtype=bool)].min()) >= 1 << 28
        want = cr.medoids(q, k)
        assert want["converged"] == 1 and (swaps is None or want["n_swap"] >= swaps), (label, n, k, want["n_swap"])
        sizes = (int(want["td"]), int(want["sums"].max()), int(want["rec"][0, 2]))
        assert min(sizes) > 1 << 32 and max(sizes) > 1 << (37 if n >= 513 else 35), (label, n, k, sizes)
        assert cr.same(capi.pan_medoids(ora, q, k), want), (label, n, k)
    assert sum(w["n_swap"] for w in (cr.medoids(q, k) for label, q, k, _ in inputs if label == "planted")) >= 6
    assert cr.first_gain_parts(inputs[-1][1]) >= 1 << 31
    n, k = cr.MAGNITUDE_CHECKER
    q = cr.full_random(n, n + k)
    assert cr.same(capi.pan_medoids(ora, q, k), cr.medoids(q, k))
