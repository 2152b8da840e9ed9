"""Phylogenetic signal (`pangene phylosig`, `pangene --phylosig`, pg_pan_phylosig) through the checker build: the host driver linked
against the oracle backend, whose table has no pan_phylosig entry, so the permutation step comes from the plain loops of
pan_phylosig.hpp over the tree records.  Everything is compared with the numpy restatement of tests/support/phylosig_ref.py, and that
with a brute force over all inner-node assignments on every tree shape of 2 .. 8 leaves."""
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
import curves_ref  # noqa: E402
import pairs_ref as pr  # noqa: E402
import phylosig_ref as ps  # noqa: E402

NAMES = ["C4", "bact20", "human8"]
COSTS = ((1, 1), (2, 1), (1, 3))
EARLIER = ("matrix", "call", "curves", "dist", "assoc", "trait", "tree", "qtrait", "cluster", "permanova", "mantel", "gainloss", "coevo")


def run_cli(args, exe=CLI):
    r = subprocess.run([exe] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    return r.returncode, r.stdout, r.stderr


def gfa_of(name):
    return os.path.join(GOLD, name + ".gfa.gz")


def pafs_of(name):
    d = os.path.join(GOLD, name)
    return sorted(os.path.join(d, f) for f in os.listdir(d) if ".paf" in f)


@pytest.fixture(scope="module")
def ora(built):
    import oracle_host
    lib = oracle_host.load()
    C.c_int.in_dll(lib, "pg_verbose").value = 0
    return lib


def random_records(rng, A):
    """upgma-shaped records of a random rooted tree: any two live slots are joined"""
    live, rec = list(range(A)), []
    while len(live) > 1:
        i, j = (int(v) for v in rng.choice(live, size=2, replace=False))
        rec.append((i, j, 0, 0, 0, len(live)))
        live.remove(j)
    return np.array(rec, dtype=np.int64).reshape(-1, 6)


@pytest.fixture(scope="module")
def wanted():
    """the restatement's table per (fixture, option set), computed once"""
    return {(name, i): ps.table(gfa_of(name), **kw) for name in NAMES for i, kw in enumerate(ps.OPTION_SETS)}


@pytest.mark.parametrize("name", NAMES)
def test_file_route(built, wanted, name):
    """the whole text of the table against the restatement for the five option sets, and -p 0.05 as a filter of the default"""
    for i, kw in enumerate(ps.OPTION_SETS):
        rc, out, err = run_cli(["phylosig"] + ps.option_args(**kw)[0] + [gfa_of(name)])
        assert rc == 0, err
        assert out == wanted[name, i], (kw, out[:300], wanted[name, i][:300])
        assert out.startswith(ps.HEADER)
    rc, out, err = run_cli(["phylosig", gfa_of(name)])  # the defaults without any option
    assert rc == 0 and out == wanted[name, 0]
    assert out.count(b"\n") > 1 or name == "C4"
    rc, flt, err = run_cli(["phylosig", "-p", "0.05", gfa_of(name)])
    assert rc == 0 and flt == ps.table(gfa_of(name), max_p=0.05)
    lines = out.split(b"\n")[1:-1]  # the same filter over the integer columns of the default table: p = (1 + n) / (1 + P)
    keep = [ln for ln in lines if min((1.0 + int(ln.split(b"\t")[6])) / 1001.0, (1.0 + int(ln.split(b"\t")[7])) / 1001.0) <= 0.05]
    assert flt == ps.HEADER + b"".join(ln + b"\n" for ln in keep)


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, ora, wanted, tmp_path, name):
    """`pangene --phylosig ... *.paf` prints what `pangene phylosig` prints for the GFA of the same run, and what the restatement does;
    capi.run() gives the same bytes as the binary"""
    from pangene_amd import capi
    files = pafs_of(name)
    rc, gfa, err = run_cli(files)
    assert rc == 0, err
    path = str(tmp_path / "g.gfa")
    with open(path, "wb") as f:
        f.write(gfa)
    for kw in ps.OPTION_SETS:
        sub, long = ps.option_args(**kw)
        rc1, a, err = run_cli(long + files)
        rc2, b, _ = run_cli(["phylosig"] + sub + [path])
        assert rc1 == 0 and rc2 == 0, err
        assert a == b == ps.table(path, **kw), kw
        assert capi.run(ora, files, long) == a, kw
    rc, a, _ = run_cli(["--phylosig"] + files)
    assert rc == 0 and a == ps.table(path)
    rc, b, _ = run_cli(["--phylosig=50", "--phylosig-seed=7", "--phylosig-min=1"] + files)
    assert rc == 0 and b == ps.table(path, **ps.OPTION_SETS[3])


@pytest.mark.parametrize("name", NAMES)
def test_pg_pan_phylosig_on_the_fixtures(ora, name):
    """pg_pan_phylosig over the fixture's gene matrix and pg_pan_tree's records: the restatement's arrays, for the five option sets"""
    from pangene_amd import capi
    import gainloss_ref as gr
    names, _, P = gr.items(gfa_of(name), "gene")
    A = len(names)
    for kw in ps.OPTION_SETS:
        method = kw.get("method", "upgma")
        rec = gr.records(P, kw.get("metric", "jaccard"), method)
        kids = pr.tree(rec, A, method)
        k = dict(g=kw.get("g", 1), l=kw.get("l", 1), n_perm=kw.get("n_perm", 1000), seed=kw.get("seed", 11), min_count=kw.get("min_count", 2))
        got = capi.pan_phylosig(ora, P, rec, method, k["g"], k["l"], k["n_perm"], k["seed"], k["min_count"])
        assert ps.same(got, ps.pan_phylosig(P, kids, **k)), kw


def test_orders_are_the_pinned_ones():
    """the restatement's two forms of fisher_yates_order agree with each other and with the order every other restatement uses"""
    for A, seed in ((1, 11), (2, 11), (7, 3), (65, 11), (300, 0xFFFFFFFF)):
        o = ps.orders(A, seed, 1, 5)
        for q in range(5):
            assert o[:, q].tolist() == ps.fisher_yates_order(A, seed, 1 + q) == curves_ref.order(A, 1 + q, seed)


def brute_costs(leaves, kids, g, l):
    """leaves (R, A) bool: the smallest g gains + l losses over all 2^(inner nodes) assignments, int64 (R,)"""
    R, A = leaves.shape
    J = len(kids)
    inner = (np.arange(1 << J)[:, None] >> np.arange(J)[None, :] & 1).astype(np.int64)  # (assignments, joins)

    def state(v):  # (assignments or 1, R or 1)
        return leaves[:, v].astype(np.int64)[None, :] if v < A else inner[:, v - A][:, None]
    cost = np.zeros((1 << J, R), dtype=np.int64)
    for t, (a, b) in enumerate(kids):
        p = state(A + t)
        for c in (a, b):
            s = state(c)
            cost = cost + g * ((p == 0) & (s == 1)) + l * ((p == 1) & (s == 0))
    return cost.min(axis=0)


def test_against_brute_force_on_every_shape():
    """every tree shape of 2 .. 8 leaves, three cost pairs: cost(n, p) of every class is the minimum over all state assignments of the tip
    set the orders give, every replicate of class n has n tips present, and n_le / n_ge are what direct loops count"""
    rng = np.random.default_rng(12)
    for A in range(2, 9):
        n_perm = 9 if A < 8 else 4
        cls = list(range(1, A))
        for si, kids in enumerate(ps.all_shapes(A)):
            seed = 100 * A + si
            rk = ps.orders(A, seed, 1, n_perm)
            tips = rk[:, None, :] < np.array(cls)[None, :, None]  # (A, classes, perms)
            assert np.array_equal(tips.sum(axis=0), np.repeat(np.array(cls)[:, None], n_perm, axis=1))
            for g, l in COSTS:
                rows = ps.replicate_costs(kids, A, cls, n_perm, seed, g, l)
                want = brute_costs(tips.reshape(A, -1).T, kids, g, l).reshape(len(cls), n_perm)
                assert np.array_equal(rows, want), (A, si, g, l)
            if si % 7 == 0:  # the counts by direct loops, on items of every size
                P = rng.random((12, A)) < 0.5
                res = ps.pan_phylosig(P, kids, 2, 1, n_perm, seed, 1)
                assert res["cost"].tolist() == brute_costs(P, kids, 2, 1).tolist()
                for i in np.nonzero(res["tested"])[0]:
                    c = res["cls"].tolist().index(int(res["present"][i]))
                    assert ps.brute_counts(res["cost_rows"][c].tolist(), int(res["cost"][i])) == (int(res["n_le"][i]), int(res["n_ge"][i]))


def test_properties(ora):
    """exact properties on a random tree: the tips of a replicate, n_le + n_ge >= P, Cost <= MaxCost, sum = the row sums of the cost rows,
    and an item whose carriers are exactly one clade"""
    from pangene_amd import capi
    rng = np.random.default_rng(21)
    A, M, n_perm, seed = 23, 120, 60, 5
    rec = random_records(rng, A)
    kids = pr.tree(rec, A, "upgma")
    P = rng.random((M, A)) < rng.random(M)[:, None]
    members = [[x] for x in range(A)]
    for a, b in kids:
        members.append(members[a] + members[b])
    clades = [m for m in members[A:-1] if 2 <= len(m) <= A - 2]
    for k, m in enumerate(clades[:6]):  # six items that are one clade each
        P[k] = False
        P[k, m] = True
    for g, l in COSTS:
        want = ps.pan_phylosig(P, kids, g, l, n_perm, seed, 2)
        got = capi.pan_phylosig(ora, P, rec, "upgma", g, l, n_perm, seed, 2)
        assert ps.same(got, want)
        t = got["tested"] == 1
        assert t.sum() > 50 and len(want["cls"]) > 5
        rk = ps.orders(A, seed, 1, n_perm)
        for n in want["cls"]:
            assert np.array_equal((rk < n).sum(axis=0), np.full(n_perm, n))
        assert np.all(got["n_le"][t] + got["n_ge"][t] >= n_perm) and np.all(got["n_le"][~t] == 0) and np.all(got["n_ge"][~t] == 0)
        n = got["present"].astype(np.int64)
        assert np.all(got["cost"][t] <= np.minimum(n * g, (A - n) * l)[t])
        assert np.array_equal(got["sum"][want["cls"]], want["cost_rows"].sum(axis=1)) and got["sum"].sum() == want["cost_rows"].sum()
        for k in range(min(6, len(clades))):  # one gain above the clade is a reconstruction: Cost <= g, and no item that varies costs less than min(g, l)
            row = want["cost_rows"][want["cls"].tolist().index(len(clades[k]))]
            assert got["tested"][k] == 1 and min(g, l) <= got["cost"][k] <= g and row.min() >= min(g, l)
            assert got["n_le"][k] == int((row <= got["cost"][k]).sum()) and got["n_ge"][k] == int((row >= got["cost"][k]).sum())


def test_a_clade_costs_one_change(ora):
    """g = l: an item whose carriers are exactly one clade has Cost == g, the smallest cost a replicate can have, so its n_le counts only
    the replicates of that cost"""
    from pangene_amd import capi
    rng = np.random.default_rng(22)
    A, n_perm, seed = 19, 80, 9
    rec = random_records(rng, A)
    kids = pr.tree(rec, A, "upgma")
    members = [[x] for x in range(A)]
    for a, b in kids:
        members.append(members[a] + members[b])
    clades = [m for m in members[A:-1] if 2 <= len(m) <= A - 2]
    P = np.zeros((len(clades), A), dtype=bool)
    for k, m in enumerate(clades):
        P[k, m] = True
    for g in (1, 3):
        got = capi.pan_phylosig(ora, P, rec, "upgma", g, g, n_perm, seed, 2)
        want = ps.pan_phylosig(P, kids, g, g, n_perm, seed, 2)
        assert ps.same(got, want) and np.all(got["tested"] == 1) and np.all(got["cost"] == g)
        for k, m in enumerate(clades):
            row = want["cost_rows"][want["cls"].tolist().index(len(m))]
            assert row.min() >= g and got["n_le"][k] == int((row == g).sum()) and got["n_ge"][k] == n_perm


def test_small_shapes(ora):
    """no assemblies, one, two; no items; no tested item; no permutation"""
    from pangene_amd import capi
    r = capi.pan_phylosig(ora, np.zeros((3, 0), dtype=bool), None, "upgma")
    assert r["cost"].tolist() == [0, 0, 0] and r["tested"].tolist() == [0, 0, 0] and r["sum"].tolist() == [0]
    r = capi.pan_phylosig(ora, np.array([[1], [0]], dtype=bool), None, "upgma", min_count=1)
    assert r["tested"].tolist() == [0, 0] and r["sum"].tolist() == [0, 0]
    P = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=bool)
    r = capi.pan_phylosig(ora, P, None, "nj", 2, 5, 10, 3, 1)
    assert ps.same(r, ps.pan_phylosig(P, [(0, 1)], 2, 5, 10, 3, 1)) and r["tested"].tolist() == [0, 1, 1, 0] and r["n_le"].tolist() == [0, 10, 10, 0] and r["sum"].tolist() == [0, 20, 0]
    r = capi.pan_phylosig(ora, np.zeros((0, 5), dtype=bool), random_records(np.random.default_rng(1), 5), "upgma")
    assert r["cost"].shape == (0,) and r["sum"].tolist() == [0] * 6
    P = np.random.default_rng(2).random((9, 6)) < 0.5
    rec = random_records(np.random.default_rng(2), 6)
    r = capi.pan_phylosig(ora, P, rec, "upgma", min_count=4)
    assert not r["tested"].any() and not r["sum"].any()
    r = capi.pan_phylosig(ora, P, rec, "upgma", n_perm=0, min_count=1)
    assert ps.same(r, ps.pan_phylosig(P, pr.tree(rec, 6, "upgma"), 1, 1, 0, 11, 1)) and not r["n_le"].any() and not r["sum"].any()


def test_empty_inputs_print_the_header_only(built, tmp_path):
    empty = tmp_path / "empty.gfa"
    empty.write_text("")
    rc, got, err = run_cli(["phylosig", str(empty)])
    assert rc == 0 and got == ps.HEADER, err
    one = tmp_path / "one.gfa"  # one assembly: nothing can be tested
    one.write_text("S\tg1\t*\nS\tg2\t*\nL\tg1\t+\tg2\t+\t0M\nW\ts1\t0\tc1\t*\t*\t>g1>g2\n")
    rc, got, _ = run_cli(["phylosig", "-c", "1", str(one)])
    assert rc == 0 and got == ps.HEADER == ps.table(str(one), min_count=1)
    rc, got, _ = run_cli(["phylosig", "-c", "100000", gfa_of("C4")])  # no tested item
    assert rc == 0 and got == ps.HEADER


def test_refusals_and_usage(built, ora, tmp_path):
    from pangene_amd import capi
    gfa = gfa_of("C4")
    for bad, msg in ((["-g", "0"], b"-g must be in [1, 255]"), (["-g", "256"], b"-g must be in [1, 255]"), (["-l", "0"], b"-l must be in [1, 255]"),
                     (["-l", "x"], b"-l must be in [1, 255]"), (["-a", "ml"], b"-a must be upgma or nj"), (["-m", "shared"], b"-m must be jaccard or diff"),
                     (["-t", "exon"], b"-t must be gene or adj"), (["-c", "0"], b"-c must be at least 1"), (["-n", "-1"], b"-n must be in [0, 2147483646]"),
                     (["-n", "2147483647"], b"-n must be in [0, 2147483646]"), (["-s", "-1"], b"-s must be in [0, 4294967295]"), (["-s", "4294967296"], b"-s must be in"),
                     (["-p", "-0.1"], b"-p must be a number >= 0"), (["-p", "x"], b"-p must be a number >= 0")):
        rc, out, err = run_cli(["phylosig"] + bad + [gfa])
        assert rc == 1 and out == b"" and msg in err, (bad, err)
    rc, out, err = run_cli(["phylosig", "-r", "late", gfa])  # there is no tie rule here
    assert rc == 1 and out == b""
    files = pafs_of("C4")
    for bad in ("--phylosig=x", "--phylosig=-1", "--phylosig-gain=0", "--phylosig-loss=256", "--phylosig-method=ml", "--phylosig-metric=shared", "--phylosig-type=exon",
                "--phylosig-min=0", "--phylosig-seed=-1", "--phylosig-max-p=-1"):
        rc, out, err = run_cli(["--phylosig", bad] + files)
        assert rc == 1 and out == b"" and bad.split("=")[0].encode() in err, bad
        with pytest.raises(ValueError):
            capi.run(ora, files, ["--phylosig", bad])
    rc, out, err = run_cli(["--phylosig-type=adj"] + files)
    assert rc == 1 and out == b"" and b"need --phylosig" in err and b"--phylosig-type" in err and b"--phylosig-max-p" in err
    with pytest.raises(ValueError):
        capi.run(ora, files, ["--phylosig-type=adj"])
    rc, out, err = run_cli(["--coevo", "--phylosig"] + files)
    assert rc == 1 and out == b"" and b"--phylosig cannot be combined with" in err
    assert all(b"--" + w.encode() in err for w in EARLIER) and b"or --coevo" in err
    with pytest.raises(ValueError) as e:
        capi.run(ora, files, ["--coevo", "--phylosig"])
    assert all("--" + w in str(e.value) for w in EARLIER)
    rc, out, err = run_cli(["--matrix", "--phylosig"] + files)
    assert rc == 1 and out == b"" and b"cannot be combined" in err
    rc, out, err = run_cli(["--gpus", "2", "--phylosig"] + files)
    assert rc == 1 and out == b"" and b"--phylosig needs every genome in one process" in err
    rc, out, err = run_cli(["phylosig", str(tmp_path / "missing.gfa")])
    assert rc == 1 and out == b""
    rc, out, err = run_cli(["phylosig"])
    assert rc == 0 and out.startswith(b"Usage: pangene phylosig [options] <in.gfa>\n")
    assert all(w in out for w in (b"--phylosig[=INT]", b"-t STR", b"(type)", b"-m STR", b"(metric)", b"-a STR", b"(method)", b"-g INT", b"(gain)", b"-l INT", b"(loss)", b"-n INT",
                                  b"-s INT", b"(seed)", b"-c INT", b"(min)", b"-p FLOAT", b"(max-p)", b"[1000]", b"[11]", b"[2]", b"p_signal", b"p_scatter"))
    # pg_pan_phylosig itself: NULLs, option values out of range and bad records are PGA_ERR_ARG (-3), sizes out of range PGA_ERR_RANGE (-2)
    P = np.ascontiguousarray(np.random.default_rng(2).random((6, 4)) < 0.5, dtype=np.uint8)
    rec = np.ascontiguousarray(random_records(np.random.default_rng(2), 4))
    item, total = np.zeros((6, 5), dtype=np.int32), np.zeros(5, dtype=np.int64)
    pp, rp = P.ctypes.data_as(C.POINTER(C.c_uint8)), rec.ctypes.data_as(C.POINTER(C.c_int64))
    ip, tp = item.ctypes.data_as(C.POINTER(C.c_int32)), total.ctypes.data_as(C.POINTER(C.c_int64))

    def call(p=pp, r=rp, method=1, o=None, i=ip, t=tp, M=6, A=4, **kw):
        opt = capi.phylosig_opt(ora, n_perm=5)
        for k, v in kw.items():
            setattr(opt, k, v)
        return ora.pg_pan_phylosig(p, M, A, r, method, None if o == "null" else C.byref(opt), i, t)

    assert call() == 0
    assert call(gain=0) == -3 and call(gain=256) == -3 and call(loss=0) == -3 and call(loss=256) == -3 and call(n_perm=-1) == -3 and call(min_count=0) == -3
    assert call(o="null") == -3 and call(p=None) == -3 and call(r=None) == -3 and call(i=None) == -3 and call(t=None) == -3 and call(method=2) == -3
    assert call(M=-1) == -3 and call(A=-1) == -3
    r2 = rec.copy()
    r2[0, 0], r2[0, 1] = 0, 4
    assert call(r=r2.ctypes.data_as(C.POINTER(C.c_int64))) == -3
    assert call(A=65536) == -2 and call(M=16777216) == -2
    with pytest.raises(ValueError):
        capi.phylosig_opt(ora, gain=0)
    with pytest.raises(ValueError):
        capi.phylosig_opt(ora, min_count=0)
    with pytest.raises(ValueError):
        capi.pan_phylosig(ora, P, rec[:2], "upgma")
    assert C.sizeof(capi.pg_phylosig_opt_t) == 40
