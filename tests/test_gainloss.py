"""Gene gain and loss on the tree (`pangene gainloss`, `pangene --gainloss`, pg_pan_gainloss) through the checker build: the host driver
linked against the oracle backend, whose table has no pan_gainloss entry, so the two passes come from the plain loops of
pan_gainloss.hpp over the records themselves.  Everything is compared with the numpy restatement of tests/support/gainloss_ref.py, and
that with a brute force over all inner-node assignments."""
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
import gainloss_ref as gr  # noqa: E402
import pairs_ref as pr  # noqa: E402

NAMES = ["C4", "bact20", "human8"]
COSTS = ((1, 1), (2, 1), (1, 2), (5, 3), (255, 255))


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
    return oracle_host.load()


def random_records(rng, A):
    """upgma-shaped records of a random rooted tree: any two live slots are joined"""
    live, rec = list(range(A)), []
    while len(live) > 1:
        i, j = (int(v) for v in rng.choice(live, size=2, replace=False))
        rec.append((i, j, 0, 0, 0, len(live)))
        live.remove(j)
    return np.array(rec, dtype=np.int64).reshape(-1, 6)


def all_patterns(A):
    """every leaf pattern of A leaves as the rows of a presence matrix (2^A, A)"""
    return (np.arange(1 << A)[:, None] >> np.arange(A)[None, :] & 1).astype(bool)


@pytest.mark.parametrize("name", NAMES)
def test_file_route(built, name):
    """the whole text of both tables against the restatement for the five option sets"""
    for kw in gr.OPTION_SETS:
        sub, _ = gr.option_args(**kw)
        rc, out, err = run_cli(["gainloss"] + sub + [gfa_of(name)])
        assert rc == 0, err
        want = gr.table(gfa_of(name), **kw)
        assert out == want, (kw, out[:300], want[:300])
        assert out.count(b"\n") > 1 or kw.get("min_changes")  # (no item of C4 changes twice)
    rc, out, err = run_cli(["gainloss", gfa_of(name)])  # and the defaults without any option
    assert rc == 0 and out == gr.table(gfa_of(name))


@pytest.mark.parametrize("name", NAMES)
def test_in_memory_route(built, tmp_path, name):
    """`pangene --gainloss ... *.paf` prints what `pangene gainloss` prints for the GFA of the same run, and what the restatement does"""
    files = pafs_of(name)
    rc, gfa, err = run_cli(files)
    assert rc == 0, err
    path = str(tmp_path / "g.gfa")
    with open(path, "wb") as f:
        f.write(gfa)
    for kw in gr.OPTION_SETS:
        sub, long = gr.option_args(**kw)
        rc1, a, err = run_cli(long + files)
        rc2, b, _ = run_cli(["gainloss"] + sub + [path])
        assert rc1 == 0 and rc2 == 0, err
        assert a == b == gr.table(path, **kw), kw
    rc, a, _ = run_cli(["--gainloss"] + files)
    assert rc == 0 and a == gr.table(path)
    if name == "C4":  # and capi.run, the same route in-process
        import oracle_host
        from pangene_amd import capi
        lib = oracle_host.load()
        C.c_int.in_dll(lib, "pg_verbose").value = 0
        kw = gr.OPTION_SETS[2]
        assert capi.run(lib, files, gr.option_args(**kw)[1]) == gr.table(path, **kw)
        with pytest.raises(ValueError):
            capi.run(lib, files, ["--gainloss-gain=2"])
        with pytest.raises(ValueError):
            capi.run(lib, files, ["--gainloss", "--gainloss-gain=0"])
        with pytest.raises(ValueError):
            capi.run(lib, files, ["--gainloss", "--mantel"])


def test_against_brute_force(ora):
    """capi.pan_gainloss on random rooted trees of 1 .. 8 leaves with every leaf pattern: the restatement's arrays, and the cost the
    smallest over all inner-node assignments"""
    from pangene_amd import capi
    rng = np.random.default_rng(3)
    for A in range(1, 9):
        P = all_patterns(A)
        for it in range(2 if A < 8 else 1):
            rec = random_records(rng, A)
            kids = pr.tree(rec, A, "upgma")
            for (g, l), mode in zip(COSTS, ("late", "early", "late", "early", "late")):
                want = gr.reconstruct(P, kids, g, l, mode)
                got = capi.pan_gainloss(ora, P, rec if A >= 3 else None, "upgma", g, l, mode)
                assert gr.same(got, want), (A, g, l, mode)
                if it == 0 and (g, l) in ((1, 1), (5, 3)):
                    assert [gr.brute(P[i], kids, g, l) for i in range(len(P))] == want["cost"].tolist(), (A, g, l)


def test_identities(ora):
    """cost = g gains + l losses; the items' gains and losses add up to the nodes'; a leaf's state is its bit; the root's branch is empty"""
    from pangene_amd import capi
    rng = np.random.default_rng(4)
    A, M = 23, 300
    P = rng.random((M, A)) < 0.4
    for method in ("upgma", "nj"):
        rec, _ = capi.pan_tree(ora, P, "jaccard", method)
        kids = pr.tree(rec, A, method)
        for g, l in COSTS:
            for mode in ("late", "early"):
                r = capi.pan_gainloss(ora, P, rec, method, g, l, mode)
                want = gr.reconstruct(P, kids, g, l, mode)
                assert gr.same(r, want)
                assert np.array_equal(r["cost"], g * r["gains"] + l * r["losses"])
                assert r["gains"].sum() == r["node_gains"].sum() and r["losses"].sum() == r["node_losses"].sum()
                assert r["node_gains"][-1] == 0 and r["node_losses"][-1] == 0
                assert np.array_equal(r["node_present"][:A], P.sum(axis=0)) and np.array_equal(want["state"][:A], P.T)
                assert np.array_equal(r["present"], P.sum(axis=1))


def test_cost_is_the_same_under_the_three_readings_of_the_trifurcation(ora):
    """g = l = 1: the cost belongs to the unrooted tree, so ((x, y), z), ((x, z), y) and ((y, z), x) agree; the library reads the first"""
    from pangene_amd import capi
    rng = np.random.default_rng(6)
    A = 17
    P = rng.random((200, A)) < 0.5
    rec, _ = capi.pan_tree(ora, P, "jaccard", "nj")
    costs = [gr.reconstruct(P, pr.tree(rec, A, "nj", t), 1, 1)["cost"] for t in range(3)]
    assert np.array_equal(costs[0], costs[1]) and np.array_equal(costs[0], costs[2])
    assert np.array_equal(capi.pan_gainloss(ora, P, rec, "nj")["cost"], costs[0])


def test_constant_items_never_change(ora):
    from pangene_amd import capi
    A = 12
    P = np.zeros((2, A), dtype=bool)
    P[0] = True
    rec = random_records(np.random.default_rng(8), A)
    for g, l in COSTS:
        for mode in ("late", "early"):
            r = capi.pan_gainloss(ora, P, rec, "upgma", g, l, mode)
            assert r["root"].tolist() == [1, 0] and r["cost"].tolist() == [0, 0] and r["gains"].tolist() == [0, 0] and r["losses"].tolist() == [0, 0]
            assert r["node_present"].tolist() == [1] * (2 * A - 1) and not r["node_gains"].any() and not r["node_losses"].any()


def test_small_shapes(ora):
    """one assembly (the leaf is the root), two (one join, no records), and no items"""
    from pangene_amd import capi
    P = np.array([[1], [0]], dtype=bool)
    r = capi.pan_gainloss(ora, P, None, "upgma")
    assert r["root"].tolist() == [1, 0] and r["cost"].tolist() == [0, 0] and r["node_present"].tolist() == [1] and gr.same(r, gr.reconstruct(P, [], 1, 1))
    P = gr_patterns = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], dtype=bool)
    for mode in ("late", "early"):
        for g, l in COSTS:
            r = capi.pan_gainloss(ora, P, None, "nj", g, l, mode)
            assert gr.same(r, gr.reconstruct(gr_patterns, [(0, 1)], g, l, mode))
    r = capi.pan_gainloss(ora, np.zeros((0, 5), dtype=bool), random_records(np.random.default_rng(1), 5), "upgma")
    assert r["cost"].shape == (0,) and r["node_present"].tolist() == [0] * 9
    r = capi.pan_gainloss(ora, np.zeros((3, 0), dtype=bool), None, "upgma")
    assert r["cost"].tolist() == [0, 0, 0] and r["node_present"].shape == (0,)


def test_empty_inputs_print_the_header_only(built, tmp_path):
    empty = tmp_path / "empty.gfa"
    empty.write_text("")
    for out, head in (("gene", gr.GENE_HEADER), ("node", gr.NODE_HEADER)):
        rc, got, err = run_cli(["gainloss", "-o", out, str(empty)])
        assert rc == 0 and got == head, err
    one = tmp_path / "one.gfa"  # one assembly: the leaf is the root
    one.write_text("S\tg1\t*\nS\tg2\t*\nL\tg1\t+\tg2\t+\t0M\nW\ts1\t0\tc1\t*\t*\t>g1>g2\n")
    rc, got, _ = run_cli(["gainloss", str(one)])
    assert rc == 0 and got == gr.GENE_HEADER + b"g1\t1\t0\t0\t0\t0\t1\ng2\t1\t0\t0\t0\t0\t1\n"
    rc, got, _ = run_cli(["gainloss", "-o", "node", str(one)])
    assert rc == 0 and got == gr.NODE_HEADER + b"s1#0\t.\t.\t1\t2\tNA\tNA\n"
    assert got == gr.table(str(one), out="node")


def test_refusals_and_usage(built, ora, tmp_path):
    from pangene_amd import capi
    gfa = gfa_of("C4")
    for bad in (["-g", "0"], ["-g", "256"], ["-l", "0"], ["-l", "x"], ["-r", "middle"], ["-o", "tree"], ["-a", "ml"], ["-m", "shared"], ["-t", "exon"], ["-c", "-1"]):
        rc, out, err = run_cli(["gainloss"] + bad + [gfa])
        assert rc == 1 and out == b"" and bad[0].encode() in err, bad
    files = pafs_of("C4")
    for bad in ("--gainloss=tree", "--gainloss-gain=0", "--gainloss-loss=256", "--gainloss-resolve=x", "--gainloss-method=ml", "--gainloss-metric=shared",
                "--gainloss-type=exon", "--gainloss-min=-1"):
        rc, out, err = run_cli(["--gainloss", bad] + files)
        assert rc == 1 and out == b"" and bad.split("=")[0].encode() in err, bad
    rc, out, err = run_cli(["--gainloss-gain=2"] + files)
    assert rc == 1 and out == b"" and b"need --gainloss" in err
    rc, out, err = run_cli(["--gainloss", "--mantel"] + files)
    assert rc == 1 and out == b"" and b"cannot be combined" in err
    rc, out, err = run_cli(["--gpus", "2", "--gainloss"] + files)
    assert rc == 1 and out == b"" and b"--gainloss" in err
    rc, out, err = run_cli(["gainloss", str(tmp_path / "missing.gfa")])
    assert rc == 1 and out == b""
    rc, out, err = run_cli(["gainloss"])
    assert rc == 0 and out.startswith(b"Usage: pangene gainloss [options] <in.gfa>\n")
    assert all(w in out for w in (b"-g INT", b"-l INT", b"-r STR", b"-o STR", b"-c INT", b"((x, y), z)", b"depend on that reading", b"[upgma]"))
    rc, out, err = run_cli([])
    assert b"--gainloss[=STR]" in err and b"pangene gainloss [-t gene|adj]" in err
    # pg_pan_gainloss itself: NULLs, option values out of range and bad records are PGA_ERR_ARG (-3), sizes out of range PGA_ERR_RANGE (-2)
    P = np.ascontiguousarray(np.random.default_rng(2).random((6, 4)) < 0.5, dtype=np.uint8)
    rec = np.ascontiguousarray(random_records(np.random.default_rng(2), 4))
    gene, node = np.zeros((6, 5), dtype=np.int32), np.zeros((7, 3), dtype=np.int64)
    pp, rp = P.ctypes.data_as(C.POINTER(C.c_uint8)), rec.ctypes.data_as(C.POINTER(C.c_int64))
    gp, np_ = gene.ctypes.data_as(C.POINTER(C.c_int32)), node.ctypes.data_as(C.POINTER(C.c_int64))

    def call(p=pp, r=rp, method=1, o=None, g=gp, n=np_, M=6, A=4, **kw):
        opt = capi.gainloss_opt(ora)
        for k, v in kw.items():
            setattr(opt, k, v)
        return ora.pg_pan_gainloss(p, M, A, r, method, None if o == "null" else C.byref(opt), g, n)

    assert call() == 0
    assert call(gain=0) == -3 and call(gain=256) == -3 and call(loss=0) == -3 and call(loss=256) == -3 and call(mode=2) == -3 and call(mode=-1) == -3
    assert call(o="null") == -3 and call(p=None) == -3 and call(r=None) == -3 and call(g=None) == -3 and call(n=None) == -3 and call(method=2) == -3
    assert call(M=-1) == -3 and call(A=-1) == -3
    for bad in ([(0, 0)], [(0, 4)], [(0, 1), (1, 2)], [(-1, 2)]):  # a slot twice in a join, out of range, retired, negative
        r2 = rec.copy()
        for t, (i, j) in enumerate(bad):
            r2[t, 0], r2[t, 1] = i, j
        assert call(r=r2.ctypes.data_as(C.POINTER(C.c_int64))) == -3, bad
    assert call(A=65536) == -2 and call(M=16777216) == -2
    with pytest.raises(ValueError):
        capi.gainloss_opt(ora, gain=0)
    with pytest.raises(ValueError):
        capi.pan_gainloss(ora, P, rec[:2], "upgma")
