"""pg_post_process without its host step (pga_post_front: k_post_count + k_post_rep in front of k_post_apply).

The kernels against the plain restatement of the host's step (tests/support/front_ref.py, itself checked against the exact sort order by
tests/test_front.py), and whole runs under both values of PANGENE_FRONT: the same bytes, the route that was announced, the wait that
went away, and -- on a set whose isoforms tie at a gene's largest key -- one repeated front, after which the data set keeps the host
route without trying again."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_files

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import front_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu

_RUN = os.path.join(ROOT, "tests", "support", "front_run.py")


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def _check(sums, gid, Q, G, ratio, no_pj, drop, expect_tie):
    import front_direct
    rng = np.random.default_rng(len(gid))
    max_ori = rng.integers(-5, 1 << 20, size=len(gid)).astype(np.int32)
    got = front_direct.post_rep(sums, max_ori, gid, Q, G * float(ratio), not no_pj, drop)
    ref = fr.post_rep_ref(sums, gid, Q, G, ratio, no_pj, drop)
    assert ref["tie"] == expect_tie
    assert got["max_ori"].tolist() == max_ori.tolist()
    assert got["n"].tolist() == ref["n"] and got["avg"].tolist() == ref["avg"]
    assert got["pj"].tolist() == ref["pj"]
    assert (got["tie"] != 0) == ref["tie"]  # a tie at a gene's largest key is REPORTED, whichever protein was taken
    ok = [g for g in range(Q) if g not in ref["tie_genes"]]
    assert [int(got["rep_pid"][g]) for g in ok] == [ref["rep_pid"][g] for g in ok]
    rep = np.zeros(len(gid), dtype=np.uint8)
    for g in range(Q):
        members = np.flatnonzero(gid == g)
        assert int(got["rep"][members].sum()) == (1 if len(members) else 0)  # one representative a gene, tie or not
        if g in ok and ref["rep_pid"][g] >= 0:
            rep[ref["rep_pid"][g]] = 1
    tied = np.isin(gid, ref["tie_genes"])
    assert got["rep"][~tied].tolist() == rep[~tied].tolist()
    return got, ref


@pytest.mark.parametrize("seed,no_pj,drop", [(0, False, False), (1, False, True), (2, True, True), (3, False, False)])
def test_representatives_of_genes_with_1_2_and_5_proteins(built, seed, no_pj, drop):
    """300 genes of 1, 2 and 5 proteins scattered over ~650 protein ids (three workgroups), a tenth of the proteins without a rank-0 hit
    (count == 0: no division), a twentieth with a negative sum (the key's unsigned arithmetic); ties BELOW a gene's
    largest key raise nothing; genes without any protein keep rep_pid = -1"""
    rng = np.random.default_rng(seed)
    sizes = rng.choice([1, 1, 2, 5, 0], size=300).tolist()
    five = [g for g, s in enumerate(sizes) if s == 5]
    sums, gid = fr.instance(rng, sizes, tie_below=five[:10])
    got, ref = _check(sums, gid, len(sizes), 100, 0.05, no_pj, drop, False)
    assert {sizes[g] for g in range(len(sizes)) if got["rep_pid"][g] >= 0} == {1, 2, 5}
    assert all(got["rep_pid"][g] == -1 for g, s in enumerate(sizes) if s == 0)
    assert 0 in ref["n"] and (sums[0] < 0).any()
    assert no_pj or 0 < sum(ref["pj"]) < len(gid)


def test_a_tie_at_the_maximum_raises_the_flag_and_one_below_does_not(built):
    rng = np.random.default_rng(5)
    sizes = [1, 2, 5, 2, 5, 1, 3] * 10
    sums, gid = fr.instance(rng, sizes, tie_below=[4, 11, 6])
    _check(sums, gid, len(sizes), 100, 0.05, False, False, False)
    sums, gid = fr.instance(rng, sizes, tie_at_max=[3], tie_below=[4])
    _check(sums, gid, len(sizes), 100, 0.05, False, False, True)
    sums, gid = fr.instance(rng, sizes, tie_at_max=[2, 9, 69])
    _check(sums, gid, len(sizes), 100, 0.05, False, False, True)


def test_all_zero_keys(built):
    """proteins nothing was counted for: alone in their gene they are its representative (key 0 is the largest), two of them tie"""
    rng = np.random.default_rng(6)
    sizes = [1, 2, 5, 1, 1, 2]
    sums, gid = fr.instance(rng, sizes, zero_key_genes=[0, 3])
    got, _ = _check(sums, gid, len(sizes), 100, 0.05, False, False, False)
    assert got["rep_pid"][0] >= 0 and got["n"][got["rep_pid"][0]] == 0 and got["avg"][got["rep_pid"][0]] == 0
    sums, gid = fr.instance(rng, sizes, zero_key_genes=[0, 1])
    _check(sums, gid, len(sizes), 100, 0.05, False, False, True)
    sums = np.zeros((6, 4), dtype=np.int64)
    _check(sums, np.arange(4, dtype=np.int32), 4, 100, 0.05, False, True, False)


@pytest.mark.parametrize("drop", [False, True])
def test_the_joint_pseudo_predicate_at_its_edges(built, drop):
    """c1 exactly at n_genome * min_vertex_ratio (>= and <= both hold), one below and one above; c0 == 0 with and without a sum (NaN, inf: false
    unless the quotient is +inf); s0 == 0 with c0 > 0 (a division by zero that gives +inf: true); the ratio just below, at and above 0.99"""
    G, ratio = 20, 0.25  # the threshold is 5.0
    rows = [  # c0, c1, s0, s1
        (3, 5, 300, 500), (3, 4, 300, 400), (3, 6, 300, 600), (0, 6, 0, 600), (0, 6, 7, 600), (2, 6, 0, 600), (2, 6, 0, 0), (2, 6, 0, -600),
        (1, 6, 100, 593), (1, 6, 100, 594), (1, 6, 100, 595), (100, 6, 10000, 594), (4, 0, 400, 0), (0, 0, 0, 0), (7, 6, -700, -600), (7, 6, 700, -600), (1, 0, 5, 0)]
    sums = np.zeros((6, len(rows)), dtype=np.int64)
    for p, (c0, c1, s0, s1) in enumerate(rows):
        sums[0, p], sums[2, p], sums[3, p], sums[4, p], sums[5, p] = 1000 + p, c0, c1, s0, s1
    sums[0, -1] = -1  # one hit with a negative score: 0xffffffff in the key's upper half, an average no int32 holds
    _, ref = _check(sums, np.arange(len(rows), dtype=np.int32), len(rows), G, ratio, False, drop, False)
    assert ref["n"][-1] == 1 and ref["avg"][-1] == -(1 << 31)
    assert ref["pj"][:3] == [1, int(drop), 1] and ref["pj"][3:8] == [0, 0, 1, 0, 0] and ref["pj"][8:11] == [0, 1, 1]


# ---------------------------------------------------------------------------------------------------------------------------------
# whole runs
# ---------------------------------------------------------------------------------------------------------------------------------
def _run(tmp_path, tag, route, variant, files, exact, extra=None):
    prefix = str(tmp_path / tag)
    env = dict(os.environ, PANGENE_TIMING="1", PANGENE_FRONT=route, FRONT_EXACT=str(exact), **(extra or {}))
    r = subprocess.run([sys.executable, _RUN, prefix, variant] + files, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    info = json.loads(r.stdout.decode().strip().splitlines()[-1])
    first, _, second = r.stderr.decode().partition("[front_run] pass 2")
    for k, text in (("p1", first), ("p2", second)):
        lines = [l for l in text.splitlines() if l.startswith("[front] ")]
        info[k] = {"device": sum(l.startswith("[front] pg_post_process: representatives on the device") for l in lines),
                   "host": sum(l.startswith("[front] pg_post_process: representatives on the host") for l in lines),
                   "tie": sum("share its largest key" in l for l in lines), "sticky": sum("a gene of this data set has two proteins" in l for l in lines)}
    out = {t: [open(prefix + t + "." + x, "rb").read() for x in ("gfa", "arc", "seg")] for t in ("", ".2")}
    return info, out


def _tied(tmp_path):
    """synth.bact(8, 300) with genome 1 replaced by a copy of genome 0, and three proteins renamed to isoform a (in genome 0) and isoform b (in
    its copy) of one gene each: the two isoforms have the same hits, so the same sum and count -- two proteins at their gene's largest key"""
    from pangene_amd import synth
    texts = list(synth.bact(8, 300))
    base = texts[0][1]
    texts[1] = (texts[1][0], base.replace("g0#0#", "g1#0#"))
    names = sorted({line.split("\t", 1)[0] for line in base.splitlines()})
    assert len(names) > 100
    for k, iso in ((0, "a"), (1, "b")):
        t = texts[k][1]
        for p in (names[5], names[50], names[100]):
            assert p + "\t" in t
            t = t.replace(p + "\t", "T%s:%s\t" % (p, iso))
        texts[k] = (texts[k][0], t)
    return synth.write_files(iter(texts), str(tmp_path / "tied"))


_GOLDEN = ("bact20", "human8f")


def _sets(tmp_path):
    from pangene_amd import synth
    return {"bact": lambda: synth.write_files(synth.bact(8, 300), str(tmp_path / "bact")), "tied": lambda: _tied(tmp_path),
            "human_iso": lambda: synth.write_files(synth.human(6, 400, iso=3), str(tmp_path / "human")),
            "many_doms": lambda: synth.write_files(synth.many_doms(), str(tmp_path / "doms")),
            "dense": lambda: synth.write_files(synth.dense(), str(tmp_path / "dense")),
            "bact20": lambda: golden_files("bact20"), "human8f": lambda: golden_files("human8f")}


@pytest.mark.parametrize("name,variant,exact", [("bact", "", 1), ("bact", "-G", 1), ("bact", "-p0 -a1", 1), ("human_iso", "", 1), ("human_iso", "-p0 -a1", 1), ("many_doms", "-G", 1), ("many_doms", "", 1),
                                                ("dense", "", 1), ("tied", "", 1), ("tied", "-p0 -a1", 1), ("bact20", "", 2), ("bact20", "-G", 2), ("human8f", "-p0 -a1", 2)])
def test_both_routes_give_the_same_graph(built, expected, tmp_path, name, variant, exact):
    """GFA bytes (with -G the selection lines too), q->seg and q->arc under PANGENE_FRONT=device and =host, in a first pass and in a second one over the
    resident shard; the golden sets against the recorded md5 of the reference as well.  Every pg_post_process of the host run says `host`; those of
    the device run say `device` until a tie is found, and the second pass has one wait fewer for each of them."""
    files = _sets(tmp_path)[name]()
    dev, out_d = _run(tmp_path, "d", "device", variant, files, exact)
    host, out_h = _run(tmp_path, "h", "host", variant, files, exact)
    print(name, repr(variant), "device", dev, "host", host)
    assert out_d[""] == out_h[""] and out_d[".2"] == out_h[".2"] and out_d[""] == out_d[".2"]
    assert dev["n_seg"] > 0 and dev["n_arc"] > 0
    if name in _GOLDEN:
        assert hashlib.md5(out_d[""][0]).hexdigest() == expected[name][variant]["md5"]
    assert host["p1"]["device"] == 0 and host["p2"]["device"] == 0 and host["p1"]["host"] >= 1 and host["p2"]["host"] >= 1
    assert dev["p1"]["device"] >= 1
    if dev["p1"]["tie"] == 0:  # the device route all the way
        assert dev["p1"]["host"] == 0 and dev["p2"] == {"device": host["p2"]["host"], "host": 0, "tie": 0, "sticky": 0}
        assert host["waits_post"] - dev["waits_post"] == 1
        assert exact != 1 or dev["waits_post"] == 0  # (exact mode 2 hands the reference's order over inside pg_post_process, which waits on either route)
        assert host["waits_post"] + host["waits_gen"] - dev["waits_post"] - dev["waits_gen"] == dev["p2"]["device"]
    else:
        assert dev["p2"]["device"] == 0
        assert (dev["waits_post"], dev["waits_gen"]) == (host["waits_post"], host["waits_gen"])


def test_tied_isoforms_repeat_the_front_once_and_keep_the_host_route(built, tmp_path):
    """Two isoforms of one gene with equal sums and counts (_tied; synth.human(6, 400, iso=3) has isoforms but, as measured, none that tie at a gene's
    largest key: it stays on the device route in the test above).  The first pg_post_process takes the device route, the vertex step's wait
    brings the tie flag, the pass is repeated from stage A with the representatives picked on the host; the second pass over the data set starts on
    the host route (no second speculation, no repeat).  bact has one protein a gene: no flag can go up."""
    files = _sets(tmp_path)["tied"]()
    dev, _ = _run(tmp_path, "t", "device", "", files, 1)
    print(dev)
    assert dev["p1"]["device"] == 1 and dev["p1"]["tie"] == 1 and dev["p1"]["host"] >= 1 and dev["p1"]["sticky"] == dev["p1"]["host"]
    assert dev["p2"]["device"] == 0 and dev["p2"]["tie"] == 0 and dev["p2"]["host"] >= 1 and dev["p2"]["sticky"] == dev["p2"]["host"]
    bact, _ = _run(tmp_path, "b", "device", "", _sets(tmp_path)["bact"](), 1)
    assert bact["p1"]["tie"] == 0 and bact["p2"]["tie"] == 0 and bact["p1"]["host"] == 0 and bact["p2"]["host"] == 0


def test_device_route_after_a_pass_on_the_host_route(built, tmp_path):
    """A context whose last pg_post_process took the host route (here: a first pass at pg_verbose = 3, where the log counts the pseudogene hits) no longer prepares
    the genes' keys in pga_post_partials; the device route of the next pass computes them itself.  Same bytes as two passes on the host route."""
    files = _sets(tmp_path)["bact"]()
    dev, out_d = _run(tmp_path, "v", "device", "", files, 1, {"FRONT_RUN_VERBOSE_FIRST": "1"})
    host, out_h = _run(tmp_path, "w", "host", "", files, 1)
    print(dev)
    assert dev["p1"]["device"] == 0 and dev["p1"]["host"] >= 1 and dev["p2"]["device"] >= 1 and dev["p2"]["host"] == 0
    assert out_d[""] == out_h[""] and out_d[".2"] == out_h[".2"] and out_d[""] == out_d[".2"]
