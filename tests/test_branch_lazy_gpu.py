"""The lazy form of a queued branch round (k_branch.hpp: BrLazy): the main pair list carries part 1 and row 0 of part 2, the decision lists the
pairs the later rows can still consult in a residual list, and k_br_finish replays those rows.

1. The device chain (pga_selftest_branch: counts -> list -> k_n_local -> decision -> residual list -> k_n_local -> k_br_finish) against a plain
   restatement of branch.c:60-90 over a given, deliberately non-transitive "is local" relation (tests/support/branch_ref.py), both forms.
2. A data set on which pg_flt_high_occ's max_dist_loci test deletes segments (tests/golden/distloci), against the reference's recorded md5.
3. Whole runs of two synthetic sets: the bytes of PANGENE_BR_LAZY=0 against the default's, also with the lists rebuilt inside the loop."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden_files
from pangene_amd import capi

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import branch_ref as br  # noqa: E402

pytestmark = pytest.mark.gpu

_RUN = os.path.join(ROOT, "tests", "support", "loop_tail_run.py")
BD, BDIST, BCUT = 0.02, 0.3, 0.6
SIZES = (2, 3, 7, 63, 64, 65)


def _pairs(*ps):
    return {frozenset(p) for p in ps}


def _clique(members):
    """every member local with the first one; up to seven members, with every other one too (the record table has a genome for every local pair of
    the largest vertex: the large vertices keep to stars, so that k_n_local runs with the sixteen lanes a pair of the flagship's 100 genomes)"""
    members = list(members)
    if len(members) <= 7:
        return {frozenset((a, b)) for a in members for b in members if a < b}
    return {frozenset((members[0], b)) for b in members[1:]}


def _vertices():
    rng = np.random.default_rng(11)
    V = [([], set()), ([50], set())]  # no arc, one arc: n_dist_loci = 0
    flat = lambda n: [100] * n  # noqa: E731
    for n in SIZES:
        V.append((flat(n), _pairs(*[(0, j) for j in range(1, n)])))  # everything local to arc 0
        V.append((flat(n), set()))  # pairwise distant: n groups
        if n >= 3:
            V.append((flat(n), _pairs(*[(0, j) for j in range(2, n)])))  # arc 1 the only one without a group after row 0: the empty stretch
            V.append((flat(n), _pairs(*[(j, j + 1) for j in range(n - 1)])))  # a chain: every arc joins group 1, all but arc 1 through a later row
            V.append((flat(n), _pairs(*[(0, j) for j in range(1, n - 1)]) | _pairs((1, n - 1))))  # the last arc joins group 1 through row 1 only
        if n >= 7:
            a, b = n // 3, 2 * n // 3
            V.append((flat(n), _clique(range(0, a)) | _clique(range(a, n))))  # two groups
            V.append((flat(n), _clique(range(0, a)) | _clique(range(a, b)) | _clique(range(b, n))))  # three groups
            V.append((flat(n), _clique(range(0, n, 2)) | _clique(range(1, n, 2))))  # two groups, interleaved
        # weak and best-scoring arcs in every position relative to arc 0, over a random relation of a few local pairs
        for k in range(6 if n <= 7 else 3):
            sc = rng.choice([100, 100, 99, 90, 60, 30], size=n).tolist()
            if k == 0:
                sc[0] = 100  # arc 0 best
            if k == 1:
                sc[0], sc[-1] = 30, 100  # arc 0 weak, the best arc last
            if k == 2:
                sc[0], sc[n // 2] = 60, 100
            m = min(n * (n - 1) // 2, int(rng.integers(1, 3 * n)))
            loc = set()
            while len(loc) < m:
                i, j = rng.integers(0, n, size=2)
                if i != j:
                    loc.add(frozenset((int(i), int(j))))
            V.append((sc, loc))
    V.append(([100] * 7, set()))  # seven pairwise-distant arcs: n_dist_loci = 7
    V.append(([100, 100, 100], _pairs((0, 1), (1, 2))))  # 0-1 and 1-2 local, 0-2 not: arc 2 joins group 1 through row 1
    if len(V) % 2:
        V.append(([], set()))
    return V


def _device(t, lazy, res_cap=0, gate_closed=0):
    raw = C.CDLL(capi.LIB_HIP)
    n_vtx, n_arc = len(t["vs"]), len(t["s1"])
    aw, vwk = np.zeros(n_arc, dtype=np.uint8), np.zeros(n_vtx, dtype=np.uint8)
    ndl, lens = np.full(n_vtx, -5, dtype=np.int32), np.zeros(4, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = raw.pga_selftest_branch(p(t["vs"]), p(t["ve"]), p(t["s1"]), p(t["agid"]), C.c_int32(n_vtx), C.c_int64(n_arc), p(t["rp"]), C.c_int32(t["Q"]), C.c_int32(t["GL"]),
                                 C.c_double(BD), C.c_double(BDIST), C.c_double(BCUT), C.c_int32(10), C.c_int32(2), C.c_int32(lazy), C.c_int64(res_cap), C.c_int32(gate_closed),
                                 p(aw), p(ndl), p(vwk), p(lens))
    assert rc == 0
    return aw, ndl, vwk, lens.tolist()


@pytest.fixture(scope="module")
def case():
    V = _vertices()
    ref = [br.decide_ref(sc, loc, BD, BDIST, BCUT) for sc, loc in V]
    return V, br.tables(V), ref


def test_the_cases_are_what_they_claim(case):
    """the restatement on the hand-made vertices: the group counts and the stretches the cases are there for"""
    V, _, ref = case
    ndl = {(len(sc), r[1]) for (sc, _), r in zip(V, ref)}
    assert {(7, 7), (7, 2), (7, 3), (3, 1), (64, 64), (63, 3), (64, 2), (65, 65)} <= ndl
    assert any(r[1] == 2 and r[2] == 0 and len(sc) >= 3 for (sc, _), r in zip(V, ref))  # the empty stretch
    assert any(r[1] == 1 and r[2] > 0 for (sc, _), r in zip(V, ref))  # joined group 1 through a later row
    assert any(1 in r[0] for r in ref) and any(2 in r[0] for r in ref)


@pytest.mark.parametrize("lazy", [1, 0])
def test_device_against_the_restatement(built, case, lazy):
    """weak_br of every arc and n_dist_loci of every vertex, for equality; the lengths of the two lists"""
    V, t, ref = case
    aw, ndl, vwk, lens = _device(t, lazy)
    want_aw = [w for r in ref for w in r[0]]
    print("lazy", lazy, "vertices", len(V), "arcs", len(want_aw), "genomes", t["GL"], "lens", lens)
    assert aw.tolist() == want_aw
    assert ndl.tolist() == [r[1] for r in ref]
    assert lens[0] == sum(br.n_pairs(sc, BD, lazy) for sc, _ in V)
    assert lens[1] == (sum(r[2] for (sc, _), r in zip(V, ref) if len(sc) <= br.WAVE) if lazy else 0)
    assert lens[2] == 1 and lens[3] == 0
    for (sc, _), r, w in zip(V, ref, vwk.tolist()):
        if 2 <= len(sc) <= br.WAVE:
            assert w == (1 if any(r[0]) else 0)


def test_both_forms_agree_and_the_lazy_list_is_shorter(built, case):
    _, t, _ = case
    a, b = _device(t, 1), _device(t, 0)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[2].tolist() == b[2].tolist()
    assert a[3][0] + a[3][1] < b[3][0]


def test_a_closed_gate_leaves_everything_alone(built, case):
    _, t, _ = case
    aw, ndl, vwk, lens = _device(t, 1, gate_closed=1)
    assert not aw.any() and not vwk.any() and (ndl == -5).all() and lens[0] == 0 and lens[1] == 0


def test_a_residual_list_beyond_its_room_ends_in_the_repeat(built, case):
    """room for four pairs: the first attempt raises the sticky flag and leaves the length it needed, the second has the room and the same results"""
    _, t, ref = case
    aw, ndl, vwk, lens = _device(t, 1, res_cap=4)
    assert lens[2] == 2 and lens[3] == 0
    assert aw.tolist() == [w for r in ref for w in r[0]] and ndl.tolist() == [r[1] for r in ref]


# ---------------------------------------------------------------------------------------------------------------------------------
# whole runs
# ---------------------------------------------------------------------------------------------------------------------------------
def _run(tmp_path, tag, env, variant, files):
    prefix = str(tmp_path / tag)
    e = {k: v for k, v in os.environ.items() if k not in ("PANGENE_BR_LAZY", "PANGENE_BR_LAZY_RIDE", "PANGENE_LOOP_RES_CAP")}
    r = subprocess.run([sys.executable, _RUN, prefix, variant] + files, env=dict(e, PANGENE_TIMING="1", **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    json.loads(r.stdout.decode().strip().splitlines()[-1])
    return open(prefix + ".gfa", "rb").read(), r.stderr.decode()


_LAZY_RAN = "[pga_branch_loop] lazy rounds"


@pytest.mark.parametrize("env", [{}, {"PANGENE_BR_LAZY": "0"}, {"PANGENE_LOOP_RES_CAP": "2"}, {"PANGENE_BR_LAZY_RIDE": "0"}], ids=["lazy", "full", "res_cap=2", "no_rider"])
def test_max_dist_loci_deletes_segments(built, tmp_path, env):
    """tests/golden/distloci (tests/golden/distloci.json says how it was made and what the reference did with it): segments with n_dist_loci >= 4,
    some deleted by pg_flt_high_occ's max_dist_loci test -- a lazily computed value decides.  The bytes against the reference's md5: the lazy form
    (the residual counts riding in the launch of the hit marking), every pair listed, a residual list that needs the repeat with room, the
    residual counts in a launch of their own."""
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "distloci.json")))
    gfa, err = _run(tmp_path, "d", env, meta["variant"], golden_files("distloci"))
    assert hashlib.md5(gfa).hexdigest() == meta["md5"]
    assert (_LAZY_RAN in err) == (env.get("PANGENE_BR_LAZY") != "0")
    if "PANGENE_LOOP_RES_CAP" in env:
        assert err.count(_LAZY_RAN) >= 2  # P0240's twelve pairwise-distant arcs need 55 residual pairs a side: the queue ran again with room


@pytest.mark.parametrize("live", ["", "1"], ids=["", "live_lists=1"])
@pytest.mark.parametrize("which", ["bact", "human"])
def test_whole_path_both_forms(built, tmp_path, which, live):
    from pangene_amd import synth
    data = synth.bact(8, 300) if which == "bact" else synth.human(6, 400, iso=3)
    files = synth.write_files(data, str(tmp_path / "in"))
    env = {"PANGENE_LIVE_LISTS": live} if live else {}
    if which == "human":
        env["LOOP_TAIL_EXACT"] = "1"  # (the isoforms' ties: in exact mode 2 the rounds of this set are host-driven, and nothing would be lazy)
    a, err_a = _run(tmp_path, "a", env, "", files)
    b, err_b = _run(tmp_path, "b", dict(env, PANGENE_BR_LAZY="0"), "", files)
    assert len(a) > 1000 and a == b
    queued = "[pga_branch_loop] counters" in err_a
    print(which, repr(live), "rounds queued:", queued, "lazy:", _LAZY_RAN in err_a)
    assert (_LAZY_RAN in err_a) == queued and _LAZY_RAN not in err_b
    assert queued or which == "human"  # the bacterial set's rounds are queued: the comparison is about the lazy form
