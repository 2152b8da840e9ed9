"""The lean form of the unsharded queued rounds (pga_branch_loop, PANGENE_LOOP_LEAN: a bit mask read at every call, default every part):
  1  the MODE-0 sweeps evaluate their open hits themselves where no sweep of the upload listed one: no k_sweep_slow (k_sweep_rounds, launch_sweep)
  2  no k_gene_arcs_big where no gene can need it; a gene that does voids the run on the device and the queue is repeated with it (status 4)
  4  k_br_finish and k_round_del in one launch (k_br_finish_del)
  8  the round's k_flag_vtx inside the sweep that follows it
Every whole-run case compares PANGENE_LOOP_LEAN=0 (every launch as before) with single bits and with all of them: the GFA with its W lines, the BED lines
of EVERY hit (filtered ones included: the per-hit flag words as the formats print them), the segment table (n_dist_loci, the `del` bits) and the arc table
of the written graph, byte for byte, over two passes of one upload (the second pass is the one that knows the upload: inline sweeps, the learnt gene
kernel); against the reference's md5 where the fixture has one.  The routes are asserted from the hook pga_selftest_loop_route.  Children of their own,
each under a timeout: the switches are part of a process's environment.

The sweep alone (part 1) on crafted shards: tests/support/loop_lean_sweep.py."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT, golden_files

sys.path.insert(0, os.path.join(ROOT, "tests", "support"))
import loop_lean_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

_RUN = os.path.join(ROOT, "tests", "support", "loop_lean_run.py")
_SWEEP = os.path.join(ROOT, "tests", "support", "loop_lean_sweep.py")
_DROP = ("PANGENE_LOOP_LEAN", "PANGENE_SWEEP_INLINE", "PANGENE_LOOP_PAIR_CAP", "PANGENE_GENE_TABLE_LOG2", "PANGENE_BR_LAZY", "PANGENE_LOOP_FUSE", "PANGENE_LIVE_LISTS", "PANGENE_LOOP")
_CACHE = {}
# big_gene: the gene-major index over every hit of the upload, not over those stage A left (a gene's stretch is then what the input says), and every round
# run in full -- no branch round of this tidy graph changes anything, so behind their gates the arc rounds of the queue would find nothing to do and
# never look at the gene
_NO_LIVE = {"PANGENE_LIVE_LISTS": "0", "PANGENE_LOOP": "noskip"}


@pytest.mark.parametrize("shard", lc.NAMES)
def test_inline_sweep(built, shard):
    """list form, inline form and oracle agree on every per-hit array; the hook counts the inline hits; the counters survive every change of form"""
    e = {k: v for k, v in os.environ.items() if k not in _DROP}
    r = subprocess.run([sys.executable, _SWEEP, shard], env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = r.stdout.decode()
    print(out[-1500:])
    assert r.returncode == 0 and "ALL OK" in out, out[-3000:]


def _files(tmp_path_factory, name):
    from pangene_amd import synth
    if name == "distloci":
        return json.load(open(os.path.join(ROOT, "tests", "golden", "distloci.json")))["variant"], golden_files("distloci")
    if name == "bact20":
        return "", golden_files("bact20")
    if name == "hub":
        if ("files", name) not in _CACHE:
            _CACHE["files", name] = synth.write_files(lc.hub_gene(), str(tmp_path_factory.mktemp("lean_" + name)))
        return lc.HUB_VARIANT, _CACHE["files", name]
    key = ("files", name)
    if key not in _CACHE:
        gen = {"bact": lambda: synth.bact(8, 300), "bact2": lambda: synth.bact(8, 300, seed=2), "big512": lambda: lc.big_gene(512), "big513": lambda: lc.big_gene(513)}[name]()
        _CACHE[key] = synth.write_files(gen, str(tmp_path_factory.mktemp("lean_" + name)))
    return "", _CACHE[key]


def _run(tmp_path_factory, name, lean, env=()):
    """{gfa, bed, seg, arc: bytes; info: the child's JSON line}, once per (set, mask, environment)"""
    key = (name, lean, tuple(sorted(dict(env).items())))
    if key not in _CACHE:
        variant, files = _files(tmp_path_factory, name)
        prefix = str(tmp_path_factory.mktemp("lean_run") / "o")
        e = {k: v for k, v in os.environ.items() if k not in _DROP}
        e.update(dict(env), PANGENE_LOOP_LEAN=str(lean))
        r = subprocess.run([sys.executable, _RUN, prefix, variant, "2"] + files, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        out = {k: open(prefix + "." + k, "rb").read() for k in ("gfa", "bed", "seg", "arc")}
        out["info"] = json.loads(r.stdout.decode().strip().splitlines()[-1])
        out["files"] = files
        _CACHE[key] = out
    return _CACHE[key]


def _same(a, b):
    for k in ("gfa", "bed", "seg", "arc"):
        assert a[k] == b[k], "%s differs from the PANGENE_LOOP_LEAN=0 run" % k
    assert len(a["gfa"]) > 1000 and a["info"]["n_seg"] == b["info"]["n_seg"] and a["info"]["n_arc"] == b["info"]["n_arc"]


def _routes(o, lean):
    """the hook's words after pass 1 and pass 2: the queue ran with this mask, and the words hang together"""
    r1, r2 = o["info"]["route"]
    print("lean", lean, "routes", r1, r2)
    assert r1[9] >= 1 and r2[9] > r1[9], "the rounds were not queued: the comparison is about nothing"
    assert r1[0] == lean and r2[0] == lean
    if not lean & 1:
        assert r1[1] == 0 and r2[1] == 0 and r1[2] == 0 and r2[2] == 0
    else:  # the first pass has not seen the upload's slow lists; the second evaluates open hits itself exactly when every list was empty
        assert (r1[1] == 0 or r1[9] > 1) and r1[5] >= 0 and (r2[1] > 0) == (r1[5] == 0) and r2[2] == 0  # (a repeated queue knows what the void one fetched)
    if not lean & 2:
        assert r1[3] == 0 and r2[3] == 0 and r2[4] == 0 and r2[6] == 0
    # bit 8: sweeps of the call that took the round's k_flag_vtx with them (none of these sets runs with live lists)
    assert (r1[7] > 0 and r2[7] > 0) if lean & 8 else (r1[7] == 0 and r2[7] == 0)
    return r1, r2


@pytest.mark.parametrize("lean", [1, 2, 4, 8, 15])
@pytest.mark.parametrize("name", ["distloci", "bact"])
def test_every_part_alone_and_all_together(built, tmp_path_factory, name, lean):
    """tests/golden/distloci: pg_flt_high_occ's max_dist_loci test deletes two segments inside the queue (rounds 1 and 7) -- a lazily finished n_dist_loci
    decides a deletion (the dependency the fused tail keeps inside a workgroup), and the deleted genes' hits are filtered by the sweep that follows.
    synth.bact(8, 300): 281 segments, so 2 S % 4 == 2 and the last workgroup of k_br_finish_del holds one segment."""
    base, o = _run(tmp_path_factory, name, 0), _run(tmp_path_factory, name, lean)
    _routes(base, 0)
    r1, _ = _routes(o, lean)
    _same(o, base)
    if name == "distloci":
        assert hashlib.md5(o["gfa"]).hexdigest() == json.load(open(os.path.join(ROOT, "tests", "golden", "distloci.json")))["md5"]
        assert r1[8] == 242 and o["info"]["n_seg"] == 240
    else:
        assert r1[8] % 2 == 1, "S is even: the last workgroup of the fused tail is not covered"
    if lean & 2:
        assert r1[3] == 1 and r1[4] == 0 and r1[6] == 0  # nothing here needs the second gene kernel: left out, no repeat


def test_an_even_number_of_segments_too(built, tmp_path_factory):
    base, o = _run(tmp_path_factory, "bact2", 0), _run(tmp_path_factory, "bact2", 4)
    r1, _ = _routes(o, 4)
    _same(o, base)
    assert r1[8] % 2 == 0


def test_a_deleted_genes_hits_lie_in_a_halo(built, tmp_path_factory):
    """the flag transform inside the sweep on slots that neighbouring tiles stage too.  From the BED lines of the PANGENE_LOOP_LEAN=0 run: every gene of
    distloci has a vertex when the queue begins (S = the number of genes), so the hits that end without vtx and with flt are those of the two genes the
    queue deleted; their global X positions (per genome: contig, cs, file order) fall into the first or last 32 slots of a 256-hit tile."""
    base, o = _run(tmp_path_factory, "distloci", 0), _run(tmp_path_factory, "distloci", 8)
    _same(o, base)
    per, order = {}, []
    for ln in base["bed"].decode().splitlines():
        f = ln.split("\t")
        g = f[0].split("#")[0]
        if g not in per:
            per[g] = []
            order.append(g)
        tags = {t.split(":")[0]: t.split(":")[2] for t in f[12:]}
        per[g].append((f[0], int(f[1]), len(per[g]), f[3], int(tags["ft"]), int(tags["vt"])))
    assert len({h[3] for hs in per.values() for h in hs}) == o["info"]["route"][0][8] == 242
    x, in_halo, names = 0, 0, set()
    for g in order:
        ctg = {}
        for h in per[g]:
            ctg.setdefault(h[0], len(ctg))
        for h in sorted(per[g], key=lambda h: (ctg[h[0]], h[1], h[2])):
            if h[5] == 0:
                assert h[4] == 1  # PG_SET_FILTER(vtx == 0)
                names.add(h[3])
                in_halo += x % 256 < 32 or x % 256 >= 224
            x += 1
    assert x == base["info"]["hits"] == lc.n_lines(base["files"])
    print("deleted", sorted(names), "hits in halo slots", in_halo)
    assert len(names) == 2 and in_halo > 0


@pytest.mark.parametrize("lean", [2, 15])
def test_a_gene_of_512_hits_stays_in_the_wave_kernel(built, tmp_path_factory, lean):
    """GA_WAVE_HITS = 512: the largest gene the wave kernel takes.  No second gene kernel, no repeat, in either pass."""
    base, o = _run(tmp_path_factory, "big512", 0, _NO_LIVE.items()), _run(tmp_path_factory, "big512", lean, _NO_LIVE.items())
    assert base["info"]["hits"] == lc.n_lines(base["files"]) == 64 * 48  # (every line is a hit of the upload: XBIG's stretch of the index holds 512)
    r1, r2 = _routes(o, lean)
    _same(o, base)
    assert r1[3] == 1 and r2[3] == 1 and r2[4] == 0 and r2[6] == 0 and r2[9] == 2


@pytest.mark.parametrize("lean", [2, 15])
def test_a_gene_of_513_hits_costs_one_repeat_an_upload(built, tmp_path_factory, lean):
    """status 4 once: the repeat runs with k_gene_arcs_big and the upload keeps it -- the second pass takes no repeat"""
    base, o = _run(tmp_path_factory, "big513", 0, _NO_LIVE.items()), _run(tmp_path_factory, "big513", lean, _NO_LIVE.items())
    assert base["info"]["hits"] == lc.n_lines(base["files"]) == 64 * 48 + 1
    assert _routes(base, 0)[1][9] == 2
    r1, r2 = _routes(o, lean)
    _same(o, base)
    assert r1[3] == 0 and r1[4] == 1 and r1[6] == 1 and r1[9] == 2  # the void queue and its repeat
    assert r2[3] == 0 and r2[4] == 1 and r2[6] == 1 and r2[9] == 3  # one more call, no repeat


@pytest.mark.parametrize("lean", [2, 15])
def test_a_gene_with_more_neighbours_than_the_wave_kernels_table(built, tmp_path_factory, lean):
    """loop_lean_cases.hub_gene: gene HUB has 192 hits (the wave kernel stages them all) and about 278 distinct (orientation, target) keys: the wave kernel's
    table of 128 overflows, the workgroup kernel's of 512 does not; no table switch.  Without k_gene_arcs_big behind it the give-up is status 4 once: the
    repeat runs with the kernel, the upload keeps it, the second pass takes no repeat; every table equals the PANGENE_LOOP_LEAN=0 run's (in which
    k_gene_arcs_big takes the gene in every round until the queue deletes it for its degree)."""
    base, o = _run(tmp_path_factory, "hub", 0, _NO_LIVE.items()), _run(tmp_path_factory, "hub", lean, _NO_LIVE.items())
    assert base["info"]["hits"] == lc.n_lines(base["files"]) == 64 * (140 + 3 + 100)
    assert _routes(base, 0)[1][9] == 2 and base["info"]["n_seg"] == 141  # (142 vertices when the queue begins: HUB goes inside it)
    r1, r2 = _routes(o, lean)
    _same(o, base)
    assert r1[8] == 142
    assert r1[3] == 0 and r1[4] == 1 and r1[6] == 1 and r1[9] == 2  # the void queue and its repeat with k_gene_arcs_big
    assert r2[3] == 0 and r2[4] == 1 and r2[6] == 1 and r2[9] == 3  # one more call, no repeat


def test_open_hits_evaluated_in_place_with_the_flag_transform(built, tmp_path_factory):
    """sweep_slow_one<0, true>: the same set has a pile of 100 mutually overlapping hits a genome (more than a window holds: open hits wherever it falls)
    and a deletion inside the queue; with PANGENE_SWEEP_INLINE=1 every sweep of the rounds evaluates its open hits itself, and under bit 8 their partners'
    flag words, read from global memory, pass through k_flag_vtx's transform first.  Against the PANGENE_LOOP_LEAN=0 run in the list form."""
    env = dict(_NO_LIVE, PANGENE_SWEEP_INLINE="1")
    base, o = _run(tmp_path_factory, "hub", 0, _NO_LIVE.items()), _run(tmp_path_factory, "hub", 15, env.items())
    _same(o, base)
    for r in o["info"]["route"]:
        print(r)
        assert r[0] == 15 and r[1] > 0 and r[2] > 0 and r[7] > 0 and r[7] <= r[1]


def test_a_table_of_four_entries(built, expected, tmp_path_factory):
    """PANGENE_GENE_TABLE_LOG2=2: a gene with five neighbours overflows the wave kernel's table -- the same give-up branch of k_gene_arcs_wave_t as a gene of
    513 hits (above: that test is the one that reaches it inside the queue).  On bact20 the table of four overflows in the host-driven arc round in front of
    the queue already, which then never starts (the hook says so: no call); what is held here is that the switch changes nothing about that route."""
    env = {"PANGENE_GENE_TABLE_LOG2": "2"}
    base, o = _run(tmp_path_factory, "bact20", 0, env.items()), _run(tmp_path_factory, "bact20", 2, env.items())
    _same(o, base)
    assert hashlib.md5(o["gfa"]).hexdigest() == expected["bact20"][""]["md5"]
    r1, r2 = o["info"]["route"]
    print(r1, r2)
    assert r2[4] == (1 if r2[9] else 0)  # (should a queue start after all: one repeat for the gene, no more)


@pytest.mark.parametrize("lean", [4, 15])
def test_a_pair_list_beyond_its_room(built, tmp_path_factory, lean):
    """PANGENE_LOOP_PAIR_CAP=8: from the first round whose list does not fit the decision and the finish part leave (the overflow test), the delete part
    still runs -- ungated, on what the rounds before left, as the launch of its own does -- and the repeat with room is clean"""
    env = {"PANGENE_LOOP_PAIR_CAP": "8"}
    base, o = _run(tmp_path_factory, "distloci", 0, env.items()), _run(tmp_path_factory, "distloci", lean, env.items())
    _same(o, base)
    _same(o, _run(tmp_path_factory, "distloci", 0))
    r1, r2 = o["info"]["route"]
    assert r1[0] == lean and r1[9] == 2 and r2[9] == 3  # the queue ran twice in the first pass, once in the second
