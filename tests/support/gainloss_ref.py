"""TEST INFRASTRUCTURE: a plain numpy restatement of pangene gainloss (DESIGN.md section 8 "Gain and loss"; include/pangene_amd.h
pg_pan_gainloss, include/pangene_hip.h pga_pan_gainloss) for tests/test_gainloss.py and tests/test_gainloss_gpu.py.  The definition node
by node over the tree of pairs_ref.tree, every item at once as an int64 vector; both tables as the bytes the command prints; a counter of
how often each of the three ties occurs; a brute force over all inner-node assignments for at most 8 leaves; and the backend's view of
the tree: the postfix program of pairs_ref.program with the node every op makes and the op of its parent."""
import itertools

import numpy as np

import dist_ref as dr
import pairs_ref as pr
import tree_ref as tr

GENE_HEADER = b"Gene\tPresent\tCost\tChanges\tGains\tLosses\tRoot\n"
NODE_HEADER = b"Node\tChild1\tChild2\tLeaves\tPresent\tGains\tLosses\n"
TIES = ("root", "under0", "under1")  # root d = 0; child d = -g under an absent parent; child d = l under a present parent


def reconstruct(P, kids, g=1, l=1, mode="late", ties=None):
    """P (M, A) bool, kids as pairs_ref.tree returns them (node x < A = leaf x, node A + t = join t, the root last).  A dict: present,
    cost, gains, losses, root (int64 (M,)), state (bool (2 A - 1, M)), node_present, node_gains, node_losses (int64 (2 A - 1,)).
    ties, a dict, has the three counts of TIES added to it."""
    P = np.asarray(P) != 0
    M, A = P.shape
    assert A >= 1 and len(kids) == A - 1 and mode in ("late", "early")
    n = A + len(kids)
    w = (g, l)
    C = np.zeros((n, 2, M), dtype=np.int64)
    for x in range(A):
        C[x, 0] = np.where(P[:, x], g + l, 0)
        C[x, 1] = np.where(P[:, x], 0, g + l)
    for t, (a, b) in enumerate(kids):
        for s in (0, 1):
            C[A + t, s] = sum(np.minimum(C[c, s], C[c, 1 - s] + w[s]) for c in (a, b))
    state = np.zeros((n, M), dtype=bool)
    root = n - 1
    state[root] = C[root, 1] < C[root, 0]
    gains, losses = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64)
    node_g, node_l = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    count = dict.fromkeys(TIES, 0)
    count["root"] += int((C[root, 1] == C[root, 0]).sum())
    for t in range(len(kids) - 1, -1, -1):
        p = state[A + t]
        for c in kids[t]:
            # under an absent parent the child switches to 1 when C1 + g < C0, under a present one to 0 when C0 + l < C1; early: <=
            up0, up1 = C[c, 1] + g, C[c, 0] + l
            sw0 = up0 <= C[c, 0] if mode == "early" else up0 < C[c, 0]
            sw1 = up1 <= C[c, 1] if mode == "early" else up1 < C[c, 1]
            count["under0"] += int((~p & (up0 == C[c, 0])).sum())
            count["under1"] += int((p & (up1 == C[c, 1])).sum())
            sw = np.where(p, sw1, sw0)
            state[c] = p ^ sw
            gn, ls = sw & ~p, sw & p
            gains += gn
            losses += ls
            node_g[c], node_l[c] = gn.sum(), ls.sum()
    if ties is not None:
        for k in TIES:
            ties[k] = ties.get(k, 0) + count[k]
    cost = np.where(state[root], C[root, 1], C[root, 0])
    return {"present": P.sum(axis=1).astype(np.int64), "cost": cost, "gains": gains, "losses": losses, "root": state[root].astype(np.int64), "state": state,
            "node_present": state.sum(axis=1).astype(np.int64), "node_gains": node_g, "node_losses": node_l}


def brute(row, kids, g=1, l=1):
    """the smallest g * gains + l * losses over every assignment of the inner nodes of one item; at most 8 leaves"""
    A = len(row)
    assert A <= 8
    best = None
    for inner in itertools.product((0, 1), repeat=len(kids)):
        s = [int(b) for b in row] + list(inner)
        cost = 0
        for t, (a, b) in enumerate(kids):
            for c in (a, b):
                cost += g * (s[A + t] == 0 and s[c] == 1) + l * (s[A + t] == 1 and s[c] == 0)
        best = cost if best is None else min(best, cost)
    return best


def same(got, want):
    """what capi.pan_gainloss returns against reconstruct"""
    return all(np.array_equal(np.asarray(got[k], dtype=np.int64), want[k]) for k in ("present", "cost", "gains", "losses", "root", "node_present", "node_gains", "node_losses"))


def gene_table(item_names, res, min_changes=0):
    out = [GENE_HEADER]
    for i, nm in enumerate(item_names):
        ch = int(res["gains"][i] + res["losses"][i])
        if ch >= min_changes:
            out.append(("%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (nm, res["present"][i], res["cost"][i], ch, res["gains"][i], res["losses"][i], res["root"][i])).encode())
    return b"".join(out)


def node_table(asm_names, kids, res):
    A = len(asm_names)
    name = lambda v: asm_names[v] if v < A else "@%d" % (v - A)  # noqa: E731
    leaves = [1] * A
    for a, b in kids:
        leaves.append(leaves[a] + leaves[b])
    out = [NODE_HEADER]
    for v in range(A + len(kids)):
        kid = (".", ".") if v < A else (name(kids[v - A][0]), name(kids[v - A][1]))
        gl = ("NA", "NA") if v == A + len(kids) - 1 else (str(int(res["node_gains"][v])), str(int(res["node_losses"][v])))
        out.append(("%s\t%s\t%s\t%d\t%d\t%s\t%s\n" % (name(v), kid[0], kid[1], leaves[v], res["node_present"][v], gl[0], gl[1])).encode())
    return b"".join(out)


def items(gfa, kind):
    """(assembly names, item names, presence (M, A) bool) of a GFA as pangene gainloss reads it: genes by name, adjacencies in first-seen
    order, named by their two steps as a walk writes them"""
    names, P, walks = dr.read_gfa(gfa)
    seg = {}
    for ln in dr._lines(gfa):
        t = ln.rstrip("\r").split("\t")
        if ln[:1] == "S" and len(t) >= 3:
            seg.setdefault(t[1], len(seg))
        elif ln[:1] == "L" and len(t) >= 5 and t[2] in ("+", "-") and t[4] in ("+", "-"):
            seg.setdefault(t[1], len(seg))
            seg.setdefault(t[3], len(seg))
    seg_name = list(seg)
    assert len(seg_name) == P.shape[0]
    if kind == "gene":
        return names, seg_name, P
    key = {}
    for _, steps in walks:
        for u, v in zip(steps, steps[1:]):
            key.setdefault(min((u, v), (v ^ 1, u ^ 1)), len(key))
    step = lambda u: ("<" if u & 1 else ">") + seg_name[u >> 1]  # noqa: E731
    return names, [step(u) + step(v) for u, v in key], dr.adj_presence(walks, len(names))


def records(P, metric, method):
    """the records of `pangene tree -m metric -a method` over the items P (M, A); None below 3 assemblies"""
    if P.shape[1] < 3:
        return None
    return tr.joins(tr.fixed(dr.shared(P), metric)[0], method)


def table(gfa, kind="gene", metric="jaccard", method="upgma", g=1, l=1, mode="late", out="gene", min_changes=0):
    """What `pangene gainloss` prints for a GFA file"""
    names, item_names, P = items(gfa, kind)
    A = len(names)
    if A == 0 or P.shape[0] == 0:
        return GENE_HEADER if out == "gene" else NODE_HEADER
    kids = pr.tree(records(P, metric, method), A, method)
    res = reconstruct(P, kids, g, l, mode)
    return gene_table(item_names, res, min_changes) if out == "gene" else node_table(names, kids, res)


def program(kids, A):
    """The backend's view of a tree: (op, order, need) of pairs_ref.program, node_of[k] = the node op k makes, par[k] = the op of its
    parent (-1 for the root, the last op)"""
    op, order, need = pr.program(kids, A)
    up = {}
    for t, (a, b) in enumerate(kids):
        up[a] = up[b] = A + t
    node_of, stack, pushed = [], [], 0
    for o in op:
        if o == 0:
            v = order[pushed]
            pushed += 1
        else:
            v = up[stack.pop()]
            stack.pop()
        stack.append(v)
        node_of.append(v)
    op_of = {v: k for k, v in enumerate(node_of)}
    par = np.array([op_of[up[v]] if v in up else -1 for v in node_of], dtype=np.int32)
    return op, order, need, np.array(node_of, dtype=np.int64), par


def state_words(state_rows, WW):
    """bool (rows, M) -> uint64 (rows, WW): bit i & 63 of word i >> 6 = column i"""
    R, M = state_rows.shape
    pad = np.zeros((R, WW * 64), dtype=np.uint8)
    pad[:, :M] = state_rows
    return np.packbits(pad.reshape(R, WW, 64), axis=2, bitorder="little").view(np.uint64).reshape(R, WW)


def option_args(kind="gene", metric="jaccard", method="upgma", g=1, l=1, mode="late", out="gene", min_changes=0):
    """the same options as the arguments of `pangene gainloss` and of `pangene --gainloss`"""
    sub = ["-t", kind, "-m", metric, "-a", method, "-g", str(g), "-l", str(l), "-r", mode, "-o", out, "-c", str(min_changes)]
    long = ["--gainloss=" + out, "--gainloss-type=" + kind, "--gainloss-metric=" + metric, "--gainloss-method=" + method, "--gainloss-gain=%d" % g,
            "--gainloss-loss=%d" % l, "--gainloss-resolve=" + mode, "--gainloss-min=%d" % min_changes]
    return sub, long


def capi_options(kind="gene", metric="jaccard", method="upgma", g=1, l=1, mode="late", out="gene", min_changes=0):
    """the same options as the keywords of capi.gainloss_opt"""
    return dict(type=kind, metric=metric, method=method, gain=g, loss=l, mode=mode, out=out, min_changes=min_changes)


# the option sets the fixtures go through: defaults; -a nj -g 2; -t adj -m diff -r early -l 3; -o node; -c 2
OPTION_SETS = ({}, {"method": "nj", "g": 2}, {"kind": "adj", "metric": "diff", "mode": "early", "l": 3}, {"out": "node"}, {"min_changes": 2})
