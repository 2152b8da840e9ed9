"""TEST INFRASTRUCTURE: a plain numpy restatement of pangene coevo (DESIGN.md section 8 "Co-evolution"; include/pangene_amd.h pg_pan_coevo,
include/pangene_hip.h pga_pan_coevo) for tests/test_coevo.py and tests/test_coevo_gpu.py.  Built on gainloss_ref.reconstruct: the event of
item i on the branch above node v is X[v, i] = state[v] - state[parent of v] (1 a gain, -1 a loss; the root, the last node, has no
branch).  The pair counts come from four matrix products over the gain and loss indicators (float32: the counts stay far below 2^24, so
they are exact), the selection is integer arithmetic; the table as the bytes the command prints; a brute force that recounts same and opp
pair by pair with Python loops; and the backend's event rows in op order."""
import math

import numpy as np

import gainloss_ref as gr
import pairs_ref as pr

HEADER = b"ItemA\tItemB\tnA\tnB\teA\teB\tsame\topp\tr\tp_hyper\n"
SIGNS = ("both", "pos", "neg")


def permille(min_r):
    return int(math.floor(1000.0 * min_r + 0.5))


def events(P, kids, g=1, l=1, mode="late"):
    """X int8 (B, M) in node order (branch v = the branch above node v, v < 2 A - 2) and the reconstruction it comes from"""
    res = gr.reconstruct(P, kids, g, l, mode)
    A = np.asarray(P).shape[1]
    n = A + len(kids)
    up = np.full(n, -1, dtype=np.int64)
    for t, (a, b) in enumerate(kids):
        up[a] = up[b] = A + t
    st = res["state"].astype(np.int8)
    return st[:n - 1] - st[up[:n - 1]], res


def select(P, kids, g=1, l=1, mode="late", min_r=0.8, min_events=2, sign="both"):
    """(events int64 (M,), pairs int64 (n, 4) = i, j, same, opp in ascending (i, j))"""
    X, res = events(P, kids, g, l, mode)
    e = np.abs(X).sum(axis=0).astype(np.int64)
    assert np.array_equal(e, res["gains"] + res["losses"])
    el = np.flatnonzero(e >= min_events)
    p = permille(min_r)
    Gm, Lm = (X[:, el] == 1).T.astype(np.float32), (X[:, el] == -1).T.astype(np.float32)
    out = []
    for lo in range(0, len(el), 1024):
        hi = min(lo + 1024, len(el))
        same = (Gm[lo:hi] @ Gm.T + Lm[lo:hi] @ Lm.T).astype(np.int64)
        opp = (Gm[lo:hi] @ Lm.T + Lm[lo:hi] @ Gm.T).astype(np.int64)
        d = same - opp
        ok = 1000000 * d * d >= p * p * e[el[lo:hi]][:, None] * e[el][None, :]
        if sign == "pos":
            ok &= d >= 0
        elif sign == "neg":
            ok &= d < 0
        ok &= np.arange(lo, hi)[:, None] < np.arange(len(el))[None, :]
        a, b = np.nonzero(ok)
        out.append(np.stack([el[a + lo], el[b], same[a, b], opp[a, b]], axis=1))
    pairs = np.concatenate(out, axis=0) if out else np.zeros((0, 4), dtype=np.int64)
    return e, pairs.reshape(-1, 4).astype(np.int64)


def brute(P, kids, i, j, g=1, l=1, mode="late"):
    """(same, opp) of one pair, branch by branch with Python loops over the states"""
    st = gr.reconstruct(P, kids, g, l, mode)["state"]
    A = np.asarray(P).shape[1]
    same = opp = 0
    for t, (a, b) in enumerate(kids):
        for c in (a, b):
            xi, xj = int(st[c, i]) - int(st[A + t, i]), int(st[c, j]) - int(st[A + t, j])
            if xi != 0 and xj != 0:
                if xi == xj:
                    same += 1
                else:
                    opp += 1
    return same, opp


def p_hyper(B, ea, eb, k):
    """P(X >= k), X ~ Hypergeometric(B, ea, eb)"""
    lf = math.lgamma
    lo, hi = max(0, ea + eb - B), min(ea, eb)
    if k <= lo:
        return 1.0
    base = lf(ea + 1) + lf(B - ea + 1) + lf(eb + 1) + lf(B - eb + 1) - lf(B + 1)
    s = sum(math.exp(base - lf(x + 1) - lf(ea - x + 1) - lf(eb - x + 1) - lf(B - ea - eb + x + 1)) for x in range(hi, k - 1, -1))
    return min(s, 1.0)


def rows(item_names, P, e, pairs):
    """the table's lines as tuples: (ItemA, ItemB, nA, nB, eA, eB, same, opp, r, p_hyper)"""
    P = np.asarray(P) != 0
    n = P.sum(axis=1)
    B = 2 * P.shape[1] - 2
    out = []
    for i, j, same, opp in pairs.tolist():
        ea, eb = int(e[i]), int(e[j])
        out.append((item_names[i], item_names[j], int(n[i]), int(n[j]), ea, eb, same, opp, (same - opp) / math.sqrt(ea * eb), p_hyper(B, ea, eb, same + opp)))
    return out


def text(rws):
    return HEADER + b"".join(("%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%.4f\t%.3e\n" % r).encode() for r in rws)


def parse(out):
    """the lines of a printed table as tuples like rows()"""
    lines = out.split(b"\n")
    assert lines[0] + b"\n" == HEADER and lines[-1] == b""
    res = []
    for ln in lines[1:-1]:
        t = ln.decode().split("\t")
        assert len(t) == 10
        res.append((t[0], t[1]) + tuple(int(x) for x in t[2:8]) + (float(t[8]), float(t[9])))
    return res


def compare(out, want_rows):
    """a printed table against rows(): names and integer columns exactly and in order, r within 1e-4 absolute, p_hyper within 1e-3
    relative -- one unit of the last digit the formats print, which is all a second libm may move"""
    got = parse(out)
    assert len(got) == len(want_rows), (len(got), len(want_rows))
    for g_, w in zip(got, want_rows):
        assert g_[:8] == w[:8], (g_, w)
        assert abs(g_[8] - w[8]) <= 1e-4, (g_, w)
        assert abs(g_[9] - w[9]) <= 1e-3 * w[9], (g_, w)


def table_rows(gfa, kind="gene", metric="jaccard", method="upgma", g=1, l=1, mode="late", min_r=0.8, min_events=2, sign="both"):
    """the rows `pangene coevo` prints for a GFA file"""
    names, item_names, P = gr.items(gfa, kind)
    A = len(names)
    if A <= 1 or P.shape[0] == 0:
        return []
    kids = pr.tree(gr.records(P, metric, method), A, method)
    e, pairs = select(P, kids, g, l, mode, min_r, min_events, sign)
    return rows(item_names, P, e, pairs)


def option_args(kind="gene", metric="jaccard", method="upgma", g=1, l=1, mode="late", min_r=0.8, min_events=2, sign="both", max_pair=None):
    """the same options as the arguments of `pangene coevo` and of `pangene --coevo`"""
    sub = ["-t", kind, "-m", metric, "-a", method, "-g", str(g), "-l", str(l), "-e", mode, "-r", "%g" % min_r, "-c", str(min_events), "-s", sign]
    long = ["--coevo=%g" % min_r, "--coevo-type=" + kind, "--coevo-metric=" + metric, "--coevo-method=" + method, "--coevo-gain=%d" % g, "--coevo-loss=%d" % l,
            "--coevo-resolve=" + mode, "--coevo-min=%d" % min_events, "--coevo-sign=" + sign]
    if max_pair is not None:
        sub += ["-x", str(max_pair)]
        long += ["--coevo-max=%d" % max_pair]
    return sub, long


def capi_options(kind="gene", metric="jaccard", method="upgma", g=1, l=1, mode="late", min_r=0.8, min_events=2, sign="both"):
    """the same options as the keywords of capi.coevo_opt"""
    return dict(type=kind, metric=metric, method=method, gain=g, loss=l, mode=mode, min_r=min_r, min_events=min_events, sign=sign)


def event_rows(X_op, el, WB):
    """the backend's event rows: X_op int8 (B, M) in OP order, el the eligible items -> uint32 (E, 2, WB): plane 0 the gains, plane 1 the
    losses, bit k & 31 of word k >> 5 = branch k"""
    B = X_op.shape[0]
    pad = np.zeros((len(el), 2, WB * 32), dtype=np.uint8)
    pad[:, 0, :B] = (X_op[:, el] == 1).T
    pad[:, 1, :B] = (X_op[:, el] == -1).T
    return np.packbits(pad.reshape(len(el), 2, WB, 32), axis=3, bitorder="little").view(np.uint32).reshape(len(el), 2, WB)


# the option sets the fixtures go through
OPTION_SETS = ({"method": "nj"}, {"kind": "adj"}, {"mode": "early", "l": 3}, {"sign": "neg"}, {"min_events": 1, "min_r": 0.5})
