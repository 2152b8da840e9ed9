"""TEST INFRASTRUCTURE: a plain numpy restatement of pangene dist (include/pangene_amd.h pg_dist_opt_t, pg_pan_shared) for
tests/test_dist.py and tests/test_dist_gpu.py: its own reading of a GFA's S-, L- and W-lines, the items of each assembly (genes, or the
gene adjacencies of its walks), S = B @ B.T in int64 and the text the command prints."""
import gzip

import numpy as np

METRICS = ("jaccard", "shared", "diff")


def _lines(path):
    with open(path, "rb") as f:
        head = f.read(2)
    op = gzip.open if head == b"\x1f\x8b" else open
    with op(path, "rt") as f:
        return f.read().split("\n")


def read_gfa(path):
    """(names, gene presence (G, A) bool, walks [(assembly, [step, ...]), ...]) as gfa2matrix reads a GFA: segments in the order S- and
    L-lines introduce them, a W-line step whose segment is not known yet is dropped, assemblies = sample#hap in first-seen order;
    step = segment * 2 + (orientation == '<')."""
    seg, names, walks = {}, {}, []
    import re
    for l in _lines(path):
        l = l.rstrip("\r")
        if not l:
            continue
        t = l.split("\t")
        if l[0] == "S" and len(t) >= 3:
            seg.setdefault(t[1], len(seg))
        elif l[0] == "L" and len(t) >= 5 and t[2] in ("+", "-") and t[4] in ("+", "-"):
            seg.setdefault(t[1], len(seg))
            seg.setdefault(t[3], len(seg))
        elif l[0] == "W" and len(t) >= 7:
            a = names.setdefault(t[1] + "#" + t[2], len(names))
            steps = [seg[n] * 2 + (o == "<") for o, n in re.findall(r"([><])([^\s><]+)", t[6]) if n in seg]
            walks.append((a, steps))
    P = np.zeros((len(seg), len(names)), dtype=bool)
    for a, steps in walks:
        for s in steps:
            P[s >> 1, a] = True
    return list(names), P, walks


def adj_presence(walks, A):
    """(n_adjacency, A) bool: consecutive steps (u, v) of one walk, the key min((u, v), (v ^ 1, u ^ 1))"""
    key, cells = {}, []
    for a, steps in walks:
        for u, v in zip(steps, steps[1:]):
            k = min((u, v), (v ^ 1, u ^ 1))
            cells.append((key.setdefault(k, len(key)), a))
    P = np.zeros((len(key), A), dtype=bool)
    for m, a in cells:
        P[m, a] = True
    return P


def presence(path, kind):
    names, P, walks = read_gfa(path)
    return names, (P if kind == "gene" else adj_presence(walks, len(names)))


def shared(P):
    """S (A, A) int64 of a presence matrix (M, A)"""
    B = np.asarray(P, dtype=np.int64).T
    return B @ B.T


def metric(S, name):
    """(A, A): float64 for jaccard, int64 otherwise"""
    n = np.diag(S).astype(np.int64)
    if name == "shared":
        return S.astype(np.int64)
    if name == "diff":
        return n[:, None] + n[None, :] - 2 * S
    u = n[:, None] + n[None, :] - S
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1.0 - S.astype(np.float64) / u.astype(np.float64)
    return np.where(u == 0, 0.0, d)


def text(names, S, name="jaccard", phylip=False):
    """What pangene dist prints"""
    D = metric(S, name)
    fmt = (lambda x: "%.6f" % x) if name == "jaccard" else (lambda x: str(int(x)))
    out = [str(len(names))] if phylip else ["\t".join(["Asm"] + list(names))]
    for i, nm in enumerate(names):
        out.append("\t".join([nm] + [fmt(x) for x in D[i]]))
    return ("\n".join(out) + "\n").encode()
