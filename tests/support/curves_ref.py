"""TEST INFRASTRUCTURE: a plain numpy restatement of the accumulation curves (include/pangene_amd.h pg_pan_curves) and the order
generator they are defined with, for tests/test_curves.py and tests/test_curves_gpu.py."""
import numpy as np

M64 = (1 << 64) - 1
STATS = ("pan", "core", "new", "unique")


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def order(A, p, seed=11):
    """Order p of A columns: 0 is the identity, p >= 1 a Fisher-Yates shuffle driven by splitmix64 from (seed << 32) | p."""
    o = list(range(A))
    if p == 0:
        return o
    x = _mix(((seed & 0xFFFFFFFF) << 32) | p)
    for i in range(A - 1, 0, -1):
        x = (x + 0x9E3779B97F4A7C15) & M64
        j = _mix(x) % (i + 1)
        o[i], o[j] = o[j], o[i]
    return o


def _mix_u64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def orders(A, first, n, seed=11):
    """(n, A) int32: row i = order(A, first + i, seed), first >= 1 -- the same swap sequence with the n generators stepped together in
    uint64 arrays (products wrap modulo 2^64), for rows too long for the Python-integer loop of order() (tests/test_trait.py checks
    that the two agree)"""
    assert first >= 1
    o = np.tile(np.arange(A, dtype=np.int32), (n, 1))
    with np.errstate(over="ignore"):
        x = _mix_u64(np.uint64((seed & 0xFFFFFFFF) << 32) | np.arange(first, first + n, dtype=np.uint64))
        rows = np.arange(n)
        for i in range(A - 1, 0, -1):
            x = x + np.uint64(0x9E3779B97F4A7C15)
            j = (_mix_u64(x) % np.uint64(i + 1)).astype(np.int64)
            oi = o[:, i].copy()
            o[:, i] = o[rows, j]
            o[rows, j] = oi
    return o


def curves_one(P, o):
    """(4, A) for one order: cum = P[:, order].cumsum(1); pan = genes with cum > 0, core = cum == k, unique = cum == 1, new = diff(pan)."""
    P = np.asarray(P, dtype=bool)
    G, A = P.shape
    if A == 0:
        return np.zeros((4, 0), dtype=np.int64)
    cum = P[:, o].astype(np.int32).cumsum(1)
    k = np.arange(1, A + 1)
    pan = (cum > 0).sum(0)
    core = (cum == k[None, :]).sum(0)
    unique = (cum == 1).sum(0)
    new = np.diff(np.concatenate([[0], pan]))
    return np.stack([pan, core, new, unique])


def curves(P, n_perm=10, seed=11, perms=None):
    """(4, n_perm, A); perms: only these orders (the others stay 0)"""
    P = np.asarray(P, dtype=bool)
    A = P.shape[1]
    out = np.zeros((4, n_perm, A), dtype=np.int64)
    for p in (range(n_perm) if perms is None else perms):
        out[:, p, :] = curves_one(P, order(A, p, seed))
    return out


def text(out):
    """What pangene curves prints for out (4, n, A)."""
    _, n, A = out.shape
    lines = ["\t".join(["Stat", "Perm"] + [str(k) for k in range(1, A + 1)])]
    for s, name in enumerate(STATS):
        for p in range(n):
            lines.append("\t".join([name, str(p)] + [str(int(v)) for v in out[s, p]]))
    return ("\n".join(lines) + "\n").encode()


def parse_matrix(b):
    """gfa2matrix output -> presence (G, A) bool"""
    rows = b.decode().rstrip("\n").split("\n")
    names = rows[0].split("\t")[1:]
    A = 0 if names == [""] else len(names)  # no W-lines: "Gene<TAB>" and rows "name<TAB>"
    P = np.zeros((len(rows) - 1, A), dtype=bool)
    for i, r in enumerate(rows[1:]):
        v = r.split("\t")[1:]
        if A:
            P[i] = [int(x) > 0 for x in v]
    return P


def u_shaped(G, A, seed):
    """core genes, cloud genes and a few in between: presence (G, A)"""
    rng = np.random.default_rng(seed)
    kind = rng.random(G)
    freq = np.where(kind < 0.4, 1.0 - rng.random(G) * 0.02, np.where(kind < 0.9, rng.random(G) * 3.0 / max(A, 1), rng.random(G)))
    P = rng.random((G, A)) < freq[:, None]
    P[kind < 0.1] = True  # strict core
    return P
