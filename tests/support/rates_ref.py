"""TEST INFRASTRUCTURE: a plain numpy restatement of pangene rates (DESIGN.md section 8 "Gain and loss rates"; include/pangene_amd.h
pg_pan_rates, include/pangene_hip.h pga_pan_rates) for tests/test_rates.py and tests/test_rates_gpu.py, written from the definition and
independent of the product: the branch lengths of the records, the tables, Felsenstein pruning node by node over the tree of
pairs_ref.tree with every item at once as a vector (float64, or numpy.longdouble for the 80-bit variant), the outside pass and the
posteriors, the lattice search with the gap between its best and second-best value, the rate scan, and a brute force over all
2^(A - 1) assignments of the inner nodes for at most 9 leaves."""
import math

import numpy as np

import gainloss_ref as gr
import pairs_ref as pr

EPS = 2.0 ** -53
T_FLOOR = 2.0 ** -20
GENE_HEADER = b"Gene\tPresent\tlnL\tGains\tLosses\tChanges\tRoot\tRate\tLRT\tp_rate\n"
NODE_HEADER = b"Node\tChild1\tChild2\tLeaves\tLength\tPresent\tGains\tLosses\n"
SCAN = tuple(2.0 ** k for k in range(-4, 5))
SCAN_ORDER = (4, 3, 5, 2, 6, 1, 7, 0, 8)  # nearer 1 first, then the smaller


def lengths(rec, A, method):
    """the raw branch length above every node (node ids of pairs_ref.tree; the root's is 0), in record units"""
    kids = pr.tree(rec, A, method)
    n = A + len(kids)
    ln = [0.0] * n
    if A == 2:
        return kids, np.array([0.5, 0.5, 0.0])
    rec = np.asarray(rec, dtype=np.int64).reshape(-1, 6)
    if method == "nj":
        for t in range(A - 3):
            _, _, dij, Ri, Rj, r = (int(v) for v in rec[t])
            li = (dij + (Ri - Rj) / (r - 2)) / 2
            ln[kids[t][0]], ln[kids[t][1]] = li, dij - li
        _, _, _, dxy, dxz, dyz = (int(v) for v in rec[A - 3])
        (x, y), (xy, z) = kids[A - 3], kids[A - 2]
        ln[x], ln[y] = (dxy + dxz - dyz) / 2, (dxy + dyz - dxz) / 2
        ln[xy] = ln[z] = (dxz + dyz - dxy) / 2 / 2
    else:
        height = [0.0] * n
        for t, (a, b) in enumerate(kids):
            h = int(rec[t, 2]) / 2
            ln[a], ln[b] = h - height[a], h - height[b]
            height[A + t] = h
    return kids, np.array(ln)


def normalise(ln):
    """(t, T): max(len, 0) / T floored at 2^-20, the root's 0; T = 0: no model"""
    pos = np.maximum(ln[:-1], 0.0)
    T = float(sum(pos.tolist()))
    t = np.zeros(len(ln))
    if T > 0:
        t[:-1] = np.maximum(pos / T, T_FLOOR)
    return t, T


def tables(lam, mu, t):
    """(tab (n, 4) = P00 P01 P10 P11 per node, pi (2,))"""
    s = lam + mu
    pi1, pi0 = lam / s, mu / s
    q = -np.expm1(-s * np.asarray(t, dtype=np.float64))
    p01, p10 = pi1 * q, pi0 * q
    return np.stack([1.0 - p01, p01, p10, 1.0 - p10], axis=1), np.array([pi0, pi1])


def _rescale(a, b):
    big = np.maximum(a, b)
    _, e = np.frexp(big)
    e = np.where((big > 0) & np.isfinite(big), e, 0).astype(np.int64)
    return np.ldexp(a, -e), np.ldexp(b, -e), e


def up(P, kids, tab, pi, dtype=np.float64, rescale=True):
    """P (M, A) bool.  inn (n, 2, M): the scaled inside vectors, E (n, M): their exponents, and L = m 2^e per item"""
    P = np.asarray(P) != 0
    M, A = P.shape
    n = A + len(kids)
    tab, pi = np.asarray(tab, dtype=dtype), np.asarray(pi, dtype=dtype)
    inn, E = np.zeros((n, 2, M), dtype=dtype), np.zeros((n, M), dtype=np.int64)
    for x in range(A):
        inn[x, 0], inn[x, 1] = ~P[:, x], P[:, x]
    for t, (a, b) in enumerate(kids):
        i0 = (tab[a, 0] * inn[a, 0] + tab[a, 1] * inn[a, 1]) * (tab[b, 0] * inn[b, 0] + tab[b, 1] * inn[b, 1])
        i1 = (tab[a, 2] * inn[a, 0] + tab[a, 3] * inn[a, 1]) * (tab[b, 2] * inn[b, 0] + tab[b, 3] * inn[b, 1])
        e = 0
        if rescale:
            i0, i1, e = _rescale(i0, i1)
        inn[A + t, 0], inn[A + t, 1], E[A + t] = i0, i1, E[a] + E[b] + e
    L = pi[0] * inn[n - 1, 0] + pi[1] * inn[n - 1, 1]
    m, e = np.frexp(L)
    return inn, E, m, np.where(L > 0, e + E[n - 1], 0).astype(np.int64)


def down(inn, kids, tab, pi):
    """(present, gain, loss), each (n, M): every node's posterior presence, and per branch the posterior of absent above / present below
    and the reverse (0 for the root)"""
    n, _, M = inn.shape
    A = n - len(kids)
    out = np.zeros((n, 2, M))
    present, gain, loss = np.zeros((n, M)), np.zeros((n, M)), np.zeros((n, M))
    L = pi[0] * inn[n - 1, 0] + pi[1] * inn[n - 1, 1]
    present[n - 1] = np.where(L > 0, pi[1] * inn[n - 1, 1] / np.where(L > 0, L, 1.0), 0.0)
    out[n - 1, 0], out[n - 1, 1] = pi[0], pi[1]
    for t in range(len(kids) - 1, -1, -1):
        v = A + t
        for c, d in (kids[t], kids[t][::-1]):
            O0 = out[v, 0] * (tab[d, 0] * inn[d, 0] + tab[d, 1] * inn[d, 1])
            O1 = out[v, 1] * (tab[d, 2] * inn[d, 0] + tab[d, 3] * inn[d, 1])
            J00, J01, J10, J11 = O0 * tab[c, 0] * inn[c, 0], O0 * tab[c, 1] * inn[c, 1], O1 * tab[c, 2] * inn[c, 0], O1 * tab[c, 3] * inn[c, 1]
            Z = (J00 + J01) + (J10 + J11)
            ok = Z > 0
            Zs = np.where(ok, Z, 1.0)
            present[c], gain[c], loss[c] = np.where(ok, (J01 + J11) / Zs, 0.0), np.where(ok, J01 / Zs, 0.0), np.where(ok, J10 / Zs, 0.0)
            out[c, 0], out[c, 1], _ = _rescale(O0 * tab[c, 0] + O1 * tab[c, 2], O0 * tab[c, 1] + O1 * tab[c, 3])
    return present, gain, loss


def brute(row, kids, tab, pi):
    """one item by enumeration over all assignments of the inner nodes, A <= 9: (L, present (n,), gain (n,), loss (n,))"""
    A = len(row)
    assert A <= 9
    n, n_in = A + len(kids), len(kids)
    S = np.zeros((1 << n_in, n), dtype=np.int64)
    S[:, :A] = np.asarray(row, dtype=np.int64)
    S[:, A:] = np.arange(1 << n_in)[:, None] >> np.arange(n_in)[None, :] & 1
    w = np.asarray(pi)[S[:, n - 1]].astype(np.float64)
    for t, (a, b) in enumerate(kids):
        for c in (a, b):
            w = w * np.asarray(tab)[c].reshape(2, 2)[S[:, A + t], S[:, c]]
    L = math.fsum(w.tolist())
    present = np.array([math.fsum((w * S[:, v]).tolist()) for v in range(n)]) / L
    gain, loss = np.zeros(n), np.zeros(n)
    for t, (a, b) in enumerate(kids):
        for c in (a, b):
            gain[c] = math.fsum((w * ((S[:, A + t] == 0) & (S[:, c] == 1))).tolist()) / L
            loss[c] = math.fsum((w * ((S[:, A + t] == 1) & (S[:, c] == 0))).tolist()) / L
    return L, present, gain, loss


def ln_of(m, e):
    return np.log(np.asarray(m, dtype=np.float64)) + np.asarray(e, dtype=np.float64) * math.log(2.0)


def loglik(P, kids, t, lam, mu):
    """(ll (M,) = ln L_g - ln(1 - L_absent), LL summed in ascending order, L_absent) over the items of P, none absent everywhere"""
    tab, pi = tables(lam, mu, t)
    Q = np.vstack([np.asarray(P) != 0, np.zeros((1, np.asarray(P).shape[1]), dtype=bool)])
    _, _, m, e = up(Q, kids, tab, pi)
    L0 = math.ldexp(float(m[-1]), int(e[-1]))
    corr = math.log1p(-L0)
    lnl = ln_of(m[:-1], e[:-1])
    s = 0.0
    for v in lnl.tolist():
        s += v
    return lnl - corr, s - len(lnl) * corr, L0


def ll_bound(G, A, LL, L0):
    """The bound on LL at given rates: every ln L_g carries the relative bound 8 (2 A - 1) 2^-53 of its L as an absolute error, the
    correction term ln(1 - L_absent), taken G times, carries that of L_absent times L_absent / (1 - L_absent), and the G + 1 terms are
    added with (G + 1) 2^-53 |LL|"""
    b = 8 * (2 * A - 1) * EPS
    return G * b + G * b * L0 / (1.0 - L0) + (G + 1) * EPS * abs(LL)


def search(P, kids, t):
    """The lattice search: (lambda, mu, rounds, converged, gap), gap = the smallest difference between the best and the second-best
    lattice value over all rounds, and path = the best index of every round"""
    cx = cy = 0.0
    h, moves, rounds, gap, path = 2.0, 0, 0, math.inf, []
    while True:
        vals = [loglik(P, kids, t, 2.0 ** (cx + (i - 2) * h), 2.0 ** (cy + (j - 2) * h))[1] for i in range(5) for j in range(5)]
        rounds += 1
        best = max(range(25), key=lambda s: (vals[s], -s))
        gap = min(gap, vals[best] - sorted(vals)[-2])
        path.append(best)
        bi, bj = divmod(best, 5)
        cx, cy = min(max(cx + (bi - 2) * h, -20.0), 20.0), min(max(cy + (bj - 2) * h, -20.0), 20.0)
        if (bi in (0, 4) or bj in (0, 4)) and moves < 16:
            moves += 1
            continue
        if h <= 2.0 ** -10:
            break
        h /= 2
    conv = int(not (abs(cx) >= 20 or abs(cy) >= 20 or moves >= 16))
    return 2.0 ** cx, 2.0 ** cy, rounds, conv, gap, path


def model(P, rec, method, gain=None, loss=None):
    """What capi.pan_rates returns, from the definition; fitted when gain is None.  Also gap and path of the search, bound (of lnL),
    and the per-branch matrices present, gain_b, loss_b (n, G used)."""
    P = np.asarray(P) != 0
    M, A = P.shape
    nan = float("nan")
    kids, ln = (pr.tree(rec, A, method), np.zeros(max(2 * A - 1, 0))) if A < 2 else lengths(rec, A, method)
    n = len(ln)
    t, T = normalise(ln) if A >= 2 else (ln, 0.0)
    res = {"gain": nan, "loss": nan, "lnL": nan, "rounds": 0, "converged": 0, "T": T, "node_length": t.copy()}
    for k in ("lnL_item", "gains", "losses", "root", "rate", "lrt", "p_rate"):
        res[k] = np.full(M, nan)
    for k in ("node_present", "node_gains", "node_losses"):
        res[k] = np.zeros(n)
    used = np.nonzero(P.any(axis=1))[0] if A else np.zeros(0, dtype=np.int64)
    res["used"] = used
    if A < 2 or not T > 0 or len(used) == 0:
        return res
    Pu = P[used]
    if gain is None:
        lam, mu, res["rounds"], res["converged"], res["gap"], res["path"] = search(Pu, kids, t)
    else:
        lam, mu, res["converged"] = float(gain), float(loss), 1
    res["gain"], res["loss"] = lam, mu
    ll, LL, L0 = loglik(Pu, kids, t, lam, mu)
    res["lnL"], res["bound"] = LL, ll_bound(len(used), A, LL, L0)
    tab, pi = tables(lam, mu, t)
    inn, _, _, _ = up(Pu, kids, tab, pi)
    present, g, l = down(inn, kids, tab, pi)
    res["present"], res["gain_b"], res["loss_b"] = present, g, l
    res["gains"][used], res["losses"][used], res["root"][used] = g.sum(axis=0), l.sum(axis=0), present[n - 1]
    res["node_present"], res["node_gains"], res["node_losses"] = present.sum(axis=1), g.sum(axis=1), l.sum(axis=1)
    lls = np.stack([loglik(Pu, kids, t, r * lam, r * mu)[0] for r in SCAN])
    best = np.full(len(used), 4)
    for r in SCAN_ORDER:
        best = np.where(lls[r] > lls[best, np.arange(len(used))], r, best)
    lrt = np.maximum(2.0 * (lls[best, np.arange(len(used))] - lls[4]), 0.0)
    res["lnL_item"][used], res["rate"][used], res["lrt"][used] = lls[4], np.asarray(SCAN)[best], lrt
    res["p_rate"][used] = [math.erfc(math.sqrt(v / 2.0)) for v in lrt.tolist()]
    res["scan"] = lls
    return res


def tolerances(A, n_sum=0):
    """(L, posterior, node total): the relative bounds of DESIGN.md section 8 "Gain and loss rates", Tests, for a tree of A leaves"""
    return 8 * (2 * A - 1) * EPS, 32 * (2 * A - 1) * EPS, 32 * (2 * A - 1) * EPS + n_sum * EPS


def close(got, want, rel, absolute=1e-200):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= rel * np.abs(want) + absolute))


def items_tree(gfa, kind="gene", metric="jaccard", method="upgma"):
    """(assembly names, item names, P, records) of a GFA as pangene rates reads it"""
    names, item_names, P = gr.items(gfa, kind)
    return names, item_names, P, (gr.records(P, metric, method) if len(names) >= 3 else None)


def parse(text):
    """The bytes `pangene rates` prints: (header line, the fields of the # line as a dict, the rows as lists of fields)"""
    lines = text.decode().split("\n")
    assert lines[-1] == ""
    head, rows, info = lines[0] + "\n", [], None
    for ln in lines[1:-1]:
        if ln.startswith("#"):
            info = dict(f.split("=", 1) for f in ln.split("\t")[1:])
        else:
            rows.append(ln.split("\t"))
    return head.encode(), info, rows


def option_args(kind="gene", metric="jaccard", method="upgma", gain=None, loss=None, out="gene", min_changes=0):
    """the same options as the arguments of `pangene rates` and of `pangene --rates`"""
    sub = ["-t", kind, "-m", metric, "-a", method, "-o", out, "-c", repr(float(min_changes))]
    long = ["--rates=" + out, "--rates-type=" + kind, "--rates-metric=" + metric, "--rates-method=" + method, "--rates-min=" + repr(float(min_changes))]
    if gain is not None:
        sub += ["-g", repr(float(gain)), "-l", repr(float(loss))]
        long += ["--rates-gain=" + repr(float(gain)), "--rates-loss=" + repr(float(loss))]
    return sub, long


def check_table(text, gfa, kind="gene", metric="jaccard", method="upgma", gain=None, loss=None, out="gene", min_changes=0):
    """The printed table against the restatement: "" when it agrees, else what differs.  With given rates every number is compared; a
    fitted table is compared at the rates it prints: lnL, and the structure of the rows"""
    names, item_names, P, rec = items_tree(gfa, kind, metric, method)
    M, A = P.shape
    head, info, rows = parse(text)
    if head != (GENE_HEADER if out == "gene" else NODE_HEADER):
        return "header"
    if A < 2 or M == 0:
        return "" if info is None and not rows else "rows without a model"
    if info is None:
        return "no # line"
    pr6 = 5e-6
    lam, mu = float(info["gain"]), float(info["loss"])
    if gain is not None and not (close(lam, gain, pr6) and close(mu, loss, pr6)):
        return "the given rates"
    # A fitted table prints its rates with six digits, which is not enough to recompute its posteriors within their bounds: of such a
    # table lnL is compared at the printed rates (near the optimum 5e-6 of a rate moves lnL by far less than its own six digits) and the
    # rows by their structure; every number of a fitted model is compared through pg_pan_rates, which returns the rates in full.
    given = gain is not None
    want = model(P, rec, method, gain if given else lam, loss if given else mu)
    tol_L, tol_post, tol_node = tolerances(A, M)
    if int(info["A"]) != A or int(info["G"]) != len(want["used"]) or info["items"] != kind or info["metric"] != metric or info["method"] != method:
        return "the # line: %s" % info
    if not close(float(info["lnL"]), want["lnL"], pr6, want["bound"]):
        return "lnL %s against %r" % (info["lnL"], want["lnL"])
    if out == "gene":
        got = [r[0] for r in rows]
        at = {item_names[i]: i for i in want["used"]}
        if len(set(got)) != len(got) or not set(got) <= set(at) or (min_changes == 0 and len(got) != len(at)):
            return "the items printed"
        if given:  # an item whose Changes are within their tolerance of the threshold may go either way
            ch = want["gains"] + want["losses"]
            sure_in = set(item_names[i] for i in want["used"] if ch[i] * (1 - tol_post) > min_changes)
            sure_out = set(item_names[i] for i in want["used"] if ch[i] * (1 + tol_post) < min_changes)
            if not sure_in <= set(got) or set(got) & sure_out:
                return "the items the threshold keeps"
        ll_abs = 2 * tol_L * (1 + abs(want["lnL"]) / max(len(want["used"]), 1))  # of one item's lnL: its L, the correction, and the two roundings of the logarithms
        for k, r in enumerate(rows):
            i = at[r[0]]
            v = [float(x) for x in r[1:]]
            if v[0] != int(P[i].sum()) or (k > 0 and at[rows[k - 1][0]] >= i):
                return "item %s: Present or the order" % r[0]
            if not given:
                continue
            w = [want["lnL_item"][i], want["gains"][i], want["losses"][i], want["gains"][i] + want["losses"][i], want["root"][i]]
            if not (close(v[1], w[0], pr6, ll_abs) and close(v[2:6], w[1:], pr6 + tol_post)):
                return "item %s: %s against %s" % (r[0], v, w)
            # the scan: the multiplier printed is the restatement's, or one whose lnL is within the bound of it; LRT is a difference of two
            # lnL; p_rate is erfc(sqrt(LRT / 2)) of the value printed, and d ln erfc(x) / dx is about -2 x, so that the six digits of LRT
            # move it by up to 2.5e-6 LRT relatively
            u = list(np.nonzero(want["used"] == i)[0])[0]
            col = want["scan"][:, u]
            if v[6] not in SCAN or col[SCAN.index(v[6])] < col.max() - 4 * ll_abs:
                return "the multiplier of item %s: %s" % (r[0], v[6])
            if not close(v[7], want["lrt"][i], pr6, 8 * ll_abs):
                return "LRT of item %s: %s against %s" % (r[0], v[7], want["lrt"][i])
            if not close(v[8], math.erfc(math.sqrt(v[7] / 2.0)), 5e-6 * (2.0 + v[7])):
                return "p_rate of item %s: %s" % (r[0], v[8])
        return ""
    kids = pr.tree(rec, A, method)
    if len(rows) != A + len(kids):
        return "the number of nodes"
    name = lambda v: names[v] if v < A else "@%d" % (v - A)  # noqa: E731
    leaves = [1] * A
    for a, b in kids:
        leaves.append(leaves[a] + leaves[b])
    for v, r in enumerate(rows):
        kid = [".", "."] if v < A else [name(kids[v - A][0]), name(kids[v - A][1])]
        if r[:4] != [name(v)] + kid + [str(leaves[v])]:
            return "node %d: %s" % (v, r[:4])
        if not close(float(r[4]), want["node_length"][v], pr6):
            return "node %d: length %s" % (v, r)
        if v == len(rows) - 1 and r[6:] != ["NA", "NA"]:
            return "the root's NA"
        if not given:
            continue
        if not close(float(r[5]), want["node_present"][v], pr6 + tol_node):
            return "node %d: present %s against %s" % (v, r, want["node_present"][v])
        if v < len(rows) - 1 and not (close(float(r[6]), want["node_gains"][v], pr6 + tol_node) and close(float(r[7]), want["node_losses"][v], pr6 + tol_node)):
            return "node %d: %s against %s %s" % (v, r, want["node_gains"][v], want["node_losses"][v])
    return ""


# the option sets the fixtures go through: given rates (three), then the fit (two)
OPTION_SETS = ({"gain": 1.5, "loss": 2.0}, {"gain": 0.25, "loss": 3.0, "method": "nj", "out": "node"},
               {"gain": 2.0, "loss": 0.5, "kind": "adj", "metric": "diff", "min_changes": 1.0}, {}, {"method": "nj", "out": "node"})


def capi_options(kind="gene", metric="jaccard", method="upgma", gain=None, loss=None, out="gene", min_changes=0):
    return dict(type=kind, metric=metric, method=method, out=out, gain=gain or 0.0, loss=loss or 0.0, min_changes=min_changes)


def fit_same(lib, M, A, seed, method):
    """A named case of the fit: the restatement's gap between the best and the second-best lattice value is at least 100 times the bound
    on lnL, so the lattice paths must coincide -- the rounds, and the rates at 1e-12 -- and every number is compared at those rates"""
    from pangene_amd import capi
    import tree_ref as tr
    P = tr.lineage_presence(M, A, seed)
    rec = gr.records(P, "jaccard", method)
    want = model(P, rec, method)
    if not want["gap"] >= 100 * want["bound"]:
        return False
    got = capi.pan_rates(lib, P, rec, method)
    if not (got["rounds"] == want["rounds"] and got["converged"] == want["converged"] and close(got["gain"], want["gain"], 1e-12) and close(got["loss"], want["loss"], 1e-12)):
        return False
    return model_same(got, model(P, rec, method, got["gain"], got["loss"]), P)


def model_same(got, want, P):
    """what capi.pan_rates returns against the restatement at the same rates"""
    M, A = P.shape
    tol_L, tol_post, tol_node = tolerances(A, M)
    G = len(want["used"])
    ll_abs = 2 * tol_L * (1 + abs(want["lnL"]) / max(G, 1))
    nan_same = all(np.array_equal(np.isnan(got[k]), np.isnan(want[k])) for k in ("lnL_item", "gains", "losses", "root", "rate", "lrt", "p_rate"))
    u = want["used"]
    ok = nan_same and got["T"] == want["T"] and close(got["lnL"], want["lnL"], 0.0, want["bound"])
    ok = ok and close(got["lnL_item"][u], want["lnL_item"][u], 0.0, ll_abs)
    ok = ok and all(close(got[k][u], want[k][u], tol_post) for k in ("gains", "losses", "root"))
    ok = ok and np.array_equal(got["node_length"], want["node_length"]) and all(close(got[k], want[k], tol_node) for k in ("node_present", "node_gains", "node_losses"))
    # the scan: the multiplier is the restatement's, or one whose lnL is within the bound of it; LRT is a difference of two lnL
    col = want["scan"]
    at = np.searchsorted(np.asarray(SCAN), got["rate"][u])
    ok = ok and bool(np.all(col[at, np.arange(G)] >= col.max(axis=0) - 4 * ll_abs)) and close(got["lrt"][u], want["lrt"][u], 0.0, 8 * ll_abs)
    return ok
