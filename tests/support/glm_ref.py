"""TEST INFRASTRUCTURE: a numpy restatement of pangene glm (include/pangene_amd.h pg_glm_opt_t, pg_pan_glm; DESIGN.md section 8
"Structure-adjusted association") for tests/test_glm.py, tests/test_glm_gpu.py and tests/support/glm_direct.py: the null fits, the sums,
V, Z, p by math.erfc, Benjamini-Hochberg and lambda, with an 80-bit (numpy.longdouble) variant of the sums and V, the parser of the
printed text, and the checks of a result against the restatement.  No tolerance is taken from the code under test:
  a raw sum   |S - S_ref| <= 4 A 2^-53 sum over the gene's assemblies of |cols_i|: the bound of a dot product for any order of the sum
              (the factor 4 as in pcoa_direct.py).  U and s_w are raw sums.
  V           |V - V_ref| <= tolV s_w with tolV = max(16 x the largest |V_np64 - V_np80| / s_w the restatement shows on the inputs of
              the test, 8 (k + 3) A 2^-53).
  Z, Beta, SE, p, q, Lambda: what follows from those two by first-order propagation (below), plus 5e-6 relative for %.6g.  q carries
              the largest relative bound of a p of its trait (Benjamini-Hochberg is continuous in p), Lambda the largest bound of a Z^2
              (a median moves by no more than its inputs do).
  axes        on the command line the covariates are the library's own principal coordinates.  pcoa_ref.py holds a coordinate to
              1e-7 sqrt(l_1) where the gap to the next eigenvalue is 0.01 l_1 (Davis-Kahan from the stopping rule, times ten), that is to
              1e-9 l_1 / gap in general; what matters here is the span of the axes used, so the gap is the one behind the LAST axis used.
              `delta`, that bound in units of a unit-variance axis, enters U and V to first order: each of the k + 1 columns of Z moves
              eta_i by at most delta |beta_j|, so r_i and w_i by at most delta |beta|_1 w_i <= delta |beta|_1 / 4, and w z_ij by delta
              more; the factor 4 (k + 1) (1 + |beta|_1) covers that and the refit.  Where delta is above 1e-4 the span of the axes is not
              determined well enough and the numbers are not compared.  With explicit covariates delta is 0.
  thresholds  Fit and collinear are compared only where the restatement is a factor 100 clear of the threshold: V / s_w outside
              [1e-10, 1e-6]; a last step above 1e-7 when the cap ends the fit, a fit that converges before the last two iterations, every
              pivot a hundred times the cut, and max |eta| a hundred times its own uncertainty (1e-9 sum |z_ij|) away from 30.  Iter +-1."""
import gzip
import math

import numpy as np

EPS = 2.0 ** -53
TEXT = 5e-6
COLLINEAR = 1e-8
PIVOT = 1e-12
CHI2_MEDIAN = 0.4549364
MAX_ITER, MAX_HALVE, STEP, ETA, LL_NOISE = 30, 10, 1e-9, 30.0, 1e-10


def cholesky(H):
    """L (lower) of H, or None when a pivot is not above PIVOT times its diagonal entry"""
    n = H.shape[0]
    L = np.zeros_like(H)
    for j in range(n):
        d = H[j, j] - L[j, :j] @ L[j, :j]
        if not d > PIVOT * H[j, j]:
            return None
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (H[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def _solve(L, b):
    y = np.linalg.solve(L, b)
    return np.linalg.solve(L.T, y)


def _loglik(y, eta):
    return float(np.sum(y * eta - (np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta))))))


def null_fit(y, Z, family):
    """The null model of y (N,) on Z (N, k + 1, the first column ones): a dict fit, iter, r, w, L (of Z'WZ), beta and `clear`: whether
    the decision `fit` stands a factor 100 away from each of its thresholds (the cap, |eta| = 30, the pivots)."""
    N, k1 = Z.shape
    out = {"fit": 0, "iter": 0, "clear": True}
    if family == "quant":
        H = Z.T @ Z
        L = cholesky(H)
        if L is None:
            return out
        beta = _solve(L, Z.T @ y)
        res = y - Z @ beta
        s2 = float(res @ res) / (N - k1)
        if not s2 > 0:
            return out
        out.update(fit=1, r=res / s2, w=np.full(N, 1.0 / s2), L=L / math.sqrt(s2), beta=beta, clear=_pivots_clear(H) and s2 > 1e-20 * float(y @ y))
        return out
    beta = np.zeros(k1)
    ybar = float(y.mean())
    beta[0] = math.log(ybar / (1.0 - ybar))
    ll = _loglik(y, Z @ beta)
    converged, steps = False, []
    for it in range(1, MAX_ITER + 1):
        with np.errstate(over="ignore"):
            mu = 1.0 / (1.0 + np.exp(-(Z @ beta)))
        w = mu * (1.0 - mu)
        H = Z.T @ (Z * w[:, None])
        L = cholesky(H)
        if L is None:
            out["iter"] = it - 1
            out["clear"] = False  # (a failed pivot under way: which iteration meets it depends on rounding)
            return out
        d = _solve(L, Z.T @ (y - mu))
        for h in range(MAX_HALVE + 1):
            cand = beta + d
            llc = _loglik(y, Z @ cand)
            if llc >= ll - LL_NOISE * (1.0 + abs(ll)) or h == MAX_HALVE:  # (a fall within the rounding of the sum is none)
                break
            d = d * 0.5
        beta, ll = cand, llc
        out["iter"] = it
        steps.append(float(np.abs(d).max()))
        if steps[-1] <= STEP:
            converged = True
            break
    if not converged:
        out["clear"] = steps[-1] > 100 * STEP
        return out
    # the cap: Newton converges quadratically, so two builds differ by at most one iteration (Iter +-1); Fit then hangs on the cap only
    # for a fit that converges in the last two iterations.  |eta| = 30: a coefficient is settled to 1e-9, so an eta to 1e-9 sum |z_ij|;
    # the decision is clear when max |eta| is a hundred times that away from 30
    clear = out["iter"] <= MAX_ITER - 2
    eta = Z @ beta
    big = float(np.abs(eta).max())
    slack = 100 * STEP * float(np.abs(Z).sum(axis=1).max())
    out["clear"] = clear and abs(big - ETA) >= slack
    if big > ETA:
        return out
    mu = 1.0 / (1.0 + np.exp(-eta))
    w = mu * (1.0 - mu)
    H = Z.T @ (Z * w[:, None])
    L = cholesky(H)
    if L is None:
        out["clear"] = False
        return out
    out.update(fit=1, r=y - mu, w=w, L=L, beta=beta)
    out["clear"] = out["clear"] and _pivots_clear(H)
    return out


def _pivots_clear(H):
    """every pivot of the factorisation at least 100 PIVOT of its diagonal entry"""
    n = H.shape[0]
    L = np.zeros_like(H)
    for j in range(n):
        d = H[j, j] - L[j, :j] @ L[j, :j]
        if not d > 100 * PIVOT * H[j, j]:
            return False
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (H[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return True


def columns(valid, r, w, Zc, A):
    """cols (A, 16): valid, r, w, w z_1 .. for the assemblies `valid` (indices), zero rows elsewhere"""
    c = np.zeros((A, 16))
    c[valid, 0] = 1.0
    c[valid, 1] = r
    c[valid, 2] = w
    k = Zc.shape[1] - 1
    c[valid, 3:3 + k] = w[:, None] * Zc[:, 1:]
    return c


def sums(P, cols, dtype=np.float64):
    """S (G, 16) = P . cols in `dtype`"""
    return np.asarray(P, dtype=dtype) @ np.asarray(cols, dtype=dtype)


def v_of(S, L, dtype=np.float64):
    """V (G,) = S_2 - |L^-1 (S_2 ..)|^2 by forward substitution in `dtype`"""
    k1 = L.shape[0]
    L = np.asarray(L, dtype=dtype)
    b = np.asarray(S[:, 2:2 + k1], dtype=dtype)
    y = np.zeros_like(b)
    for i in range(k1):
        y[:, i] = (b[:, i] - y[:, :i] @ L[i, :i]) / L[i, i]
    return np.asarray(S[:, 2], dtype=dtype) - (y * y).sum(axis=1)


def bh(p):
    p = np.asarray(p, dtype=np.float64)
    m = len(p)
    q = np.zeros(m)
    idx = np.argsort(p, kind="stable")
    run = 1.0
    for j in range(m, 0, -1):
        run = min(run, p[idx[j - 1]] * m / j)
        q[idx[j - 1]] = run
    return q


def one_trait(P, val, cov, family, min_count=1, delta=0.0):
    """One trait over P (G, A) bool, val (A,) with NaN = missing, cov (A, k): a dict with N, summary, skip (0, 1: N < k + 3, 2: one value),
    fit, iter, clear and, when fit: cols, L, S, a, U, s_w, V, V80, tolV, eU, eV (the bounds of U and V per gene), eligible, collinear,
    margin (per gene: True when the collinear decision is a factor 100 clear), tested (indices), beta, se, z, p, q, lam and the bounds
    ez, ebeta, ese, ep, eq (per tested gene), elam."""
    P = np.asarray(P, dtype=bool)
    G, A = P.shape
    cov = np.zeros((A, 0)) if cov is None else np.asarray(cov, dtype=np.float64).reshape(A, -1)
    k = cov.shape[1]
    valid = np.flatnonzero(~np.isnan(val))
    N = len(valid)
    y = val[valid]
    r = {"N": N, "k": k, "summary": float(y.sum()) if family == "binary" else (float(y.mean()) if N else 0.0), "skip": 0, "fit": 0, "iter": 0, "clear": True}
    if N < k + 3:
        r["skip"] = 1
        return r
    if np.all(y == y[0]):
        r["skip"] = 2
        return r
    Zc = np.hstack([np.ones((N, 1)), cov[valid]])
    nf = null_fit(y, Zc, family)
    r.update(fit=nf["fit"], iter=nf["iter"], clear=nf["clear"])
    if not nf["fit"]:
        return r
    cols = columns(valid, nf["r"], nf["w"], Zc, A)
    S = sums(P, cols)
    S80 = sums(P, cols, np.longdouble)
    V = v_of(S, nf["L"])
    V80 = np.asarray(v_of(S80, nf["L"], np.longdouble), dtype=np.float64)
    a = P[:, valid].sum(axis=1)
    sw = S[:, 2]
    elig = np.minimum(a, N - a) >= min_count
    with np.errstate(divide="ignore", invalid="ignore"):
        shown = np.where(sw > 0, np.abs(V - V80) / np.where(sw > 0, sw, 1.0), 0.0)
    tolV = max(16.0 * float(shown[elig].max() if elig.any() else 0.0), 8.0 * (k + 3) * A * EPS)
    absS = sums(P, np.abs(cols))
    spread = 4.0 * (k + 1) * delta * (1.0 + float(np.abs(nf["beta"]).sum()))
    eU = 4.0 * A * EPS * absS[:, 1] + spread * (absS[:, 1] + absS[:, 2])
    eV = (tolV + spread) * sw
    collinear = ~(V > COLLINEAR * sw)
    margin = (V > 100 * COLLINEAR * sw) | (V < COLLINEAR * sw / 100)
    tested = np.flatnonzero(elig & ~collinear)
    U = S[:, 1]
    Vt, Ut = V[tested], U[tested]
    z = Ut / np.sqrt(Vt)
    p = np.array([math.erfc(abs(x) / math.sqrt(2.0)) for x in z])
    q = bh(p)
    # first-order propagation of eU and eV (a second-order allowance of 1 per cent on top)
    relV = eV[tested] / Vt
    ez = 1.01 * (eU[tested] / np.sqrt(Vt) + np.abs(z) * 0.5 * relV / np.maximum(1.0 - relV, 1e-300))
    ebeta = 1.01 * (eU[tested] / Vt + np.abs(Ut / Vt) * relV / np.maximum(1.0 - relV, 1e-300))
    ese = 1.01 * (0.5 * relV / np.maximum(1.0 - relV, 1e-300) / np.sqrt(Vt))
    ep = np.array([abs(math.erfc(max(abs(x) - e, 0.0) / math.sqrt(2.0)) - math.erfc((abs(x) + e) / math.sqrt(2.0))) for x, e in zip(z, ez)])
    rel_p = float(np.max(ep / np.maximum(p, 1e-300))) if len(p) else 0.0
    ez2 = 2 * np.abs(z) * ez + ez * ez
    r.update(cols=cols, L=nf["L"], S=S, a=a, U=U, s_w=sw, V=V, V80=V80, tolV=tolV, eU=eU, eV=eV, eligible=elig, collinear=collinear, margin=margin, tested=tested,
             beta=Ut / Vt, se=1.0 / np.sqrt(Vt), z=z, p=p, q=q, lam=float(np.median(z * z)) / CHI2_MEDIAN if len(z) else None, ez=ez, ebeta=ebeta, ese=ese, ep=ep,
             eq=q * rel_p, elam=float(ez2.max()) / CHI2_MEDIAN if len(z) else 0.0, null_beta=nf["beta"])
    return r


def reference(P, vals, cov, family, min_count=1, delta=0.0):
    vals = np.asarray(vals, dtype=np.float64).reshape(-1, np.asarray(P).shape[1])
    return [one_trait(P, v, cov, family, min_count, delta) for v in vals]


# ---- the fixtures: the genes of a GFA, its trait files, the axes ----

def gene_names(path):
    """the segment names of a GFA in the order dist_ref.read_gfa numbers them"""
    with open(path, "rb") as f:
        head = f.read(2)
    op = gzip.open if head == b"\x1f\x8b" else open
    seg = {}
    with op(path, "rt") as f:
        for l in f.read().split("\n"):
            t = l.rstrip("\r").split("\t")
            if l[:1] == "S" and len(t) >= 3:
                seg.setdefault(t[1], len(seg))
            elif l[:1] == "L" and len(t) >= 5 and t[2] in ("+", "-") and t[4] in ("+", "-"):
                seg.setdefault(t[1], len(seg))
                seg.setdefault(t[3], len(seg))
    return list(seg)


def read_traits(path, asm):
    """(trait names, values (T, A) float64 with NaN = missing) of a trait file"""
    lines = [l for l in open(path).read().split("\n") if l and not l.startswith("#")]
    names = lines[0].split("\t")[1:]
    val = np.full((len(names), len(asm)), np.nan)
    at = {n: i for i, n in enumerate(asm)}
    for l in lines[1:]:
        f = l.split("\t")
        for j, x in enumerate(f[1:]):
            if x not in ("NA", ""):
                val[j, at[f[0]]] = float(x)
    return names, val


def axes(q, F, k):
    """(take, lo, hi): take(n) = (the n unit-variance axes (A, n) of pcoa_ref.reference, delta: the tolerance of their span in units of
    an axis, from the gap behind axis n); lo, hi: the numbers of axes the definition may report for k asked"""
    import pcoa_ref as pc
    B, w, v = pc.reference(q, F)
    A = len(q)
    lo, hi = pc.n_reported(w, k)

    def take(n):
        if n == 0:
            return np.zeros((A, 0)), 0.0
        gap = w[n - 1] - (w[n] if n < len(w) else -np.inf)
        return v[:, :n] * math.sqrt(A), 1e-9 * w[0] / gap * math.sqrt(w[0] / w[n - 1])
    return take, lo, hi


# ---- the printed text ----

def parse(text):
    """the printed table -> dict: head (the fields of the # line), kind ("Cases" or "Mean"), traits {name: dict}, genes {(trait, gene): dict}"""
    if isinstance(text, bytes):
        text = text.decode()
    lines = text.split("\n")
    assert lines[-1] == "" and lines[0].startswith("#\t"), text[:200]
    head = dict(f.split(" ", 1) for f in lines[0].split("\t")[1:])
    th = lines[1].split("\t")
    assert th[:3] == ["T", "Trait", "N"] and th[3] in ("Cases", "Mean") and th[4:] == ["Iter", "Fit", "Tested", "Collinear", "Lambda"], lines[1]
    r = {"head": head, "kind": th[3], "traits": {}, "genes": {}, "order": []}
    at = 2
    while lines[at].startswith("T\t"):
        f = lines[at].split("\t")
        assert len(f) == 9, lines[at]
        r["traits"][f[1]] = {"N": int(f[2]), "summary": float(f[3]), "iter": int(f[4]), "fit": int(f[5]), "tested": int(f[6]), "collinear": int(f[7]),
                             "lam": None if f[8] == "NA" else float(f[8])}
        at += 1
    assert lines[at] == "G\tTrait\tGene\tN\ta\tBeta\tSE\tZ\tp\tq", lines[at]
    for l in lines[at + 1:-1]:
        f = l.split("\t")
        assert f[0] == "G" and len(f) == 10, l
        num = [None if x == "NA" else float(x) for x in f[5:]]
        r["genes"][f[1], f[2]] = dict(zip(("N", "a", "beta", "se", "z", "p", "q"), [int(f[3]), int(f[4])] + num))
        r["order"].append((f[1], f[2]))
    return r


def check_text(got, names, genes, refs, max_p=1.0):
    """A parsed table against the restatement of its traits (refs: one_trait per trait name in `names`).  Returns the list of what is
    wrong; threshold decisions are compared only where the restatement is clear of them."""
    bad = []
    for name, ref in zip(names, refs):
        t = got["traits"].get(name)
        if ref["skip"]:
            if t is not None:
                bad.append("%s: printed, the restatement skips it" % name)
            continue
        if t is None:
            bad.append("%s: no T line" % name)
            continue
        if t["N"] != ref["N"] or abs(t["summary"] - ref["summary"]) > TEXT * abs(ref["summary"]) + 1e-300:
            bad.append("%s: N or summary: %r" % (name, t))
        if ref["clear"] and t["fit"] != ref["fit"]:
            bad.append("%s: Fit %d, the restatement says %d" % (name, t["fit"], ref["fit"]))
        if ref["clear"] and abs(t["iter"] - ref["iter"]) > 1:
            bad.append("%s: Iter %d, the restatement says %d" % (name, t["iter"], ref["iter"]))
        mine = {g: v for (tn, g), v in got["genes"].items() if tn == name}
        if not (ref["fit"] and t["fit"]):
            if mine and ref["clear"]:
                bad.append("%s: gene lines without a fit" % name)
            continue
        n_tested, n_coll, firm = 0, 0, True
        pos = {int(g): i for i, g in enumerate(ref["tested"])}
        for g in np.flatnonzero(ref["eligible"]):
            line = mine.get(genes[g])
            if not ref["margin"][g]:
                firm = False
                continue
            if ref["collinear"][g]:
                n_coll += 1
                if line is None or line["z"] is not None:
                    bad.append("%s %s: collinear in the restatement, printed %r" % (name, genes[g], line))
                continue
            n_tested += 1
            i = pos[int(g)]
            if line is None:
                if ref["p"][i] + ref["ep"][i] <= max_p * (1 - TEXT):
                    bad.append("%s %s: no line, p = %g" % (name, genes[g], ref["p"][i]))
                continue
            if line["z"] is None:
                bad.append("%s %s: printed as collinear, V / s_w = %g" % (name, genes[g], ref["V"][g] / ref["s_w"][g]))
                continue
            if line["N"] != ref["N"] or line["a"] != ref["a"][g]:
                bad.append("%s %s: N, a = %d, %d" % (name, genes[g], line["N"], line["a"]))
            for key, want, tol in (("beta", ref["beta"][i], ref["ebeta"][i]), ("se", ref["se"][i], ref["ese"][i]), ("z", ref["z"][i], ref["ez"][i]),
                                   ("p", ref["p"][i], ref["ep"][i]), ("q", ref["q"][i], ref["eq"][i])):
                if not abs(line[key] - want) <= tol + TEXT * abs(want) + 1e-300:
                    bad.append("%s %s: %s %r, the restatement %r (bound %.3g)" % (name, genes[g], key, line[key], want, tol + TEXT * abs(want)))
        for g in np.flatnonzero(~ref["eligible"]):
            if genes[g] in mine:
                bad.append("%s %s: printed, not eligible" % (name, genes[g]))
        if firm and (t["tested"] != n_tested or t["collinear"] != n_coll):
            bad.append("%s: Tested %d Collinear %d, the restatement %d %d" % (name, t["tested"], t["collinear"], n_tested, n_coll))
        if firm and ref["lam"] is not None and (t["lam"] is None or abs(t["lam"] - ref["lam"]) > ref["elam"] + TEXT * ref["lam"]):
            bad.append("%s: Lambda %r, the restatement %r" % (name, t["lam"], ref["lam"]))
    return bad


def check_values(got, t, ref, against=None):
    """Trait t of the dict capi.pan_glm returns against one_trait's result: a exactly, U and s_w within the sum bound, V within tolV s_w.
    against: a second result dict (the other build) held to the same bounds, twice (each stands within one bound of the restatement)."""
    bad = []
    if got["N"][t] != ref["N"]:
        bad.append("N %d, the restatement %d" % (got["N"][t], ref["N"]))
    if ref["clear"] and (got["fit"][t] != ref["fit"] or abs(got["iterations"][t] - ref["iter"]) > 1):
        bad.append("fit %d iterations %d, the restatement %d %d" % (got["fit"][t], got["iterations"][t], ref["fit"], ref["iter"]))
    if not (ref["fit"] and got["fit"][t]):
        if ref["clear"] and not np.all(got["a"][t] == -1):
            bad.append("values without a fit")
        return bad
    el = ref["eligible"]
    if not np.array_equal(got["a"][t], np.where(el, ref["a"], -1)):
        bad.append("a differs")
    A = ref["cols"].shape[0]
    for key, want, tol in (("U", ref["U"], ref["eU"]), ("s_w", ref["s_w"], 4.0 * A * EPS * ref["s_w"]), ("V", ref["V"], ref["eV"])):
        err = np.abs(got[key][t] - want)[el]
        if np.any(err > tol[el]) or not np.all(np.isfinite(got[key][t])):
            bad.append("%s: off by up to %.3g of the bound" % (key, float((err / np.maximum(tol[el], 1e-300)).max())))
        if against is not None:
            err = np.abs(got[key][t] - against[key][t])[el]
            if np.any(err > 2 * tol[el]):
                bad.append("%s: the two builds differ by up to %.3g of the bound" % (key, float((err / np.maximum(tol[el], 1e-300)).max())))
    if ref["margin"][el].all() and got["tested"][t] != len(ref["tested"]):
        bad.append("tested %d, the restatement %d" % (got["tested"][t], len(ref["tested"])))
    return bad


def two_clades(seed=1, A=96, G=400, markers=60):
    """The planted-structure recipe: two clades of A / 2 assemblies, `markers` noisy clade markers (present in one clade, each cell flipped
    with probability 0.1), the other genes at random with a frequency of their own in [0.2, 0.8], gene `markers` planted: a binary trait
    with logit = -1.2 + 1.6 clade + 2.4 gene.  Returns (P (G, A) bool, y (A,), clade (A,), the markers, the planted gene)."""
    rng = np.random.default_rng(seed)
    clade = (np.arange(A) >= A // 2).astype(np.float64)
    P = rng.random((G, A)) < rng.uniform(0.2, 0.8, size=(G, 1))
    for g in range(markers):
        P[g] = (clade > 0) ^ (rng.random(A) < 0.1)
    planted = markers
    P[planted] = rng.random(A) < 0.5
    eta = -1.2 + 1.6 * clade + 2.4 * P[planted]
    y = (rng.random(A) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    return P, y, clade, np.arange(markers), planted
