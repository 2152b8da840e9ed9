"""TEST INFRASTRUCTURE: a numpy restatement of pangene pcoa (include/pangene_amd.h pg_pcoa_opt_t, pg_pan_pcoa; DESIGN.md section 8
"Principal coordinates") for tests/test_pcoa.py, tests/test_pcoa_gpu.py and tests/support/pcoa_direct.py: B = J A J in float64 and
numpy.linalg.eigh of it, the parser of the printed text, the sign alignment, and ONE check of a result against the reference with the
tolerances of the issue.  None of them is byte equality and none is tuned on the code under test; all follow from the stopping rule
(every wanted Ritz pair has a residual <= 1e-10 l_1):
  eigenvalues   |l_a - l_a^ref| <= 1e-9 l_1^ref: for a symmetric matrix the error of an eigenvalue is at most the residual norm; the
                factor 10 covers the rounding of the products (about N 2^-53 |A|) and numpy's own error.
  coordinates   compared only for an axis whose reference eigenvalue is at least 0.01 l_1 away from both neighbours:
                |x_ia - x_ia^ref| <= 1e-7 sqrt(l_1) after sign alignment (Davis-Kahan: 1e-10 / 0.01 = 1e-8 for the vector, times ten).
  eigenvectors  for EVERY reported axis |B x_a - l_a x_a| <= 1e-9 l_1 sqrt(l_a) with B from numpy (sqrt(l_a) is the norm of x_a).
  orthogonal    |x_a . x_b| <= 1e-9 l_1 for two reported axes further apart than 1e-9 l_1; closer ones share an eigenspace, which the
                residual bound and the orthogonality to the other axes cover as a whole.
  parsed text   the same plus 5e-6 relative, for %.6g.
The reference lives in the centred subspace: eigh of H' B H over the N - 1 columns of a Householder reflection H that are orthogonal
to 1, so that the eigenvalue 0 of the constant vector, which is no axis, does not stand among the reference values."""
import fractions

import numpy as np

KEEP = 1e-9       # axis a is reported when l_a > KEEP l_1
EIG_TOL = 1e-9    # of l_1
GAP = 0.01        # of l_1: the gap rule of the coordinates
COORD_TOL = 1e-7  # of sqrt(l_1)
TEXT = 5e-6       # relative, %.6g


def matrix_b(q, F):
    """B = J A J in float64, A = -1/2 d o d, d = q 2^-F"""
    d = np.asarray(q, dtype=np.float64) * 2.0 ** -F
    A = -0.5 * (d * d)
    rm = A.mean(axis=1)
    B = A - rm[:, None] - rm[None, :] + rm.mean()
    return 0.5 * (B + B.T)


def reference(q, F):
    """(B, the N - 1 eigenvalues in descending order, their unit vectors as columns) in the centred subspace"""
    B = matrix_b(q, F)
    N = B.shape[0]
    u = np.full(N, 1.0 / np.sqrt(N))
    u[0] += 1.0  # H = I - 2 u u' / u'u maps e_1 to -1 / sqrt(N): its other columns span the centred subspace
    H = np.eye(N) - 2.0 * np.outer(u, u) / (u @ u)
    Q = H[:, 1:]
    w, v = np.linalg.eigh(Q.T @ B @ Q)
    return B, w[::-1].copy(), (Q @ v)[:, ::-1].copy()


def trace_exact(q, F):
    """trace(B) = T / (2 N) 4^-F with T = the sum of q^2 over i != j, as a Fraction"""
    q = np.asarray(q, dtype=np.int64)
    T = sum(int(x) * int(x) for x in q.ravel())
    return fractions.Fraction(T, 2 * q.shape[0] * 4 ** F)


def n_reported(w, k):
    """how many axes the definition reports for the reference eigenvalues w: (lowest, highest) count, which differ only where an
    eigenvalue stands within the eigenvalue tolerance of the cut KEEP l_1"""
    k = min(k, len(w))
    if k == 0 or w[0] <= 0:
        return 0, 0
    lo = hi = 0
    for a in range(k):
        if w[a] - EIG_TOL * w[0] > KEEP * w[0] and lo == a:
            lo = a + 1
        if w[a] + EIG_TOL * w[0] > KEEP * w[0] and hi == a:
            hi = a + 1
    return lo, hi


def parse(text):
    """the printed table -> dict: head (the name-value fields of the # line), eig, expl, cum, resid (axes,), names, coord (N, axes)"""
    if isinstance(text, bytes):
        text = text.decode()
    lines = text.split("\n")
    assert lines[-1] == "" and lines[0].startswith("#\t"), text[:200]
    head = dict(f.split(" ", 1) for f in lines[0].split("\t")[1:])
    r = {"head": head, "eig": [], "expl": [], "cum": [], "resid": [], "names": [], "coord": []}
    if len(lines) == 2:
        return r
    assert lines[1] == "EV\tAxis\tEigenvalue\tExplained\tCumulative\tResidual", lines[1]
    at = 2
    while lines[at].startswith("EV\t"):
        f = lines[at].split("\t")
        assert len(f) == 6 and int(f[1]) == len(r["eig"]) + 1, lines[at]
        r["eig"].append(float(f[2])), r["expl"].append(float(f[3])), r["cum"].append(float(f[4])), r["resid"].append(float(f[5]))
        at += 1
    k = len(r["eig"])
    assert lines[at] == "\t".join(["PC", "Asm"] + ["PC%d" % (a + 1) for a in range(k)]), lines[at]
    for l in lines[at + 1:-1]:
        f = l.split("\t")
        assert f[0] == "PC" and len(f) == 2 + k, l
        r["names"].append(f[1]), r["coord"].append([float(x) for x in f[2:]])
    for key in ("eig", "expl", "cum", "resid"):
        r[key] = np.array(r[key], dtype=np.float64)
    r["coord"] = np.array(r["coord"], dtype=np.float64).reshape(len(r["names"]), k)
    return r


def of_text(text):
    """the parsed table as the dict capi.pan_pcoa returns"""
    p = parse(text)
    h = p["head"]
    return {"axes": len(p["eig"]), "steps": int(h["steps"]), "restarts": int(h["restarts"]), "converged": int(h["converged"]), "trace": float(h["trace"]),
            "eig": p["eig"], "resid": p["resid"], "coord": p["coord"], "names": p["names"], "expl": p["expl"], "cum": p["cum"], "N": int(h["N"]), "Fbits": int(h["Fbits"])}


def check(q, F, got, k, text=False, coords=True, ref=None):
    """`got` (the dict of capi.pan_pcoa, or of_text of a printed table) against the reference by the bounds at the head of this file.
    Returns (a list of what is wrong -- empty: all is well, the axes whose coordinates were compared).  text: add 5e-6 relative."""
    B, w, v = ref if ref is not None else reference(q, F)
    N = B.shape[0]
    bad, compared = [], []
    l1 = w[0]
    rel = TEXT if text else 0.0
    lo, hi = n_reported(w, k)
    axes = got["axes"]
    if not lo <= axes <= hi:
        bad.append("axes: %d, the reference gives %d .. %d" % (axes, lo, hi))
        return bad, compared
    tr = float(trace_exact(q, F))
    if abs(got["trace"] - tr) > (2e-15 + rel) * tr:
        bad.append("trace: %r, exact %r" % (got["trace"], tr))
    x = np.asarray(got["coord"], dtype=np.float64).reshape(N, axes)
    for a in range(axes):
        la = got["eig"][a]
        if not np.isfinite(la) or not np.all(np.isfinite(x[:, a])):
            bad.append("axis %d: not finite" % (a + 1))
            continue
        if abs(la - w[a]) > EIG_TOL * l1 + rel * abs(w[a]):
            bad.append("axis %d: eigenvalue %r, reference %r, off by %.3g l_1" % (a + 1, la, w[a], abs(la - w[a]) / l1))
        # an eigenvector in its own right, whatever the gap
        res = np.linalg.norm(B @ x[:, a] - la * x[:, a])
        if res > (EIG_TOL * l1 + rel * (l1 + la)) * np.sqrt(la):  # (text: each coordinate is off by up to 5e-6 of itself, and so is l)
            bad.append("axis %d: |B x - l x| = %.3g = %.3g l_1 sqrt(l)" % (a + 1, res, res / (l1 * np.sqrt(la))))
        if abs(np.linalg.norm(x[:, a]) - np.sqrt(la)) > (1e-12 + 2 * rel) * np.sqrt(la):
            bad.append("axis %d: |x| = %r, sqrt(l) = %r" % (a + 1, np.linalg.norm(x[:, a]), np.sqrt(la)))
        for b in range(a):
            if abs(w[a] - w[b]) > EIG_TOL * l1 and abs(x[:, a] @ x[:, b]) > (EIG_TOL + 2 * rel) * l1:
                bad.append("axes %d and %d: x_a . x_b = %.3g l_1" % (b + 1, a + 1, abs(x[:, a] @ x[:, b]) / l1))
        # the coordinates themselves, where the gap rule allows
        gap = min(w[a - 1] - w[a] if a > 0 else np.inf, w[a] - w[a + 1] if a + 1 < len(w) else np.inf)
        if coords and gap >= GAP * l1:
            want = v[:, a] * np.sqrt(w[a])
            if want @ x[:, a] < 0:
                want = -want
            err = np.abs(x[:, a] - want).max()
            compared.append(a)
            if err > COORD_TOL * np.sqrt(l1) + rel * np.abs(want).max():
                bad.append("axis %d: coordinates off by %.3g sqrt(l_1)" % (a + 1, err / np.sqrt(l1)))
        # the sign rule: the component largest in size is positive (a near-tie may go either way: only a clear winner is held to it)
        big = np.abs(x[:, a])
        at = int(np.argmax(big))
        if x[at, a] < 0 and np.all(np.delete(big, at) < big[at] * (1 - 1e-6)):
            bad.append("axis %d: the largest component is negative" % (a + 1))
    return bad, compared


def points(P, F=20):
    """the fixed-point Euclidean distances of the rows of P: q = floor(d 2^F + 1/2)"""
    P = np.asarray(P, dtype=np.float64)
    D = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    q = np.floor(np.ldexp(D, F) + 0.5).astype(np.int64)
    np.fill_diagonal(q, 0)
    return q


def jaccard(P, F=20):
    """q of the Jaccard distances of the rows of a 0/1 matrix, the library's rounding: floor((2^21 (u - s) + u) / (2 u))"""
    P = np.asarray(P, dtype=np.int64)
    s = P @ P.T
    n = np.diag(s)
    u = n[:, None] + n[None, :] - s
    assert F == 20
    q = np.where(u == 0, 0, ((1 << 21) * (u - s) + u) // np.maximum(2 * u, 1))
    np.fill_diagonal(q, 0)
    return q
