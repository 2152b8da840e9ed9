"""ctypes bindings of the C ABI in include/pangene_amd.h (the pangene.h-compatible surface).

Nothing here computes: every call goes into libpangene_amd.so (HIP backend).  (The checker build of the same host
driver -- linked against the plain-C oracle -- is loaded by tests/oracle_host.py, which hands its own path to load();
nothing in this package knows where it is.)
"""
from __future__ import annotations

import ctypes as C
import os
import shlex
import tempfile
from typing import List, Sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_HIP = os.path.join(ROOT, "pangene_amd", "lib", "libpangene_amd.so")

PG_F_WRITE_BED_RAW, PG_F_WRITE_BED_WALK, PG_F_WRITE_BED_FLAG, PG_F_WRITE_NO_WALK = 0x1, 0x2, 0x4, 0x8
PG_F_WRITE_VTX_SEL, PG_F_FRAG_MODE, PG_F_NO_JOINT_PSEUDO, PG_F_ORI_FOR_BRANCH = 0x10, 0x20, 0x40, 0x80
PG_F_CHECK_STRAND, PG_F_DROP_SGL_EXON = 0x100, 0x200


class pg_opt_t(C.Structure):  # layout of pangene.h:23-42 (128 bytes)
    _fields_ = [("flag", C.c_uint32), ("gene_delim", C.c_int32), ("min_prot_ratio", C.c_double), ("min_prot_iden", C.c_double),
                ("score_adj_coef", C.c_double), ("min_ov_ratio", C.c_double), ("min_vertex_ratio", C.c_double),
                ("branch_diff", C.c_double), ("branch_diff_dist", C.c_double), ("branch_diff_cut", C.c_double),
                ("max_avg_occ", C.c_int32), ("max_degree", C.c_int32), ("max_dist_loci", C.c_int32), ("n_branch_flt", C.c_int32),
                ("min_arc_cnt", C.c_int32), ("local_dist", C.c_int32), ("local_count", C.c_int32),
                ("excl", C.c_void_p), ("incl", C.c_void_p), ("preferred", C.c_void_p)]


ALLREDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32)
ALLGATHER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32)


class pg_exchange_t(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("user", C.c_void_p), ("allreduce", ALLREDUCE_CB), ("allgather", ALLGATHER_CB), ("stream_ordered", C.c_int32)]


class pg_call_opt_t(C.Structure):
    """pangene.js call options (include/pangene_amd.h)."""
    _fields_ = [("max_ext", C.c_int32), ("ignore_walk", C.c_int32), ("use_pst", C.c_int32), ("add_super", C.c_int32),
                ("print_bandage", C.c_int32), ("print_cec", C.c_int32), ("print_dfs", C.c_int32), ("ref", C.c_char_p)]


def call_opt(lib: C.CDLL, argv: Sequence[str] = ()) -> pg_call_opt_t:
    """The option letters of `pangene.js call` (-m INT -w -b -e -d -p -s -r STR)."""
    o = pg_call_opt_t()
    lib.pg_call_opt_init(C.byref(o))
    it = iter(argv)
    for a in it:
        if a == "-m": o.max_ext = int(next(it))
        elif a == "-r": o.ref = next(it).encode()
        else:
            for ch in a[1:]:
                setattr(o, {"w": "ignore_walk", "p": "use_pst", "s": "add_super", "b": "print_bandage", "e": "print_cec", "d": "print_dfs"}[ch], 1)
    return o


class pg_curves_opt_t(C.Structure):
    """Accumulation-curve options (include/pangene_amd.h): orders (the input order first) and their seed."""
    _fields_ = [("n_perm", C.c_int32), ("seed", C.c_uint32)]


CURVE_STATS = ("pan", "core", "new", "unique")


def curves_opt(lib: C.CDLL, n_perm: int | None = None, seed: int | None = None) -> pg_curves_opt_t:
    o = pg_curves_opt_t()
    lib.pg_curves_opt_init(C.byref(o))
    if n_perm is not None: o.n_perm = n_perm
    if seed is not None: o.seed = seed
    return o


def pan_curves(lib: C.CDLL, presence, n_perm: int = 10, seed: int = 11):
    """Accumulation curves of a gene x assembly presence matrix (bool numpy array or torch tensor, shape (G, A)) through
    pg_pan_curves: an int32 array (4, n_perm, A) of pan, core, new and unique genes after k = 1 .. A assemblies, per order."""
    import numpy as np
    if hasattr(presence, "detach"):  # torch tensor, on any device
        presence = presence.detach().cpu().numpy()
    p = np.ascontiguousarray(np.asarray(presence) != 0, dtype=np.uint8)
    if p.ndim != 2:
        raise ValueError("presence must be 2-D (genes x assemblies)")
    G, A = p.shape
    out = np.zeros((4, n_perm, A), dtype=np.int32)
    o = curves_opt(lib, n_perm, seed)
    rc = lib.pg_pan_curves(p.ctypes.data_as(C.POINTER(C.c_uint8)), G, A, C.byref(o), out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise RuntimeError("pg_pan_curves: status %d" % rc)
    return out


def _curves_args(argv: Sequence[str]):
    """(orders, seed) of --curves[=INT] / --curves-seed=INT in argv; orders = 0 without --curves."""
    n, seed = 0, 11
    for a in argv:
        if a == "--curves": n = 10
        elif a.startswith("--curves="): n = int(a.split("=", 1)[1])
        elif a.startswith("--curves-seed="): seed = int(a.split("=", 1)[1])
    return n, seed


class pg_dist_opt_t(C.Structure):
    """Distance options (include/pangene_amd.h): items (PG_DIST_GENE / PG_DIST_ADJ), metric, PHYLIP layout."""
    _fields_ = [("type", C.c_int32), ("metric", C.c_int32), ("phylip", C.c_int32)]


DIST_TYPES = ("gene", "adj")
DIST_METRICS = ("jaccard", "shared", "diff")


def dist_opt(lib: C.CDLL, type: str = "gene", metric: str = "jaccard", phylip: bool = False) -> pg_dist_opt_t:
    o = pg_dist_opt_t()
    lib.pg_dist_opt_init(C.byref(o))
    o.type, o.metric, o.phylip = DIST_TYPES.index(type), DIST_METRICS.index(metric), int(bool(phylip))
    return o


def _presence(presence):
    """(items, assemblies) numpy array or torch tensor -> contiguous uint8 0/1"""
    import numpy as np
    if hasattr(presence, "detach"):  # torch tensor, on any device
        presence = presence.detach().cpu().numpy()
    p = np.ascontiguousarray(np.asarray(presence) != 0, dtype=np.uint8)
    if p.ndim != 2:
        raise ValueError("presence must be 2-D (items x assemblies)")
    return p


def pan_shared(lib: C.CDLL, presence):
    """Items shared by every pair of assemblies of an item x assembly presence matrix (bool numpy array or torch tensor, shape (M, A))
    through pg_pan_shared: an int32 array (A, A), the diagonal = the items of each assembly."""
    import numpy as np
    p = _presence(presence)
    M, A = p.shape
    out = np.zeros((A, A), dtype=np.int32)
    rc = lib.pg_pan_shared(p.ctypes.data_as(C.POINTER(C.c_uint8)), M, A, out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise RuntimeError("pg_pan_shared: status %d" % rc)
    return out


def pan_dist(lib: C.CDLL, presence, metric: str = "jaccard"):
    """Pairwise distances of the assemblies of a presence matrix through pg_pan_dist: (A, A), float64 for jaccard, int64 for shared
    and diff."""
    import numpy as np
    p = _presence(presence)
    M, A = p.shape
    out = np.zeros((A, A), dtype=np.float64)
    rc = lib.pg_pan_dist(p.ctypes.data_as(C.POINTER(C.c_uint8)), M, A, DIST_METRICS.index(metric), out.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != 0:
        raise RuntimeError("pg_pan_dist: status %d" % rc)
    return out if metric == "jaccard" else out.astype(np.int64)


def _dist_args(argv: Sequence[str]):
    """(type, metric) of --dist[=gene|adj] / --dist-metric=STR in argv; type = None without --dist."""
    t, m = None, "jaccard"
    for a in argv:
        if a == "--dist": t = "gene"
        elif a.startswith("--dist="): t = a.split("=", 1)[1]
        elif a.startswith("--dist-metric="): m = a.split("=", 1)[1]
    if t is not None and t not in DIST_TYPES:
        raise ValueError("--dist must be gene or adj")
    if m not in DIST_METRICS:
        raise ValueError("--dist-metric must be jaccard, shared or diff")
    return t, m


class pg_assoc_opt_t(C.Structure):
    """Association options (include/pangene_amd.h): smallest |phi|, smallest min(a, A - a) of a gene, sign (PG_ASSOC_*), pair limit."""
    _fields_ = [("min_phi", C.c_double), ("min_count", C.c_int32), ("sign", C.c_int32), ("max_pair", C.c_int64)]


ASSOC_SIGNS = ("both", "pos", "neg")
ASSOC_MAX_PAIR = 16777216


def assoc_opt(lib: C.CDLL, min_phi: float = 0.8, min_count: int = 2, sign: str = "both", max_pair: int = ASSOC_MAX_PAIR) -> pg_assoc_opt_t:
    if not 0.0 <= float(min_phi) <= 1.0:
        raise ValueError("min_phi must be in [0, 1]")
    if int(min_count) < 1:
        raise ValueError("min_count must be at least 1")
    if sign not in ASSOC_SIGNS:
        raise ValueError("sign must be pos, neg or both")
    o = pg_assoc_opt_t()
    lib.pg_assoc_opt_init(C.byref(o))
    o.min_phi, o.min_count, o.sign, o.max_pair = float(min_phi), int(min_count), ASSOC_SIGNS.index(sign), int(max_pair)
    return o


def pan_assoc(lib: C.CDLL, presence, min_phi: float = 0.8, min_count: int = 2, sign: str = "both", max_pair: int = ASSOC_MAX_PAIR):
    """Associated gene pairs of a gene x assembly presence matrix (bool numpy array or torch tensor, shape (G, A)) through pg_pan_assoc:
    (pairs, phi) with pairs an int32 array (n, 3) of (g, h, |B_g & B_h|), g < h, ascending, and phi a float64 array (n,)."""
    import numpy as np
    p = _presence(presence)
    G, A = p.shape
    o = assoc_opt(lib, min_phi, min_count, sign, max_pair)
    cap = 65536
    while True:  # the call says how many pairs there are; a second one fetches them when the first buffer was too small
        pairs = np.zeros((cap, 3), dtype=np.int32)
        n = lib.pg_pan_assoc(p.ctypes.data_as(C.POINTER(C.c_uint8)), G, A, C.byref(o), pairs.ctypes.data_as(C.POINTER(C.c_int32)), cap)
        if n < 0:
            raise RuntimeError("pg_pan_assoc: status %d" % n)
        if n <= cap:
            break
        cap = n
    pairs = pairs[:n].copy()
    cnt = p.sum(axis=1, dtype=np.int64)
    a, b, s = cnt[pairs[:, 0]], cnt[pairs[:, 1]], pairs[:, 2].astype(np.int64)
    D, Vg, Vh = s * A - a * b, a * (A - a), b * (A - b)
    phi = D.astype(np.float64) / np.sqrt(Vg.astype(np.float64) * Vh.astype(np.float64))
    return pairs, phi


def _assoc_args(argv: Sequence[str]):
    """(min_phi, min_count, sign) of --assoc[=FLOAT] / --assoc-min-count=INT / --assoc-sign=STR in argv; min_phi = None without --assoc."""
    r, c, s = None, 2, "both"
    for a in argv:
        if a == "--assoc": r = 0.8
        elif a.startswith("--assoc="): r = float(a.split("=", 1)[1])
        elif a.startswith("--assoc-min-count="): c = int(a.split("=", 1)[1])
        elif a.startswith("--assoc-sign="): s = a.split("=", 1)[1]
    if r is not None and not 0.0 <= r <= 1.0:
        raise ValueError("--assoc must be in [0, 1]")
    if c < 1:
        raise ValueError("--assoc-min-count must be at least 1")
    if s not in ASSOC_SIGNS:
        raise ValueError("--assoc-sign must be pos, neg or both")
    return r, c, s


class pg_trait_opt_t(C.Structure):
    """Trait options (include/pangene_amd.h): permutations, their seed, smallest min(a, N - a) of a tested gene, p_fisher cutoff of the lines,
    the tree of the lineage-aware pairwise comparisons (0 none, 1 nj, 2 upgma)."""
    _fields_ = [("n_perm", C.c_int32), ("seed", C.c_uint32), ("min_count", C.c_int32), ("reserved", C.c_int32), ("max_p", C.c_double),
                ("lineage", C.c_int32)]


TRAIT_MAX_PERM = 2147483646
TRAIT_LINEAGES = (None, "nj", "upgma")


def trait_opt(lib: C.CDLL, n_perm: int = 1000, seed: int = 11, min_count: int = 1, max_p: float = 1.0, lineage=None) -> pg_trait_opt_t:
    if not 0 <= int(n_perm) <= TRAIT_MAX_PERM:
        raise ValueError("n_perm must be in [0, 2^31 - 2]")
    if int(min_count) < 1:
        raise ValueError("min_count must be at least 1")
    if lineage not in TRAIT_LINEAGES:
        raise ValueError("lineage must be nj, upgma or None")
    o = pg_trait_opt_t()
    lib.pg_trait_opt_init(C.byref(o))
    o.n_perm, o.seed, o.min_count, o.max_p = int(n_perm), int(seed) & 0xFFFFFFFF, int(min_count), float(max_p)
    o.lineage = TRAIT_LINEAGES.index(lineage)
    return o


def pan_trait(lib: C.CDLL, presence, labels, n_perm: int = 1000, seed: int = 11, min_count: int = 1):
    """Gene-trait association of a gene x assembly presence matrix (bool numpy array or torch tensor, shape (G, A)) with binary traits
    (labels: shape (T, A) or (A,), 1 / 0 and a negative value = missing) through pg_pan_trait: a dict of int32 arrays (T, G): N and t
    (columns with a value and the 1s among them), a, s (|B_g|, |B_g & y|; a = -1 for a gene that is not tested) and k (the
    permutations of the labels with |D_p| >= |D|)."""
    import numpy as np
    p = _presence(presence)
    if hasattr(labels, "detach"):  # torch tensor, on any device
        labels = labels.detach().cpu().numpy()
    y = np.asarray(labels)
    if y.ndim == 1:
        y = y[None, :]
    G, A = p.shape
    if y.ndim != 2 or y.shape[1] != A:
        raise ValueError("labels must be (traits x assemblies) over the assemblies of presence")
    y = np.ascontiguousarray(np.where(y < 0, -1, np.where(y != 0, 1, 0)), dtype=np.int8)
    T = y.shape[0]
    o = trait_opt(lib, n_perm, seed, min_count)
    out = np.zeros((5, T, G), dtype=np.int32)
    rc = lib.pg_pan_trait(p.ctypes.data_as(C.POINTER(C.c_uint8)), y.ctypes.data_as(C.POINTER(C.c_int8)), G, A, T, C.byref(o), out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise RuntimeError("pg_pan_trait: status %d" % rc)
    return {"N": out[0], "t": out[1], "a": out[2], "s": out[3], "k": out[4]}


def pan_pairs(lib: C.CDLL, presence, labels, rec, method: str = "nj"):
    """The lineage-aware pairwise comparisons of a gene x assembly presence matrix (shape (G, A)) with binary traits (labels as for
    pan_trait) on the tree of the records rec (an int64 array as pan_tree or pan_join return it for `method`; any such tree over the A
    assemblies, ignored when A < 3) through pg_pan_pairs: a dict of int32 arrays (T, G): pairs (the size of a largest set of contrasting
    leaf pairs on vertex-disjoint paths), supp and opp (the most supporting and the most opposing pairs such a largest set can have)."""
    import numpy as np
    p = _presence(presence)
    if hasattr(labels, "detach"):  # torch tensor, on any device
        labels = labels.detach().cpu().numpy()
    y = np.asarray(labels)
    if y.ndim == 1:
        y = y[None, :]
    G, A = p.shape
    if y.ndim != 2 or y.shape[1] != A:
        raise ValueError("labels must be (traits x assemblies) over the assemblies of presence")
    y = np.ascontiguousarray(np.where(y < 0, -1, np.where(y != 0, 1, 0)), dtype=np.int8)
    T = y.shape[0]
    m = TREE_METHODS.index(method)
    rec = np.ascontiguousarray(rec if rec is not None else np.zeros((0, 6)), dtype=np.int64).reshape(-1, 6)
    if A >= 3 and rec.shape[0] != A - 2 + m:
        raise ValueError("rec must hold %d records for %d assemblies and %s" % (A - 2 + m, A, method))
    out = np.zeros((3, T, G), dtype=np.int32)
    rc = lib.pg_pan_pairs(p.ctypes.data_as(C.POINTER(C.c_uint8)), y.ctypes.data_as(C.POINTER(C.c_int8)), G, A, T, rec.ctypes.data_as(C.POINTER(C.c_int64)), m,
                          out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise RuntimeError("pg_pan_pairs: status %d" % rc)
    return {"pairs": out[0], "supp": out[1], "opp": out[2]}


class pg_qtrait_opt_t(C.Structure):
    """Quantitative-trait options (include/pangene_amd.h): permutations, their seed, smallest min(a, N - a) of a tested gene, p_wilcox cutoff
    of the lines."""
    _fields_ = [("n_perm", C.c_int32), ("seed", C.c_uint32), ("min_count", C.c_int32), ("reserved", C.c_int32), ("max_p", C.c_double)]


def qtrait_opt(lib: C.CDLL, n_perm: int = 1000, seed: int = 11, min_count: int = 1, max_p: float = 1.0) -> pg_qtrait_opt_t:
    if not 0 <= int(n_perm) <= TRAIT_MAX_PERM:
        raise ValueError("n_perm must be in [0, 2^31 - 2]")
    if int(min_count) < 1:
        raise ValueError("min_count must be at least 1")
    o = pg_qtrait_opt_t()
    lib.pg_qtrait_opt_init(C.byref(o))
    o.n_perm, o.seed, o.min_count, o.max_p = int(n_perm), int(seed) & 0xFFFFFFFF, int(min_count), float(max_p)
    return o


def pan_qtrait(lib: C.CDLL, presence, values, n_perm: int = 1000, seed: int = 11, min_count: int = 1):
    """Rank-sum association of a gene x assembly presence matrix (bool numpy array or torch tensor, shape (G, A)) with quantitative
    traits (values: shape (T, A) or (A,), floating point, NaN = missing) through pg_pan_qtrait: a dict of int32 arrays (T, G): N (columns
    with a value), a (|B_g|; -1 for a gene that is not tested), D (the sum of the centred doubled midranks over the gene's columns) and
    k (the permutations of the values with |D_p| >= |D|)."""
    import numpy as np
    p = _presence(presence)
    if hasattr(values, "detach"):  # torch tensor, on any device
        values = values.detach().cpu().numpy()
    v = np.asarray(values, dtype=np.float64)
    if v.ndim == 1:
        v = v[None, :]
    G, A = p.shape
    if v.ndim != 2 or v.shape[1] != A:
        raise ValueError("values must be (traits x assemblies) over the assemblies of presence")
    if np.isinf(v).any():
        raise ValueError("values must be finite or NaN (missing)")
    v = np.ascontiguousarray(v)
    T = v.shape[0]
    o = qtrait_opt(lib, n_perm, seed, min_count)
    out = np.zeros((4, T, G), dtype=np.int32)
    rc = lib.pg_pan_qtrait(p.ctypes.data_as(C.POINTER(C.c_uint8)), v.ctypes.data_as(C.POINTER(C.c_double)), G, A, T, C.byref(o), out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise RuntimeError("pg_pan_qtrait: status %d" % rc)
    return {"N": out[0], "a": out[1], "D": out[2], "k": out[3]}


def _qtrait_args(argv: Sequence[str]):
    """(file, permutations, seed) of --qtrait=FILE / --qtrait-perm=INT / --qtrait-seed=INT in argv; file = None without --qtrait."""
    f, n, seed, extra = None, 1000, 11, False
    for a in argv:
        if a.startswith("--qtrait="): f = a.split("=", 1)[1]
        elif a.startswith("--qtrait-perm="): n, extra = int(a.split("=", 1)[1]), True
        elif a.startswith("--qtrait-seed="): seed, extra = int(a.split("=", 1)[1]), True
    if not 0 <= n <= TRAIT_MAX_PERM:
        raise ValueError("--qtrait-perm must be in [0, 2^31 - 2]")
    if extra and f is None:
        raise ValueError("--qtrait-perm and --qtrait-seed need --qtrait=FILE")
    return f, n, seed


def _trait_args(argv: Sequence[str]):
    """(file, permutations, seed, lineage) of --trait=FILE / --trait-perm=INT / --trait-seed=INT / --trait-lineage=nj|upgma in argv;
    file = None without --trait."""
    f, n, seed, lineage = None, 1000, 11, None
    for a in argv:
        if a.startswith("--trait="): f = a.split("=", 1)[1]
        elif a.startswith("--trait-perm="): n = int(a.split("=", 1)[1])
        elif a.startswith("--trait-seed="): seed = int(a.split("=", 1)[1])
        elif a.startswith("--trait-lineage="): lineage = a.split("=", 1)[1]
    if not 0 <= n <= TRAIT_MAX_PERM:
        raise ValueError("--trait-perm must be in [0, 2^31 - 2]")
    if lineage is not None and (lineage not in TRAIT_LINEAGES or f is None):
        raise ValueError("--trait-lineage must be nj or upgma and needs --trait=FILE")
    return f, n, seed, lineage


class pg_tree_opt_t(C.Structure):
    """Tree options (include/pangene_amd.h): items (PG_DIST_GENE / PG_DIST_ADJ), distance (jaccard or diff), joining method, bootstrap
    replicates and the seed of their draws."""
    _fields_ = [("type", C.c_int32), ("metric", C.c_int32), ("method", C.c_int32), ("n_boot", C.c_int32), ("seed", C.c_uint32)]


TREE_METRICS = ("jaccard", "diff")
TREE_METHODS = ("nj", "upgma")


TREE_MAX_BOOT = 2147483647


def tree_opt(lib: C.CDLL, type: str = "gene", metric: str = "jaccard", method: str = "nj", n_boot: int = 0, seed: int = 0) -> pg_tree_opt_t:
    if metric not in TREE_METRICS:
        raise ValueError("metric must be jaccard or diff (shared is not a distance)")
    if not 0 <= int(n_boot) <= TREE_MAX_BOOT:
        raise ValueError("n_boot must be in [0, 2^31 - 1]")
    o = pg_tree_opt_t()
    lib.pg_tree_opt_init(C.byref(o))
    o.type, o.metric, o.method = DIST_TYPES.index(type), DIST_METRICS.index(metric), TREE_METHODS.index(method)
    o.n_boot, o.seed = int(n_boot), int(seed) & 0xFFFFFFFF
    return o


def pan_join(lib: C.CDLL, q, method: str = "nj"):
    """The joins of a fixed-point distance matrix (int32 numpy array or torch tensor, shape (n, n), symmetric, zero diagonal, n >= 3)
    through pg_pan_join: an int64 array of records, (n - 2, 6) for nj -- (i, j, d_ij, R_i, R_j, r), the last one
    (x, y, z, d_xy, d_xz, d_yz) -- and (n - 1, 6) for upgma -- (i, j, d_ij, n_i, n_j, r)."""
    import numpy as np
    if hasattr(q, "detach"):  # torch tensor, on any device
        q = q.detach().cpu().numpy()
    q = np.ascontiguousarray(q, dtype=np.int32)
    if q.ndim != 2 or q.shape[0] != q.shape[1]:
        raise ValueError("q must be a square matrix")
    n = q.shape[0]
    m = TREE_METHODS.index(method)
    rec = np.zeros((max(n - 2 + m, 0), 6), dtype=np.int64)
    rc = lib.pg_pan_join(q.ctypes.data_as(C.POINTER(C.c_int32)), n, m, rec.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != 0:
        raise RuntimeError("pg_pan_join: status %d" % rc)
    return rec


def pan_tree(lib: C.CDLL, presence, metric: str = "jaccard", method: str = "nj"):
    """The joins of the assemblies of an item x assembly presence matrix (bool numpy array or torch tensor, shape (M, A), A >= 3)
    through pg_pan_tree: (records as pan_join returns them, F) with distances and row sums in units of 2^-F."""
    import numpy as np
    if metric not in TREE_METRICS:
        raise ValueError("metric must be jaccard or diff (shared is not a distance)")
    p = _presence(presence)
    M, A = p.shape
    m = TREE_METHODS.index(method)
    rec = np.zeros((max(A - 2 + m, 0), 6), dtype=np.int64)
    F = C.c_int32(0)
    rc = lib.pg_pan_tree(p.ctypes.data_as(C.POINTER(C.c_uint8)), M, A, DIST_METRICS.index(metric), m, rec.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(F))
    if rc != 0:
        raise RuntimeError("pg_pan_tree: status %d" % rc)
    return rec, int(F.value)


def pan_boot(lib: C.CDLL, presence, metric: str = "jaccard", method: str = "nj", n_boot: int = 100, seed: int = 0):
    """Bootstrap support of the tree of an item x assembly presence matrix (bool numpy array or torch tensor, shape (M, A), A >= 3)
    through pg_pan_boot: (records, F, count) with the records and F as pan_tree returns them and count an int32 array, one entry per
    record: the replicates, of n_boot, that have the node of that join (nj: the same split of the leaves); n_boot itself for nj's
    closing record and upgma's root."""
    import numpy as np
    if metric not in TREE_METRICS:
        raise ValueError("metric must be jaccard or diff (shared is not a distance)")
    p = _presence(presence)
    M, A = p.shape
    m = TREE_METHODS.index(method)
    rec = np.zeros((max(A - 2 + m, 0), 6), dtype=np.int64)
    count = np.zeros(max(A - 2 + m, 0), dtype=np.int32)
    F = C.c_int32(0)
    rc = lib.pg_pan_boot(p.ctypes.data_as(C.POINTER(C.c_uint8)), M, A, DIST_METRICS.index(metric), m, int(n_boot), int(seed) & 0xFFFFFFFF,
                         rec.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(F), count.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise RuntimeError("pg_pan_boot: status %d" % rc)
    return rec, int(F.value), count


def pan_boot_records(lib: C.CDLL, presence, metric: str = "jaccard", method: str = "nj", seed: int = 0, first: int = 1, n: int = 1):
    """The records of bootstrap replicates first .. first + n - 1 (first >= 1) of a presence matrix as pan_boot takes it, through
    pg_pan_boot_records: an int64 array (n, records, 6), each replicate's records as pan_join returns them."""
    import numpy as np
    if metric not in TREE_METRICS:
        raise ValueError("metric must be jaccard or diff (shared is not a distance)")
    p = _presence(presence)
    M, A = p.shape
    m = TREE_METHODS.index(method)
    rec = np.zeros((max(int(n), 0), max(A - 2 + m, 0), 6), dtype=np.int64)
    rc = lib.pg_pan_boot_records(p.ctypes.data_as(C.POINTER(C.c_uint8)), M, A, DIST_METRICS.index(metric), m, int(seed) & 0xFFFFFFFF, int(first), int(n),
                                 rec.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != 0:
        raise RuntimeError("pg_pan_boot_records: status %d" % rc)
    return rec


class pg_cluster_opt_t(C.Structure):
    """Cluster options (include/pangene_amd.h): items (PG_DIST_GENE / PG_DIST_ADJ), distance (jaccard or diff), the range of k and the
    swap iterations per k at the most."""
    _fields_ = [("type", C.c_int32), ("metric", C.c_int32), ("k_lo", C.c_int32), ("k_hi", C.c_int32), ("max_iter", C.c_int32)]


def cluster_opt(lib: C.CDLL, k_lo: int = 2, k_hi: int | None = None, type: str = "gene", metric: str = "jaccard", max_iter: int = 1000) -> pg_cluster_opt_t:
    if metric not in TREE_METRICS:
        raise ValueError("metric must be jaccard or diff (shared is not a distance)")
    k_hi = k_lo if k_hi is None else k_hi
    if not 2 <= int(k_lo) <= int(k_hi) <= TREE_MAX_BOOT:
        raise ValueError("k must be INT or INT-INT with 2 <= INT")
    if not 0 <= int(max_iter) <= TREE_MAX_BOOT:
        raise ValueError("max_iter must be in [0, 2^31 - 1]")
    o = pg_cluster_opt_t()
    lib.pg_cluster_opt_init(C.byref(o))
    o.type, o.metric, o.k_lo, o.k_hi, o.max_iter = DIST_TYPES.index(type), DIST_METRICS.index(metric), int(k_lo), int(k_hi), int(max_iter)
    return o


def _medoids_call(n, k, call):
    """The out arrays of pg_pan_medoids / pg_pan_cluster and the dict both return; call(pointers...) -> status.  The records are asked
    for again with more room when a run swapped more often than the first call had room for."""
    import numpy as np
    medoid, label, dist, size = (np.zeros(m, dtype=np.int32) for m in (k, n, n, k))
    sums = np.zeros((n, k), dtype=np.int64)
    n_rec, n_swap, conv, td = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
    cap = k + 256
    while True:
        rec = np.zeros((cap, 3), dtype=np.int64)
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        rc = call(i32(medoid), i32(label), i32(dist), i32(size), i64(sums), i64(rec), cap, C.byref(n_rec), C.byref(n_swap), C.byref(td), C.byref(conv))
        if rc != 0:
            return rc, None
        if n_rec.value <= cap:
            break
        cap = n_rec.value
    return 0, {"medoid": medoid, "label": label, "dist": dist, "size": size, "sums": sums, "rec": rec[:n_rec.value].copy(), "td": int(td.value),
               "n_swap": int(n_swap.value), "converged": int(conv.value)}


def pan_medoids(lib: C.CDLL, q, k: int, max_iter: int = 1000):
    """k-medoids over a fixed-point distance matrix (int32 numpy array or torch tensor, shape (n, n), symmetric, zero diagonal, entries in
    [0, 2^29), n >= 3, 2 <= k <= min(n - 1, 1024)) through pg_pan_medoids: a dict with medoid (k,), label (n,), dist (n,), size (k,) int32,
    sums (n, k) int64, rec (k + n_swap, 3) int64 -- BUILD's (x, -1, gain), then the swaps' (x, m, delta) --, td, n_swap and converged."""
    import numpy as np
    if hasattr(q, "detach"):  # torch tensor, on any device
        q = q.detach().cpu().numpy()
    q = np.ascontiguousarray(q, dtype=np.int32)
    if q.ndim != 2 or q.shape[0] != q.shape[1]:
        raise ValueError("q must be a square matrix")
    n, k = q.shape[0], int(k)
    rc, res = _medoids_call(n, max(k, 1), lambda *a: lib.pg_pan_medoids(q.ctypes.data_as(C.POINTER(C.c_int32)), n, k, int(max_iter), *a))
    if rc != 0:
        raise RuntimeError("pg_pan_medoids: status %d" % rc)
    return res


def pan_cluster(lib: C.CDLL, presence, k: int, metric: str = "jaccard", max_iter: int = 1000):
    """k-medoids clusters of the assemblies of an item x assembly presence matrix (bool numpy array or torch tensor, shape (M, A), A >= 3)
    through pg_pan_cluster: (the dict pan_medoids returns, F) with distances in units of 2^-F."""
    if metric not in TREE_METRICS:
        raise ValueError("metric must be jaccard or diff (shared is not a distance)")
    p = _presence(presence)
    M, A = p.shape
    F = C.c_int32(0)
    k = int(k)
    rc, res = _medoids_call(A, max(k, 1), lambda *a: lib.pg_pan_cluster(p.ctypes.data_as(C.POINTER(C.c_uint8)), M, A, DIST_METRICS.index(metric), k, int(max_iter), *a, C.byref(F)))
    if rc != 0:
        raise RuntimeError("pg_pan_cluster: status %d" % rc)
    return res, int(F.value)


class pg_permanova_opt_t(C.Structure):
    """PERMANOVA options (include/pangene_amd.h): items, distance, permutations, their seed, and the fraction bits of a matrix handed to
    pg_pan_permanova."""
    _fields_ = [("type", C.c_int32), ("metric", C.c_int32), ("n_perm", C.c_int32), ("seed", C.c_uint32), ("frac_bits", C.c_int32)]


def permanova_opt(lib: C.CDLL, type: str = "gene", metric: str = "jaccard", n_perm: int = 1000, seed: int = 11, frac_bits: int = 20) -> pg_permanova_opt_t:
    if type not in DIST_TYPES:
        raise ValueError("type must be gene or adj")
    if metric not in TREE_METRICS:
        raise ValueError("metric must be jaccard or diff (shared is not a distance)")
    if not 0 <= int(n_perm) <= TRAIT_MAX_PERM:
        raise ValueError("n_perm must be in [0, 2^31 - 2]")
    o = pg_permanova_opt_t()
    lib.pg_permanova_opt_init(C.byref(o))
    o.type, o.metric, o.n_perm, o.seed, o.frac_bits = DIST_TYPES.index(type), DIST_METRICS.index(metric), int(n_perm), int(seed) & 0xFFFFFFFF, int(frac_bits)
    return o


def _permanova_labels(labels, A):
    import numpy as np
    if hasattr(labels, "detach"):  # torch tensor, on any device
        labels = labels.detach().cpu().numpy()
    y = np.asarray(labels)
    if y.ndim == 1:
        y = y[None, :]
    if y.ndim != 2 or y.shape[1] != A:
        raise ValueError("labels must be (traits x assemblies) over the assemblies of the matrix")
    return np.ascontiguousarray(y, dtype=np.int8)


def _permanova_dict(out):
    return {"N": out[:, 0].copy(), "n1": out[:, 1].copy(), "Fe": out[:, 2].copy(), "T": out[:, 3].copy(), "A": out[:, 4].copy(), "B": out[:, 5].copy(), "k": out[:, 6].copy()}


def pan_permanova(lib: C.CDLL, q, labels, n_perm: int = 1000, seed: int = 11, frac_bits: int = 20):
    """Two-group PERMANOVA of a fixed-point distance matrix (int32 numpy array or torch tensor, shape (n, n), symmetric, zero diagonal,
    entries in [0, 2^29), frac_bits fraction bits) for binary labels (shape (T, n) or (n,): 1, 0, -1 = missing) through pg_pan_permanova: a
    dict of int64 arrays (T,): N, n1, Fe, T, A, B and k (-1 for a trait that is not tested: N < 3, an empty group, or no distance above
    zero)."""
    import numpy as np
    if hasattr(q, "detach"):
        q = q.detach().cpu().numpy()
    q = np.ascontiguousarray(q, dtype=np.int32)
    if q.ndim != 2 or q.shape[0] != q.shape[1]:
        raise ValueError("q must be a square matrix")
    n = q.shape[0]
    y = _permanova_labels(labels, n)
    T = y.shape[0]
    o = permanova_opt(lib, n_perm=n_perm, seed=seed, frac_bits=frac_bits)
    out = np.zeros((T, 7), dtype=np.int64)
    rc = lib.pg_pan_permanova(q.ctypes.data_as(C.POINTER(C.c_int32)), n, y.ctypes.data_as(C.POINTER(C.c_int8)), T, C.byref(o), out.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != 0:
        raise RuntimeError("pg_pan_permanova: status %d" % rc)
    return _permanova_dict(out)


def pan_permanova_presence(lib: C.CDLL, presence, labels, metric: str = "jaccard", n_perm: int = 1000, seed: int = 11):
    """The same for an item x assembly presence matrix (bool numpy array or torch tensor, shape (M, A)) through pg_pan_permanova_presence:
    (the dict pan_permanova returns, F) with the distances of `metric` in units of 2^-F."""
    import numpy as np
    p = _presence(presence)
    M, A = p.shape
    y = _permanova_labels(labels, A)
    T = y.shape[0]
    o = permanova_opt(lib, metric=metric, n_perm=n_perm, seed=seed)
    out = np.zeros((T, 7), dtype=np.int64)
    F = C.c_int32(0)
    rc = lib.pg_pan_permanova_presence(p.ctypes.data_as(C.POINTER(C.c_uint8)), M, A, y.ctypes.data_as(C.POINTER(C.c_int8)), T, C.byref(o),
                                       out.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(F))
    if rc != 0:
        raise RuntimeError("pg_pan_permanova_presence: status %d" % rc)
    return _permanova_dict(out), int(F.value)


def _permanova_args(argv: Sequence[str]):
    """(file, type, metric, permutations, seed) of --permanova=FILE / --permanova-type=STR / --permanova-metric=STR / --permanova-perm=INT /
    --permanova-seed=INT in argv; file = None without --permanova."""
    f, t, m, n, seed, extra = None, "gene", "jaccard", 1000, 11, False
    for x in argv:
        if x.startswith("--permanova="): f = x.split("=", 1)[1]
        elif x.startswith("--permanova-type="): t, extra = x.split("=", 1)[1], True
        elif x.startswith("--permanova-metric="): m, extra = x.split("=", 1)[1], True
        elif x.startswith("--permanova-perm="): n, extra = int(x.split("=", 1)[1]), True
        elif x.startswith("--permanova-seed="): seed, extra = int(x.split("=", 1)[1]), True
        elif x.startswith("--permanova"):
            raise ValueError("unknown option or missing value: " + x)
    if t not in DIST_TYPES:
        raise ValueError("--permanova-type must be gene or adj")
    if m not in TREE_METRICS:
        raise ValueError("--permanova-metric must be jaccard or diff")
    if not 0 <= n <= TRAIT_MAX_PERM:
        raise ValueError("--permanova-perm must be in [0, 2^31 - 2]")
    if extra and f is None:
        raise ValueError("--permanova-type, --permanova-metric, --permanova-perm and --permanova-seed need --permanova=FILE")
    return f, t, m, n, seed


class pg_mantel_opt_t(C.Structure):
    """Mantel options (include/pangene_amd.h): the two matrices, the permutations and their seed."""
    _fields_ = [("x_type", C.c_int32), ("x_metric", C.c_int32), ("y_type", C.c_int32), ("y_metric", C.c_int32), ("n_perm", C.c_int32), ("seed", C.c_uint32)]


def _mantel_spec(spec: str, what: str):
    """(type index, metric index) of gene|adj:jaccard|diff"""
    t, colon, m = spec.partition(":")
    if not colon or t not in DIST_TYPES or m not in TREE_METRICS:
        raise ValueError(what + " must be gene|adj:jaccard|diff")
    return DIST_TYPES.index(t), DIST_METRICS.index(m)


def mantel_opt(lib: C.CDLL, x: str = "gene:jaccard", y: str = "adj:jaccard", n_perm: int = 1000, seed: int = 11) -> pg_mantel_opt_t:
    xt, xm = _mantel_spec(x, "x")
    yt, ym = _mantel_spec(y, "y")
    if not 0 <= int(n_perm) <= TRAIT_MAX_PERM:
        raise ValueError("n_perm must be in [0, 2^31 - 2]")
    o = pg_mantel_opt_t()
    lib.pg_mantel_opt_init(C.byref(o))
    o.x_type, o.x_metric, o.y_type, o.y_metric, o.n_perm, o.seed = xt, xm, yt, ym, int(n_perm), int(seed) & 0xFFFFFFFF
    return o


def pan_mantel(lib: C.CDLL, qx, qy, n_perm: int = 1000, seed: int = 11):
    """Mantel test of two fixed-point distance matrices over the same assemblies (int32 numpy arrays or torch tensors, shape (n, n),
    symmetric, zero diagonal, entries in [0, 2^29)) through pg_pan_mantel: a dict of Python ints N, sx, sy, Sa, Sb, Saa, Sbb, Z, n_ge and
    n_le (Z = 0 and n_ge = n_le = -1 for a pair that is not tested: N < 3 or a matrix with one value only)."""
    import numpy as np
    qs = []
    for q in (qx, qy):
        if hasattr(q, "detach"):  # torch tensor, on any device
            q = q.detach().cpu().numpy()
        q = np.ascontiguousarray(q, dtype=np.int32)
        if q.ndim != 2 or q.shape[0] != q.shape[1]:
            raise ValueError("qx and qy must be square matrices")
        qs.append(q)
    if qs[0].shape != qs[1].shape:
        raise ValueError("qx and qy must be over the same assemblies")
    o = mantel_opt(lib, n_perm=n_perm, seed=seed)
    out = np.zeros(10, dtype=np.int64)
    rc = lib.pg_pan_mantel(qs[0].ctypes.data_as(C.POINTER(C.c_int32)), qs[1].ctypes.data_as(C.POINTER(C.c_int32)), qs[0].shape[0], C.byref(o),
                           out.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != 0:
        raise RuntimeError("pg_pan_mantel: status %d" % rc)
    return dict(zip(("N", "sx", "sy", "Sa", "Sb", "Saa", "Sbb", "Z", "n_ge", "n_le"), (int(v) for v in out)))


def _mantel_args(argv: Sequence[str]):
    """(asked for, file, x, y, permutations, seed) of --mantel[=FILE] / --mantel-x=SPEC / --mantel-y=SPEC / --mantel-perm=INT /
    --mantel-seed=INT in argv."""
    on, f, x, y, n, seed, extra, have_y = False, None, "gene:jaccard", "adj:jaccard", 1000, 11, False, False
    for a in argv:
        if a == "--mantel": on = True
        elif a.startswith("--mantel="): on, f = True, a.split("=", 1)[1]
        elif a.startswith("--mantel-x="): x, extra = a.split("=", 1)[1], True
        elif a.startswith("--mantel-y="): y, extra, have_y = a.split("=", 1)[1], True, True
        elif a.startswith("--mantel-perm="): n, extra = int(a.split("=", 1)[1]), True
        elif a.startswith("--mantel-seed="): seed, extra = int(a.split("=", 1)[1]), True
        elif a.startswith("--mantel"):
            raise ValueError("unknown option or missing value: " + a)
    _mantel_spec(x, "--mantel-x")
    _mantel_spec(y, "--mantel-y")
    if not 0 <= n <= TRAIT_MAX_PERM:
        raise ValueError("--mantel-perm must be in [0, 2^31 - 2]")
    if extra and not on:
        raise ValueError("--mantel-x, --mantel-y, --mantel-perm and --mantel-seed need --mantel")
    if have_y and f is not None:
        raise ValueError("--mantel-y cannot be combined with --mantel=FILE")
    return on, f, x, y, n, seed


GAINLOSS_MODES = ("late", "early")
GAINLOSS_OUTS = ("gene", "node")


class pg_gainloss_opt_t(C.Structure):
    """Gain and loss options (include/pangene_amd.h): the items, the tree, the two costs, the tie rule, the table and its filter."""
    _fields_ = [("type", C.c_int32), ("metric", C.c_int32), ("method", C.c_int32), ("gain", C.c_int32), ("loss", C.c_int32), ("mode", C.c_int32),
                ("out", C.c_int32), ("min_changes", C.c_int32)]


def gainloss_opt(lib: C.CDLL, type: str = "gene", metric: str = "jaccard", method: str = "upgma", gain: int = 1, loss: int = 1, mode: str = "late",
                 out: str = "gene", min_changes: int = 0) -> pg_gainloss_opt_t:
    if type not in DIST_TYPES:
        raise ValueError("type must be gene or adj")
    if metric not in TREE_METRICS:
        raise ValueError("metric must be jaccard or diff")
    if method not in TREE_METHODS:
        raise ValueError("method must be upgma or nj")
    if not (1 <= int(gain) <= 255 and 1 <= int(loss) <= 255):
        raise ValueError("gain and loss must be in [1, 255]")
    if mode not in GAINLOSS_MODES:
        raise ValueError("mode must be late or early")
    if out not in GAINLOSS_OUTS:
        raise ValueError("out must be gene or node")
    if not 0 <= int(min_changes) <= TREE_MAX_BOOT:
        raise ValueError("min_changes must be in [0, 2^31 - 1]")
    o = pg_gainloss_opt_t()
    lib.pg_gainloss_opt_init(C.byref(o))
    o.type, o.metric, o.method = DIST_TYPES.index(type), DIST_METRICS.index(metric), TREE_METHODS.index(method)
    o.gain, o.loss, o.mode, o.out, o.min_changes = int(gain), int(loss), GAINLOSS_MODES.index(mode), GAINLOSS_OUTS.index(out), int(min_changes)
    return o


def pan_gainloss(lib: C.CDLL, presence, rec, method: str, gain: int = 1, loss: int = 1, mode: str = "late"):
    """Gains and losses of the items of an item x assembly presence matrix (bool numpy array or torch tensor, shape (M, A)) on the tree of
    the records rec (an int64 array as pan_tree or pan_join return it for `method`; any such tree over the A assemblies, ignored when
    A < 3) through pg_pan_gainloss: a dict of numpy arrays: present, cost, gains, losses and root, int32 (M,), per item; node_present,
    node_gains and node_losses, int64 (2 A - 1,), per node (leaf x = x, join s = A + s; 0 gains and losses at the root)."""
    import numpy as np
    p = _presence(presence)
    M, A = p.shape
    m = TREE_METHODS.index(method)
    rec = np.ascontiguousarray(rec if rec is not None else np.zeros((0, 6)), dtype=np.int64).reshape(-1, 6)
    if A >= 3 and rec.shape[0] != A - 2 + m:
        raise ValueError("rec must hold %d records for %d assemblies and %s" % (A - 2 + m, A, method))
    o = gainloss_opt(lib, method=method, gain=gain, loss=loss, mode=mode)
    gene = np.zeros((M, 5), dtype=np.int32)
    node = np.zeros((max(2 * A - 1, 0), 3), dtype=np.int64)
    rc = lib.pg_pan_gainloss(p.ctypes.data_as(C.POINTER(C.c_uint8)), M, A, rec.ctypes.data_as(C.POINTER(C.c_int64)), m, C.byref(o),
                             gene.ctypes.data_as(C.POINTER(C.c_int32)), node.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != 0:
        raise RuntimeError("pg_pan_gainloss: status %d" % rc)
    out = {k: np.ascontiguousarray(gene[:, i]) for i, k in enumerate(("present", "cost", "gains", "losses", "root"))}
    out.update({"node_" + k: np.ascontiguousarray(node[:, i]) for i, k in enumerate(("present", "gains", "losses"))})
    return out


def _gainloss_args(argv: Sequence[str]):
    """The options of --gainloss[=gene|node] / --gainloss-type= / --gainloss-metric= / --gainloss-method= / --gainloss-gain= /
    --gainloss-loss= / --gainloss-resolve= / --gainloss-min= in argv as keywords of gainloss_opt; None without --gainloss."""
    on, extra, kw = False, False, {}
    names = {"type": "type", "metric": "metric", "method": "method", "gain": "gain", "loss": "loss", "resolve": "mode", "min": "min_changes"}
    for a in argv:
        if a == "--gainloss": on = True
        elif a.startswith("--gainloss="): on, kw["out"] = True, a.split("=", 1)[1]
        elif a.startswith("--gainloss-") and "=" in a and a[11:].split("=", 1)[0] in names:
            k, v = a[11:].split("=", 1)
            kw[names[k]] = int(v) if k in ("gain", "loss", "min") else v
            extra = True
        elif a.startswith("--gainloss"):
            raise ValueError("unknown option or missing value: " + a)
    if extra and not on:
        raise ValueError("--gainloss-type, --gainloss-metric, --gainloss-method, --gainloss-gain, --gainloss-loss, --gainloss-resolve and --gainloss-min need --gainloss")
    return kw if on else None


class pg_coevo_opt_t(C.Structure):
    """Co-evolution options (include/pangene_amd.h): the items, the tree and the reconstruction as for gainloss, then the eligibility, the
    sign, the smallest |r| and the pair limit."""
    _fields_ = [("type", C.c_int32), ("metric", C.c_int32), ("method", C.c_int32), ("gain", C.c_int32), ("loss", C.c_int32), ("mode", C.c_int32),
                ("min_events", C.c_int32), ("sign", C.c_int32), ("min_r", C.c_double), ("max_pair", C.c_int64)]


def coevo_opt(lib: C.CDLL, type: str = "gene", metric: str = "jaccard", method: str = "upgma", gain: int = 1, loss: int = 1, mode: str = "late",
              min_r: float = 0.8, min_events: int = 2, sign: str = "both", max_pair: int = ASSOC_MAX_PAIR) -> pg_coevo_opt_t:
    if type not in DIST_TYPES:
        raise ValueError("type must be gene or adj")
    if metric not in TREE_METRICS:
        raise ValueError("metric must be jaccard or diff")
    if method not in TREE_METHODS:
        raise ValueError("method must be upgma or nj")
    if not (1 <= int(gain) <= 255 and 1 <= int(loss) <= 255):
        raise ValueError("gain and loss must be in [1, 255]")
    if mode not in GAINLOSS_MODES:
        raise ValueError("mode must be late or early")
    if not 0.0 <= float(min_r) <= 1.0:
        raise ValueError("min_r must be in [0, 1]")
    if not 1 <= int(min_events) <= TREE_MAX_BOOT:
        raise ValueError("min_events must be in [1, 2^31 - 1]")
    if sign not in ASSOC_SIGNS:
        raise ValueError("sign must be pos, neg or both")
    if int(max_pair) < 0:
        raise ValueError("max_pair must not be negative")
    o = pg_coevo_opt_t()
    lib.pg_coevo_opt_init(C.byref(o))
    o.type, o.metric, o.method = DIST_TYPES.index(type), DIST_METRICS.index(metric), TREE_METHODS.index(method)
    o.gain, o.loss, o.mode, o.min_events, o.sign = int(gain), int(loss), GAINLOSS_MODES.index(mode), int(min_events), ASSOC_SIGNS.index(sign)
    o.min_r, o.max_pair = float(min_r), int(max_pair)
    return o


def pan_coevo(lib: C.CDLL, presence, rec, method: str, gain: int = 1, loss: int = 1, mode: str = "late", min_r: float = 0.8, min_events: int = 2,
              sign: str = "both", max_pair: int = ASSOC_MAX_PAIR):
    """Item pairs of an item x assembly presence matrix (bool numpy array or torch tensor, shape (M, A)) whose gains and losses fall on the
    same branches of the tree of the records rec (as for pan_gainloss) through pg_pan_coevo: (events, pairs) with events an int32 array
    (M,) of gains + losses per item and pairs an int32 array (n, 4) of (i, j, same, opp), i < j, ascending."""
    import numpy as np
    p = _presence(presence)
    M, A = p.shape
    m = TREE_METHODS.index(method)
    rec = np.ascontiguousarray(rec if rec is not None else np.zeros((0, 6)), dtype=np.int64).reshape(-1, 6)
    if A >= 3 and rec.shape[0] != A - 2 + m:
        raise ValueError("rec must hold %d records for %d assemblies and %s" % (A - 2 + m, A, method))
    o = coevo_opt(lib, method=method, gain=gain, loss=loss, mode=mode, min_r=min_r, min_events=min_events, sign=sign, max_pair=max_pair)
    events = np.zeros(M, dtype=np.int32)
    cap = 65536
    while True:  # the call says how many pairs there are; a second one fetches them when the first buffer was too small
        pairs = np.zeros((cap, 4), dtype=np.int32)
        n = lib.pg_pan_coevo(p.ctypes.data_as(C.POINTER(C.c_uint8)), M, A, rec.ctypes.data_as(C.POINTER(C.c_int64)), m, C.byref(o),
                             events.ctypes.data_as(C.POINTER(C.c_int32)), pairs.ctypes.data_as(C.POINTER(C.c_int32)), cap)
        if n < 0:
            raise RuntimeError("pg_pan_coevo: status %d" % n)
        if n <= cap:
            break
        cap = n
    return events, pairs[:n].copy()


def _coevo_args(argv: Sequence[str]):
    """The options of --coevo[=FLOAT] / --coevo-type= / --coevo-metric= / --coevo-method= / --coevo-gain= / --coevo-loss= /
    --coevo-resolve= / --coevo-min= / --coevo-sign= / --coevo-max= in argv as keywords of coevo_opt; None without --coevo."""
    on, extra, kw = False, False, {}
    names = {"type": "type", "metric": "metric", "method": "method", "gain": "gain", "loss": "loss", "resolve": "mode", "min": "min_events", "sign": "sign",
             "max": "max_pair"}
    for a in argv:
        if a == "--coevo": on = True
        elif a.startswith("--coevo="): on, kw["min_r"] = True, float(a.split("=", 1)[1])
        elif a.startswith("--coevo-") and "=" in a and a[8:].split("=", 1)[0] in names:
            k, v = a[8:].split("=", 1)
            kw[names[k]] = int(v) if k in ("gain", "loss", "min", "max") else v
            extra = True
        elif a.startswith("--coevo"):
            raise ValueError("unknown option or missing value: " + a)
    if extra and not on:
        raise ValueError("--coevo-type, --coevo-metric, --coevo-method, --coevo-gain, --coevo-loss, --coevo-resolve, --coevo-min, --coevo-sign and --coevo-max need --coevo")
    return kw if on else None


def _cluster_args(argv: Sequence[str]):
    """(k_lo, k_hi, type, metric, iterations) of --cluster=INT[-INT] / --cluster-type=STR / --cluster-metric=STR / --cluster-iter=INT in
    argv; k_lo = None without --cluster."""
    lo = hi = None
    t, m, it, extra = "gene", "jaccard", 1000, False
    for x in argv:
        if x.startswith("--cluster="):
            a, dash, b = x.split("=", 1)[1].partition("-")
            if not a.isdigit() or (dash and not b.isdigit()):
                raise ValueError("--cluster must be INT or INT-INT with 2 <= INT")
            lo, hi = int(a), int(b) if dash else int(a)
            if not 2 <= lo <= hi <= TREE_MAX_BOOT:
                raise ValueError("--cluster must be INT or INT-INT with 2 <= INT")
        elif x.startswith("--cluster-type="): t, extra = x.split("=", 1)[1], True
        elif x.startswith("--cluster-metric="): m, extra = x.split("=", 1)[1], True
        elif x.startswith("--cluster-iter="): it, extra = int(x.split("=", 1)[1]), True
        elif x.startswith("--cluster"):  # a bare --cluster, --cluster-type without a value, an unknown --cluster-* word
            raise ValueError("unknown option or missing value: " + x)
    if t not in DIST_TYPES:
        raise ValueError("--cluster-type must be gene or adj")
    if m not in TREE_METRICS:
        raise ValueError("--cluster-metric must be jaccard or diff")
    if not 0 <= it <= TREE_MAX_BOOT:
        raise ValueError("--cluster-iter must be in [0, 2^31 - 1]")
    if extra and lo is None:
        raise ValueError("--cluster-type, --cluster-metric and --cluster-iter need --cluster=INT[-INT]")
    return lo, hi, t, m, it


def _tree_boot_args(argv: Sequence[str]):
    """(replicates, seed) of --tree-boot=INT / --tree-seed=INT in argv"""
    b, seed = 0, 0
    for x in argv:
        if x.startswith("--tree-boot="): b = int(x.split("=", 1)[1])
        elif x.startswith("--tree-seed="):
            v = x.split("=", 1)[1]
            if not (v.isascii() and v.isdigit() and int(v) <= 0xFFFFFFFF):  # digits only, as the command line reads it
                raise ValueError("--tree-seed must be in [0, 2^32 - 1]")
            seed = int(v)
    if not 0 <= b <= TREE_MAX_BOOT:
        raise ValueError("--tree-boot must be in [0, 2^31 - 1]")
    return b, seed


def _tree_args(argv: Sequence[str]):
    """(type, metric, method) of --tree[=gene|adj] / --tree-metric=STR / --tree-method=STR in argv; type = None without --tree."""
    t, m, a = None, "jaccard", "nj"
    for x in argv:
        if x == "--tree": t = "gene"
        elif x.startswith("--tree="): t = x.split("=", 1)[1]
        elif x.startswith("--tree-metric="): m = x.split("=", 1)[1]
        elif x.startswith("--tree-method="): a = x.split("=", 1)[1]
    if t is not None and t not in DIST_TYPES:
        raise ValueError("--tree must be gene or adj")
    if m not in TREE_METRICS:
        raise ValueError("--tree-metric must be jaccard or diff")
    if a not in TREE_METHODS:
        raise ValueError("--tree-method must be nj or upgma")
    return t, m, a


# medoid, label, dist, size, sums, rec, rec_cap, n_rec, n_swap, td, converged of pg_pan_medoids / pg_pan_cluster
_MEDOIDS_OUT = [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]

_API = {
    "pg_opt_init": (None, [C.POINTER(pg_opt_t)]),
    "pg_data_init": (C.c_void_p, []),
    "pg_data_destroy": (None, [C.c_void_p]),
    "pg_read_paf": (C.c_int32, [C.POINTER(pg_opt_t), C.c_void_p, C.c_char_p]),
    "pg_scan_paf_ids": (C.c_int32, [C.POINTER(pg_opt_t), C.c_void_p, C.c_char_p]),
    "pg_read_paf_batch": (C.c_int32, [C.POINTER(pg_opt_t), C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint8), C.c_int32]),
    "pg_post_process": (None, [C.POINTER(pg_opt_t), C.c_void_p]),
    "pg_graph_init": (C.c_void_p, [C.c_void_p]),
    "pg_graph_gen": (None, [C.POINTER(pg_opt_t), C.c_void_p]),
    "pg_graph_destroy": (None, [C.c_void_p]),
    "pg_write_bed": (None, [C.c_void_p, C.c_int32]),
    "pg_write_graph": (None, [C.c_void_p]),
    "pg_write_walk": (None, [C.c_void_p]),
    "pg_write_matrix": (None, [C.c_void_p, C.c_int32]),
    "pg_gfa2matrix_file": (C.c_int, [C.c_char_p, C.c_int32, C.c_char_p, C.c_int32]),
    "pg_call_opt_init": (None, [C.c_void_p]),
    "pg_call_file": (C.c_int, [C.c_char_p, C.c_void_p]),
    "pg_write_call": (None, [C.c_void_p, C.c_void_p]),
    "pg_curves_opt_init": (None, [C.c_void_p]),
    "pg_curves_file": (C.c_int, [C.c_char_p, C.c_void_p]),
    "pg_write_curves": (None, [C.c_void_p, C.c_void_p]),
    "pg_pan_curves": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]),
    "pg_dist_opt_init": (None, [C.c_void_p]),
    "pg_dist_file": (C.c_int, [C.c_char_p, C.c_void_p]),
    "pg_write_dist": (None, [C.c_void_p, C.c_void_p]),
    "pg_pan_shared": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.POINTER(C.c_int32)]),
    "pg_pan_dist": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "pg_assoc_opt_init": (None, [C.c_void_p]),
    "pg_assoc_file": (C.c_int, [C.c_char_p, C.c_void_p]),
    "pg_write_assoc": (None, [C.c_void_p, C.c_void_p]),
    "pg_pan_assoc": (C.c_int64, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_int64]),
    "pg_trait_opt_init": (None, [C.c_void_p]),
    "pg_trait_file": (C.c_int, [C.c_char_p, C.c_char_p, C.c_void_p]),
    "pg_write_trait": (None, [C.c_void_p, C.c_char_p, C.c_void_p]),
    "pg_qtrait_opt_init": (None, [C.c_void_p]),
    "pg_qtrait_file": (C.c_int, [C.c_char_p, C.c_char_p, C.c_void_p]),
    "pg_write_qtrait": (None, [C.c_void_p, C.c_char_p, C.c_void_p]),
    "pg_permanova_opt_init": (None, [C.c_void_p]),
    "pg_permanova_file": (C.c_int, [C.c_char_p, C.c_char_p, C.c_void_p]),
    "pg_write_permanova": (None, [C.c_void_p, C.c_char_p, C.c_void_p]),
    "pg_pan_permanova": (C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int8), C.c_int32, C.c_void_p, C.POINTER(C.c_int64)]),
    "pg_pan_permanova_presence": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.POINTER(C.c_int8), C.c_int32, C.c_void_p, C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int32)]),
    "pg_mantel_opt_init": (None, [C.c_void_p]),
    "pg_mantel_file": (C.c_int, [C.c_char_p, C.c_char_p, C.c_void_p]),
    "pg_write_mantel": (None, [C.c_void_p, C.c_char_p, C.c_void_p]),
    "pg_pan_mantel": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.POINTER(C.c_int64)]),
    "pg_gainloss_opt_init": (None, [C.c_void_p]),
    "pg_gainloss_file": (C.c_int, [C.c_char_p, C.c_void_p]),
    "pg_write_gainloss": (None, [C.c_void_p, C.c_void_p]),
    "pg_pan_gainloss": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "pg_coevo_opt_init": (None, [C.c_void_p]),
    "pg_coevo_file": (C.c_int, [C.c_char_p, C.c_void_p]),
    "pg_write_coevo": (None, [C.c_void_p, C.c_void_p]),
    "pg_pan_coevo": (C.c_int64, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64]),
    "pg_pan_qtrait": (C.c_int, [C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]),
    "pg_pan_trait": (C.c_int, [C.POINTER(C.c_uint8), C.POINTER(C.c_int8), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]),
    "pg_pan_pairs": (C.c_int, [C.POINTER(C.c_uint8), C.POINTER(C.c_int8), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int32)]),
    "pg_tree_opt_init": (None, [C.c_void_p]),
    "pg_tree_file": (C.c_int, [C.c_char_p, C.c_void_p]),
    "pg_write_tree": (None, [C.c_void_p, C.c_void_p]),
    "pg_pan_join": (C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "pg_pan_tree": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "pg_cluster_opt_init": (None, [C.c_void_p]),
    "pg_cluster_file": (C.c_int, [C.c_char_p, C.c_void_p]),
    "pg_write_cluster": (None, [C.c_void_p, C.c_void_p]),
    "pg_pan_medoids": (C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32] + _MEDOIDS_OUT),
    "pg_pan_cluster": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + _MEDOIDS_OUT + [C.POINTER(C.c_int32)]),
    "pg_pan_boot": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                              C.POINTER(C.c_int32)]),
    "pg_pan_boot_records": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "pg_read_list_dict": (C.c_void_p, [C.c_char_p]),
    "pg_dict_destroy": (None, [C.c_void_p]),
    "pg_last_error": (C.c_int, []),
    "pg_last_error_str": (C.c_char_p, []),
    "pg_set_output": (C.c_int, [C.c_char_p]),
    "pg_set_exchange": (None, [C.POINTER(pg_exchange_t)]),
    "pg_last_path_seconds": (C.c_double, []),
    "pg_last_path_hits": (C.c_int64, []),
    "pg_last_attempts": (C.c_int, []),
    "pg_device_copy_gbps": (C.c_double, [C.c_size_t, C.c_int32]),
    "pg_trim_host_cache": (None, [C.c_size_t]),
    "pg_last_upload_seconds": (C.c_double, []),
    "pg_last_pack_seconds": (C.c_double, []),
    "pg_last_reserve_seconds": (C.c_double, []),
    "pg_shard_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pg_rerun_resident": (C.c_int, [C.c_void_p]),
    "pg_kernel_timing": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "pg_kernel_timing_reset": (C.c_int, [C.c_void_p]),
    "pg_collective_count": (C.c_int64, []),
    "pg_set_exact_mode": (None, [C.c_int]),
    "pg_phase_times": (C.c_int, [C.POINTER(C.c_double), C.c_int]),
    "pg_phase_name": (C.c_char_p, [C.c_int]),
}

# only in the HIP product library (the oracle-host test library has no RCCL exchange)
_API_HIP_ONLY = {
    "pg_rccl_unique_id": (C.c_int, [C.c_void_p]),
    "pg_rccl_init": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p]),
    "pg_rccl_finalize": (C.c_int, []),
    "pg_rccl_error": (C.c_char_p, []),
}


def load(path: str = LIB_HIP) -> C.CDLL:
    """The product library (default), or another build of the pangene.h surface at `path` (tests: the checker build)."""
    hip = os.path.abspath(path) == os.path.abspath(LIB_HIP)
    if not os.path.exists(path):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` first" % path)
    lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_NOW)
    for name, (res, args) in _API.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    if hip:
        for name, (res, args) in _API_HIP_ONLY.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def parse_args(lib: C.CDLL, argv: Sequence[str]) -> pg_opt_t:
    """The option letters of the reference's main.c:70-113."""
    opt = pg_opt_t()
    lib.pg_opt_init(C.byref(opt))
    it = iter(argv)
    for a in it:
        if a == "-J": opt.flag |= PG_F_NO_JOINT_PSEUDO
        elif a == "-E": opt.flag |= PG_F_DROP_SGL_EXON
        elif a == "-F": opt.flag |= PG_F_FRAG_MODE
        elif a == "-S": opt.flag |= PG_F_CHECK_STRAND
        elif a == "-w": opt.flag |= PG_F_WRITE_NO_WALK
        elif a == "-G": opt.flag |= PG_F_WRITE_VTX_SEL
        elif a == "--ori-sc": opt.flag |= PG_F_ORI_FOR_BRANCH
        elif a in ("--bed", "--bed=walk"): opt.flag |= PG_F_WRITE_BED_WALK
        elif a == "--bed=raw": opt.flag |= PG_F_WRITE_BED_RAW
        elif a == "--bed=flag": opt.flag |= PG_F_WRITE_BED_FLAG
        elif a in ("--matrix", "--matrix=presence", "--matrix=count", "--call") or a.startswith("--curves") or a.startswith("--dist") or a.startswith("--assoc") or a.startswith("--trait") or a.startswith("--qtrait") or a.startswith("--tree") or a.startswith("--cluster") or a.startswith("--permanova") or a.startswith("--mantel") or a.startswith("--gainloss") or a.startswith("--coevo"): pass  # handled by run()
        elif a[:2] in ("-p", "-a", "-f", "-c", "-g", "-r", "-b", "-B", "-y", "-T", "-D", "-C", "-e", "-l", "-m", "-d", "-X", "-I", "-P"):
            v = a[2:] if len(a) > 2 else next(it)
            k = a[1]
            if k == "p": opt.min_vertex_ratio = float(v)
            elif k == "a": opt.min_arc_cnt = int(v)
            elif k == "f": opt.min_ov_ratio = float(v)
            elif k == "c": opt.max_avg_occ = int(v)
            elif k == "g": opt.max_degree = int(v)
            elif k == "r": opt.max_dist_loci = int(v)
            elif k == "b": opt.branch_diff = float(v)
            elif k == "B": opt.branch_diff_cut = float(v)
            elif k == "y": opt.branch_diff_dist = float(v)
            elif k == "T": opt.n_branch_flt = int(float(v))
            elif k == "D": opt.local_dist = int(float(v) + .499)
            elif k == "C": opt.local_count = int(v)
            elif k == "e": opt.min_prot_iden = float(v)
            elif k == "l": opt.min_prot_ratio = float(v)
            elif k == "m": opt.score_adj_coef = float(v)
            elif k == "d": opt.gene_delim = ord(v[0])
            elif k == "X": opt.excl = lib.pg_read_list_dict(v.encode())
            elif k == "I": opt.incl = lib.pg_read_list_dict(v.encode())
            elif k == "P": opt.preferred = lib.pg_read_list_dict(v.encode())
        else:
            raise ValueError("unknown option " + a)
    return opt


def read_files(lib: C.CDLL, opt, d, files: Sequence[str], scan_only: Sequence[bool] | None = None, n_threads: int = 0, batch: bool = True) -> int:
    """main.c:121-122 for all files: parsed on host threads (pg_read_paf_batch) or one pg_read_paf / pg_scan_paf_ids per file."""
    n = len(files)
    if not batch:
        rc = 0
        for k, f in enumerate(files):
            fn = lib.pg_scan_paf_ids if scan_only is not None and scan_only[k] else lib.pg_read_paf
            rc += min(0, fn(C.byref(opt), d, f.encode()))
        return rc
    fns = (C.c_char_p * max(n, 1))(*[f.encode() for f in files])
    mask = (C.c_uint8 * max(n, 1))(*[1 if scan_only is not None and scan_only[k] else 0 for k in range(n)])
    return lib.pg_read_paf_batch(C.byref(opt), d, n, fns, mask, n_threads)


def run(lib: C.CDLL, files: Sequence[str], argv: Sequence[str] = (), scan_only: Sequence[bool] | None = None, batch: bool = True) -> bytes:
    """main.c:117-142 in-process: returns what the command line would print to stdout."""
    opt = parse_args(lib, argv)
    n_curves, curves_seed = _curves_args(argv)
    if n_curves and (any(x.startswith("--matrix") for x in argv) or "--call" in argv):
        raise ValueError("--curves cannot be combined with --matrix or --call")
    dist_type, dist_metric = _dist_args(argv)
    if dist_type is not None and (any(x.startswith("--matrix") for x in argv) or "--call" in argv or n_curves):
        raise ValueError("--dist cannot be combined with --matrix, --call or --curves")
    assoc_phi, assoc_count, assoc_sign = _assoc_args(argv)
    if assoc_phi is not None and (any(x.startswith("--matrix") for x in argv) or "--call" in argv or n_curves or dist_type is not None):
        raise ValueError("--assoc cannot be combined with --matrix, --call, --curves or --dist")
    trait_fn, trait_n, trait_seed, trait_lineage = _trait_args(argv)
    if trait_fn is not None and (any(x.startswith("--matrix") for x in argv) or "--call" in argv or n_curves or dist_type is not None or assoc_phi is not None):
        raise ValueError("--trait cannot be combined with --matrix, --call, --curves, --dist or --assoc")
    tree_type, tree_metric, tree_method = _tree_args(argv)
    tree_boot, tree_seed = _tree_boot_args(argv)
    if tree_type is not None and (any(x.startswith("--matrix") for x in argv) or "--call" in argv or n_curves or dist_type is not None or assoc_phi is not None
                                  or trait_fn is not None):
        raise ValueError("--tree cannot be combined with --matrix, --call, --curves, --dist, --assoc or --trait")
    qtrait_fn, qtrait_n, qtrait_seed = _qtrait_args(argv)
    if qtrait_fn is not None and (any(x.startswith("--matrix") for x in argv) or "--call" in argv or n_curves or dist_type is not None or assoc_phi is not None
                                  or trait_fn is not None or tree_type is not None):
        raise ValueError("--qtrait cannot be combined with --matrix, --call, --curves, --dist, --assoc, --trait or --tree")
    cl_lo, cl_hi, cl_type, cl_metric, cl_iter = _cluster_args(argv)
    if cl_lo is not None and (any(x.startswith("--matrix") for x in argv) or "--call" in argv or n_curves or dist_type is not None or assoc_phi is not None
                              or trait_fn is not None or tree_type is not None or qtrait_fn is not None):
        raise ValueError("--cluster cannot be combined with --matrix, --call, --curves, --dist, --assoc, --trait, --tree or --qtrait")
    pm_fn, pm_type, pm_metric, pm_n, pm_seed = _permanova_args(argv)
    if pm_fn is not None and (any(x.startswith("--matrix") for x in argv) or "--call" in argv or n_curves or dist_type is not None or assoc_phi is not None
                              or trait_fn is not None or tree_type is not None or qtrait_fn is not None or cl_lo is not None):
        raise ValueError("--permanova cannot be combined with --matrix, --call, --curves, --dist, --assoc, --trait, --tree, --qtrait or --cluster")
    mt_on, mt_fn, mt_x, mt_y, mt_n, mt_seed = _mantel_args(argv)
    if mt_on and (any(x.startswith("--matrix") for x in argv) or "--call" in argv or n_curves or dist_type is not None or assoc_phi is not None
                  or trait_fn is not None or tree_type is not None or qtrait_fn is not None or cl_lo is not None or pm_fn is not None):
        raise ValueError("--mantel cannot be combined with --matrix, --call, --curves, --dist, --assoc, --trait, --tree, --qtrait, --cluster or --permanova")
    gl_kw = _gainloss_args(argv)
    if gl_kw is not None and (any(x.startswith("--matrix") for x in argv) or "--call" in argv or n_curves or dist_type is not None or assoc_phi is not None
                              or trait_fn is not None or tree_type is not None or qtrait_fn is not None or cl_lo is not None or pm_fn is not None or mt_on):
        raise ValueError("--gainloss cannot be combined with --matrix, --call, --curves, --dist, --assoc, --trait, --tree, --qtrait, --cluster, --permanova or --mantel")
    gl_opt = gainloss_opt(lib, **gl_kw) if gl_kw is not None else None
    ce_kw = _coevo_args(argv)
    if ce_kw is not None and (any(x.startswith("--matrix") for x in argv) or "--call" in argv or n_curves or dist_type is not None or assoc_phi is not None
                              or trait_fn is not None or tree_type is not None or qtrait_fn is not None or cl_lo is not None or pm_fn is not None or mt_on
                              or gl_kw is not None):
        raise ValueError("--coevo cannot be combined with --matrix, --call, --curves, --dist, --assoc, --trait, --tree, --qtrait, --cluster, --permanova, --mantel or --gainloss")
    ce_opt = coevo_opt(lib, **ce_kw) if ce_kw is not None else None
    fd, out = tempfile.mkstemp(prefix="pangene_", suffix=".out")
    os.close(fd)
    lib.pg_set_output(out.encode())
    d = lib.pg_data_init()
    try:
        read_files(lib, opt, d, files, scan_only, batch=batch)
        lib.pg_post_process(C.byref(opt), d)
        if lib.pg_last_error():
            raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
        if opt.flag & PG_F_WRITE_BED_RAW:
            lib.pg_write_bed(d, 0)
        else:
            g = lib.pg_graph_init(d)
            lib.pg_graph_gen(C.byref(opt), g)
            if lib.pg_last_error():
                raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
            if any(x.startswith("--matrix") for x in argv): lib.pg_write_matrix(g, 1 if "--matrix=count" in argv else 0)
            elif "--call" in argv:
                co = pg_call_opt_t()
                lib.pg_call_opt_init(C.byref(co))
                lib.pg_write_call(g, C.byref(co))
                if lib.pg_last_error():
                    raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
            elif n_curves:
                lib.pg_write_curves(g, C.byref(curves_opt(lib, n_curves, curves_seed)))
                if lib.pg_last_error():
                    raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
            elif dist_type is not None:
                lib.pg_write_dist(g, C.byref(dist_opt(lib, dist_type, dist_metric)))
                if lib.pg_last_error():
                    raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
            elif assoc_phi is not None:
                lib.pg_write_assoc(g, C.byref(assoc_opt(lib, assoc_phi, assoc_count, assoc_sign)))
                if lib.pg_last_error():
                    raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
            elif trait_fn is not None:
                lib.pg_write_trait(g, trait_fn.encode(), C.byref(trait_opt(lib, trait_n, trait_seed, lineage=trait_lineage)))
                if lib.pg_last_error():
                    raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
            elif qtrait_fn is not None:
                lib.pg_write_qtrait(g, qtrait_fn.encode(), C.byref(qtrait_opt(lib, qtrait_n, qtrait_seed)))
                if lib.pg_last_error():
                    raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
            elif tree_type is not None:
                lib.pg_write_tree(g, C.byref(tree_opt(lib, tree_type, tree_metric, tree_method, tree_boot, tree_seed)))
                if lib.pg_last_error():
                    raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
            elif cl_lo is not None:
                lib.pg_write_cluster(g, C.byref(cluster_opt(lib, cl_lo, cl_hi, cl_type, cl_metric, cl_iter)))
                if lib.pg_last_error():
                    raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
            elif pm_fn is not None:
                lib.pg_write_permanova(g, pm_fn.encode(), C.byref(permanova_opt(lib, pm_type, pm_metric, pm_n, pm_seed)))
                if lib.pg_last_error():
                    raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
            elif mt_on:
                lib.pg_write_mantel(g, mt_fn.encode() if mt_fn is not None else None, C.byref(mantel_opt(lib, mt_x, mt_y, mt_n, mt_seed)))
                if lib.pg_last_error():
                    raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
            elif gl_opt is not None:
                lib.pg_write_gainloss(g, C.byref(gl_opt))
                if lib.pg_last_error():
                    raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
            elif ce_opt is not None:
                lib.pg_write_coevo(g, C.byref(ce_opt))
                if lib.pg_last_error():
                    raise RuntimeError("pangene_amd: " + lib.pg_last_error_str().decode())
            elif opt.flag & PG_F_WRITE_BED_WALK: lib.pg_write_bed(d, 1)
            elif opt.flag & PG_F_WRITE_BED_FLAG: lib.pg_write_bed(d, 0)
            else:
                lib.pg_write_graph(g)
                if not (opt.flag & PG_F_WRITE_NO_WALK): lib.pg_write_walk(g)
            lib.pg_graph_destroy(g)
    finally:
        lib.pg_data_destroy(d)
        for h in (opt.excl, opt.incl, opt.preferred):
            if h: lib.pg_dict_destroy(h)
        lib.pg_set_output(None)
    with open(out, "rb") as fh:
        data = fh.read()
    os.unlink(out)
    return data
