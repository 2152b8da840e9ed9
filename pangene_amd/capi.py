"""ctypes bindings of the C ABI in include/pangene_amd.h (the pangene.h-compatible surface).

Nothing here computes: every call goes into libpangene_amd.so (HIP backend).  (The checker build of the same host
driver -- linked against the plain-C oracle -- is loaded by tests/oracle_host.py, which hands its own path to load();
nothing in this package knows where it is.)
"""
from __future__ import annotations

import collections
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


class pg_mantel_opt_t(C.Structure):
    """Mantel options (include/pangene_amd.h): the two matrices, the permutations and their seed."""
    _fields_ = [("x_type", C.c_int32), ("x_metric", C.c_int32), ("y_type", C.c_int32), ("y_metric", C.c_int32), ("n_perm", C.c_int32), ("seed", C.c_uint32)]


def _spec_ok(spec: str) -> bool:
    t, colon, m = spec.partition(":")
    return bool(colon) and t in DIST_TYPES and m in TREE_METRICS


def _mantel_spec(spec: str, what: str):
    """(type index, metric index) of gene|adj:jaccard|diff"""
    if not _spec_ok(spec):
        raise ValueError(what + " must be gene|adj:jaccard|diff")
    t, m = spec.split(":", 1)
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


class pg_rates_opt_t(C.Structure):
    """Gain and loss rate options (include/pangene_amd.h): the items, the tree, the table, the two rates (0 = fitted) and the table's filter."""
    _fields_ = [("type", C.c_int32), ("metric", C.c_int32), ("method", C.c_int32), ("out", C.c_int32), ("gain", C.c_double), ("loss", C.c_double),
                ("min_changes", C.c_double)]


RATES_MIN, RATES_MAX = 1e-9, 1e9


def rates_opt(lib: C.CDLL, type: str = "gene", metric: str = "jaccard", method: str = "upgma", out: str = "gene", gain: float = 0.0, loss: float = 0.0,
              min_changes: float = 0.0) -> pg_rates_opt_t:
    if type not in DIST_TYPES:
        raise ValueError("type must be gene or adj")
    if metric not in TREE_METRICS:
        raise ValueError("metric must be jaccard or diff")
    if method not in TREE_METHODS:
        raise ValueError("method must be upgma or nj")
    if out not in GAINLOSS_OUTS:
        raise ValueError("out must be gene or node")
    gain, loss = float(gain), float(loss)
    if not ((gain == 0.0 and loss == 0.0) or (RATES_MIN <= gain <= RATES_MAX and RATES_MIN <= loss <= RATES_MAX)):
        raise ValueError("gain and loss must both be in [1e-9, 1e9], or both be left out")
    if not float(min_changes) >= 0.0:
        raise ValueError("min_changes must be a number >= 0")
    o = pg_rates_opt_t()
    lib.pg_rates_opt_init(C.byref(o))
    o.type, o.metric, o.method, o.out = DIST_TYPES.index(type), DIST_METRICS.index(metric), TREE_METHODS.index(method), GAINLOSS_OUTS.index(out)
    o.gain, o.loss, o.min_changes = gain, loss, float(min_changes)
    return o


def pan_rates(lib: C.CDLL, presence, rec, method: str, gain: float = 0.0, loss: float = 0.0):
    """Maximum-likelihood gain and loss rates of the items of an item x assembly presence matrix (bool numpy array or torch tensor, shape
    (M, A)) on the tree of the records rec (as for pan_gainloss; their distances give the branch lengths) through pg_pan_rates.  gain and
    loss both 0: fitted; both given: nothing is fitted.  A dict: gain, loss, lnL, T (floats), rounds, converged (ints); per item, float64
    (M,): lnL_item, gains, losses, root, rate, lrt, p_rate (NaN for an item absent from every assembly); per node, float64 (2 A - 1,):
    node_length, node_present, node_gains, node_losses (leaf x = x, join s = A + s)."""
    import numpy as np
    p = _presence(presence)
    M, A = p.shape
    m = TREE_METHODS.index(method)
    rec = np.ascontiguousarray(rec if rec is not None else np.zeros((0, 6)), dtype=np.int64).reshape(-1, 6)
    if A >= 3 and rec.shape[0] != A - 2 + m:
        raise ValueError("rec must hold %d records for %d assemblies and %s" % (A - 2 + m, A, method))
    o = rates_opt(lib, method=method, gain=gain, loss=loss)
    fit = np.zeros(6, dtype=np.float64)
    gene = np.zeros((M, 7), dtype=np.float64)
    node = np.zeros((max(2 * A - 1, 0), 4), dtype=np.float64)
    rc = lib.pg_pan_rates(p.ctypes.data_as(C.POINTER(C.c_uint8)), M, A, rec.ctypes.data_as(C.POINTER(C.c_int64)), m, C.byref(o),
                          fit.ctypes.data_as(C.POINTER(C.c_double)), gene.ctypes.data_as(C.POINTER(C.c_double)), node.ctypes.data_as(C.POINTER(C.c_double)))
    if rc != 0:
        raise RuntimeError("pg_pan_rates: status %d" % rc)
    out = {"gain": float(fit[0]), "loss": float(fit[1]), "lnL": float(fit[2]), "rounds": int(fit[3]), "converged": int(fit[4]), "T": float(fit[5])}
    out.update({k: np.ascontiguousarray(gene[:, i]) for i, k in enumerate(("lnL_item", "gains", "losses", "root", "rate", "lrt", "p_rate"))})
    out.update({"node_" + k: np.ascontiguousarray(node[:, i]) for i, k in enumerate(("length", "present", "gains", "losses"))})
    return out


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


class pg_phylosig_opt_t(C.Structure):
    """Phylogenetic signal options (include/pangene_amd.h): the items, the tree and the costs as for gainloss, then the permutations, their
    seed, the smallest count of a tested item and the filter of the table."""
    _fields_ = [("type", C.c_int32), ("metric", C.c_int32), ("method", C.c_int32), ("gain", C.c_int32), ("loss", C.c_int32), ("n_perm", C.c_int32),
                ("seed", C.c_uint32), ("min_count", C.c_int32), ("max_p", C.c_double)]


def phylosig_opt(lib: C.CDLL, type: str = "gene", metric: str = "jaccard", method: str = "upgma", gain: int = 1, loss: int = 1, n_perm: int = 1000,
                 seed: int = 11, min_count: int = 2, max_p: float = 1.0) -> pg_phylosig_opt_t:
    if type not in DIST_TYPES:
        raise ValueError("type must be gene or adj")
    if metric not in TREE_METRICS:
        raise ValueError("metric must be jaccard or diff")
    if method not in TREE_METHODS:
        raise ValueError("method must be upgma or nj")
    if not (1 <= int(gain) <= 255 and 1 <= int(loss) <= 255):
        raise ValueError("gain and loss must be in [1, 255]")
    if not 0 <= int(n_perm) <= TRAIT_MAX_PERM:
        raise ValueError("n_perm must be in [0, 2^31 - 2]")
    if not 0 <= int(seed) <= 0xFFFFFFFF:
        raise ValueError("seed must be in [0, 2^32 - 1]")
    if not 1 <= int(min_count) <= TREE_MAX_BOOT:
        raise ValueError("min_count must be in [1, 2^31 - 1]")
    if not float(max_p) >= 0.0:
        raise ValueError("max_p must be a number >= 0")
    o = pg_phylosig_opt_t()
    lib.pg_phylosig_opt_init(C.byref(o))
    o.type, o.metric, o.method = DIST_TYPES.index(type), DIST_METRICS.index(metric), TREE_METHODS.index(method)
    o.gain, o.loss, o.n_perm, o.seed, o.min_count, o.max_p = int(gain), int(loss), int(n_perm), int(seed), int(min_count), float(max_p)
    return o


def pan_phylosig(lib: C.CDLL, presence, rec, method: str, gain: int = 1, loss: int = 1, n_perm: int = 1000, seed: int = 11, min_count: int = 2):
    """The permutation tail of the parsimony cost of the items of an item x assembly presence matrix (bool numpy array or torch tensor,
    shape (M, A)) on the tree of the records rec (as for pan_gainloss) through pg_pan_phylosig: a dict of numpy arrays: present, cost,
    tested, n_le and n_ge, int32 (M,), per item; sum, int64 (A + 1,), indexed by the class size n (0 for a class that did not run)."""
    import numpy as np
    p = _presence(presence)
    M, A = p.shape
    m = TREE_METHODS.index(method)
    rec = np.ascontiguousarray(rec if rec is not None else np.zeros((0, 6)), dtype=np.int64).reshape(-1, 6)
    if A >= 3 and rec.shape[0] != A - 2 + m:
        raise ValueError("rec must hold %d records for %d assemblies and %s" % (A - 2 + m, A, method))
    o = phylosig_opt(lib, method=method, gain=gain, loss=loss, n_perm=n_perm, seed=seed, min_count=min_count)
    item = np.zeros((M, 5), dtype=np.int32)
    total = np.zeros(A + 1, dtype=np.int64)
    rc = lib.pg_pan_phylosig(p.ctypes.data_as(C.POINTER(C.c_uint8)), M, A, rec.ctypes.data_as(C.POINTER(C.c_int64)), m, C.byref(o),
                             item.ctypes.data_as(C.POINTER(C.c_int32)), total.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != 0:
        raise RuntimeError("pg_pan_phylosig: status %d" % rc)
    out = {k: np.ascontiguousarray(item[:, i]) for i, k in enumerate(("present", "cost", "tested", "n_le", "n_ge"))}
    out["sum"] = total
    return out


class pg_pcoa_opt_t(C.Structure):
    """Principal coordinates options (include/pangene_amd.h): items, distance, axes and the seed of the start vectors."""
    _fields_ = [("type", C.c_int32), ("metric", C.c_int32), ("n_axis", C.c_int32), ("seed", C.c_uint32)]


PCOA_MAX_AXIS = 16


def pcoa_opt(lib: C.CDLL, type: str = "gene", metric: str = "jaccard", n_axis: int = 3, seed: int = 0) -> pg_pcoa_opt_t:
    if type not in DIST_TYPES:
        raise ValueError("type must be gene or adj")
    if metric not in TREE_METRICS:
        raise ValueError("metric must be jaccard or diff (shared is not a distance)")
    if not 1 <= int(n_axis) <= PCOA_MAX_AXIS:
        raise ValueError("n_axis must be in [1, 16]")
    if not 0 <= int(seed) <= 0xFFFFFFFF:
        raise ValueError("seed must be in [0, 2^32 - 1]")
    o = pg_pcoa_opt_t()
    lib.pg_pcoa_opt_init(C.byref(o))
    o.type, o.metric, o.n_axis, o.seed = DIST_TYPES.index(type), DIST_METRICS.index(metric), int(n_axis), int(seed)
    return o


def _pcoa_out(n, k):
    import numpy as np
    out = {"eig": np.zeros(k), "resid": np.zeros(k), "coord": np.zeros((n, k)), "trace": C.c_double(0.0), "info": np.zeros(4, dtype=np.int32)}
    ptr = [out[key].ctypes.data_as(C.POINTER(C.c_double)) for key in ("eig", "resid", "coord")] + [C.byref(out["trace"]), out["info"].ctypes.data_as(C.POINTER(C.c_int32))]
    return out, ptr


def _pcoa_dict(out):
    axes, steps, converged, restarts = (int(v) for v in out["info"])
    return {"axes": axes, "steps": steps, "converged": converged, "restarts": restarts, "trace": float(out["trace"].value), "eig": out["eig"][:axes].copy(),
            "resid": out["resid"][:axes].copy(), "coord": out["coord"][:, :axes].copy()}


def pan_pcoa(lib: C.CDLL, q, fbits: int = 20, n_axis: int = 3, seed: int = 0):
    """Principal coordinates of a fixed-point distance matrix (int32 numpy array or torch tensor, shape (n, n), symmetric, zero diagonal,
    entries in [0, 2^29), fbits fraction bits) through pg_pan_pcoa: a dict with axes (the axes returned: those above 1e-9 of the first),
    steps, converged, restarts, trace, and float64 arrays eig (axes,), resid (axes,) and coord (n, axes).  Fewer than 3 assemblies or no
    distance above zero: no axes."""
    import numpy as np
    if hasattr(q, "detach"):  # torch tensor, on any device
        q = q.detach().cpu().numpy()
    q = np.ascontiguousarray(q, dtype=np.int32)
    if q.ndim != 2 or q.shape[0] != q.shape[1]:
        raise ValueError("q must be a square matrix")
    o = pg_pcoa_opt_t()
    lib.pg_pcoa_opt_init(C.byref(o))
    o.n_axis, o.seed = int(n_axis), int(seed) & 0xFFFFFFFF  # (the library checks n_axis: PGA_ERR_RANGE)
    n, k = q.shape[0], max(int(n_axis), 1)
    out, ptr = _pcoa_out(n, k)
    rc = lib.pg_pan_pcoa(q.ctypes.data_as(C.POINTER(C.c_int32)), n, int(fbits), C.byref(o), *ptr)
    if rc != 0:
        raise RuntimeError("pg_pan_pcoa: status %d" % rc)
    return _pcoa_dict(out)


def pan_pcoa_presence(lib: C.CDLL, presence, metric: str = "jaccard", n_axis: int = 3, seed: int = 0):
    """The same for an item x assembly presence matrix (bool numpy array or torch tensor, shape (M, A)) through pg_pan_pcoa_presence:
    (the dict pan_pcoa returns, F) with the distances of `metric` in units of 2^-F."""
    p = _presence(presence)
    M, A = p.shape
    o = pcoa_opt(lib, metric=metric, n_axis=n_axis, seed=seed)
    out, ptr = _pcoa_out(A, int(n_axis))
    F = C.c_int32(0)
    rc = lib.pg_pan_pcoa_presence(p.ctypes.data_as(C.POINTER(C.c_uint8)), M, A, C.byref(o), *ptr, C.byref(F))
    if rc != 0:
        raise RuntimeError("pg_pan_pcoa_presence: status %d" % rc)
    return _pcoa_dict(out), int(F.value)


class pg_glm_opt_t(C.Structure):
    """Structure-adjusted association options (include/pangene_amd.h): the distance of the axes, the family, the axes, their seed, the filters."""
    _fields_ = [("type", C.c_int32), ("metric", C.c_int32), ("family", C.c_int32), ("n_axis", C.c_int32), ("seed", C.c_uint32), ("min_count", C.c_int32),
                ("max_p", C.c_double)]


GLM_FAMILIES = ("binary", "quant")
GLM_MAX_AXIS = 13


def glm_opt(lib: C.CDLL, family: str = "binary", n_axis: int = 3, type: str = "gene", metric: str = "jaccard", seed: int = 0, min_count: int = 1,
            max_p: float = 1.0) -> pg_glm_opt_t:
    if family not in GLM_FAMILIES:
        raise ValueError("family must be binary or quant")
    if not 0 <= int(n_axis) <= GLM_MAX_AXIS:
        raise ValueError("n_axis must be in [0, 13]")
    if type not in DIST_TYPES:
        raise ValueError("type must be gene or adj")
    if metric not in TREE_METRICS:
        raise ValueError("metric must be jaccard or diff (shared is not a distance)")
    if not 0 <= int(seed) <= 0xFFFFFFFF:
        raise ValueError("seed must be in [0, 2^32 - 1]")
    if int(min_count) < 1:
        raise ValueError("min_count must be at least 1")
    if not float(max_p) >= 0.0:
        raise ValueError("max_p must be a number >= 0")
    o = pg_glm_opt_t()
    lib.pg_glm_opt_init(C.byref(o))
    o.type, o.metric, o.family, o.n_axis = DIST_TYPES.index(type), DIST_METRICS.index(metric), GLM_FAMILIES.index(family), int(n_axis)
    o.seed, o.min_count, o.max_p = int(seed), int(min_count), float(max_p)
    return o


def pan_glm(lib: C.CDLL, presence, values, covariates=None, family: str = "binary", min_count: int = 1):
    """Score statistics of every gene of a presence matrix (bool numpy array or torch tensor, shape (G, A)) against the traits `values`
    (float64, shape (T, A), NaN = missing; 0 and 1 for the binary family) given explicit covariates (float64, shape (A, k), k <= 13, or
    None) through pg_pan_glm: a dict of arrays a (T, G; -1 = not eligible), U, V, s_w (T, G) and N, iterations, fit, tested (T,)."""
    import numpy as np
    p = _presence(presence)
    G, A = p.shape
    if hasattr(values, "detach"):
        values = values.detach().cpu().numpy()
    v = np.ascontiguousarray(values, dtype=np.float64)
    if v.ndim == 1:
        v = v.reshape(1, -1)
    if v.ndim != 2 or v.shape[1] != A:
        raise ValueError("values must have one column per assembly")
    T = v.shape[0]
    if covariates is None:
        cov, k = np.zeros((A, 0)), 0
    else:
        if hasattr(covariates, "detach"):
            covariates = covariates.detach().cpu().numpy()
        cov = np.ascontiguousarray(covariates, dtype=np.float64)
        if cov.ndim == 1:
            cov = cov.reshape(-1, 1)
        if cov.ndim != 2 or cov.shape[0] != A:
            raise ValueError("covariates must have one row per assembly")
        k = cov.shape[1]
    if family not in GLM_FAMILIES:
        raise ValueError("family must be binary or quant")
    o = pg_glm_opt_t()
    lib.pg_glm_opt_init(C.byref(o))
    o.min_count = int(min_count)
    out, info = np.zeros((T, G, 4)), np.zeros((T, 4), dtype=np.int32)
    rc = lib.pg_pan_glm(p.ctypes.data_as(C.POINTER(C.c_uint8)), v.ctypes.data_as(C.POINTER(C.c_double)), G, A, T,
                        cov.ctypes.data_as(C.POINTER(C.c_double)) if k else None, k, GLM_FAMILIES.index(family), C.byref(o),
                        out.ctypes.data_as(C.POINTER(C.c_double)), info.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise RuntimeError("pg_pan_glm: status %d" % rc)
    return {"a": out[:, :, 0].astype(np.int64), "U": out[:, :, 1].copy(), "V": out[:, :, 2].copy(), "s_w": out[:, :, 3].copy(), "N": info[:, 0].copy(),
            "iterations": info[:, 1].copy(), "fit": info[:, 2].copy(), "tested": info[:, 3].copy()}


# ---- the long options of the analyses, as run() reads them: one table, one reader -------------------------------------------------
# A row is one --NAME-suffix=VALUE (the head row, without a suffix, is the VALUE of --NAME=VALUE): the keyword of NAME_opt() it fills,
# the converter (its ValueError is raised where the option stands), and a test of the last value given with the words after the option's
# name when it fails.  `extra` rows are refused without their --NAME; `phase` 1 rows are read after the others have been checked.
_Row = collections.namedtuple("_Row", "suffix kw conv ok msg extra phase needs_head no_file", defaults=(str, None, None, False, 0, False, False))


def _words(suffix, kw, words, msg, **k):
    return _Row(suffix, kw, str, lambda v: v in words, msg, **k)


def _ints(suffix, kw, lo, hi, msg, **k):
    return _Row(suffix, kw, int, lambda v: lo <= v <= hi, msg, **k)


def _seed32(v):  # digits only, as the command line reads it
    if not (v.isascii() and v.isdigit() and int(v) <= 0xFFFFFFFF):
        raise ValueError("--tree-seed must be in [0, 2^32 - 1]")
    return int(v)


def _k_range(v):
    a, dash, b = v.partition("-")
    if not a.isdigit() or (dash and not b.isdigit()) or not 2 <= int(a) <= int(b if dash else a) <= TREE_MAX_BOOT:
        raise ValueError("--cluster must be INT or INT-INT with 2 <= INT")
    return int(a), int(b if dash else a)


# name: of --NAME; opt: the builder NAME_opt(); write: the library's pg_write_NAME; form: --NAME in the messages; bare: what a --NAME without a value sets (None: there is no
# such thing); head: the row of --NAME=VALUE (None: VALUE is the side file); side: pg_write_NAME takes a file; strict: an unknown
# --NAME... word is refused (the older analyses let it pass); zero_off: --NAME=0 is no request at all.
_Analysis = collections.namedtuple("_Analysis", "name opt write form bare head side rows strict zero_off", defaults=(False, False))
_M_PERM, _M_INT31, _M_TYPE, _M_METRIC = "must be in [0, 2^31 - 2]", "must be in [0, 2^31 - 1]", "must be gene or adj", "must be jaccard or diff"
_RECON = (_Row("type", "type", extra=True), _Row("metric", "metric", extra=True), _Row("method", "method", extra=True), _Row("gain", "gain", int, extra=True),
          _Row("loss", "loss", int, extra=True), _Row("resolve", "mode", extra=True))  # gainloss, coevo and (without resolve) phylosig: NAME_opt() tests the values

# in the order in which --X refuses the ones before it (after --matrix and --call)
_ANALYSES = (
    _Analysis("curves", curves_opt, "pg_write_curves", "--curves", {"n_perm": 10}, _Row(None, "n_perm", int), False, (_Row("seed", "seed", int),), zero_off=True),
    _Analysis("dist", dist_opt, "pg_write_dist", "--dist", {"type": "gene"}, _words(None, "type", DIST_TYPES, _M_TYPE), False,
              (_words("metric", "metric", DIST_METRICS, "must be jaccard, shared or diff"),)),
    _Analysis("assoc", assoc_opt, "pg_write_assoc", "--assoc", {"min_phi": 0.8}, _Row(None, "min_phi", float, lambda r: 0.0 <= r <= 1.0, "must be in [0, 1]"), False,
              (_Row("min-count", "min_count", int, lambda c: c >= 1, "must be at least 1"), _words("sign", "sign", ASSOC_SIGNS, "must be pos, neg or both"))),
    _Analysis("trait", trait_opt, "pg_write_trait", "--trait=FILE", None, None, True,
              (_ints("perm", "n_perm", 0, TRAIT_MAX_PERM, _M_PERM), _Row("seed", "seed", int),
               _words("lineage", "lineage", TRAIT_LINEAGES[1:], "must be nj or upgma and needs --trait=FILE", needs_head=True))),  # (one message for both)
    _Analysis("tree", tree_opt, "pg_write_tree", "--tree", {"type": "gene"}, _words(None, "type", DIST_TYPES, _M_TYPE), False,
              (_words("metric", "metric", TREE_METRICS, _M_METRIC), _words("method", "method", TREE_METHODS, "must be nj or upgma"),
               _ints("boot", "n_boot", 0, TREE_MAX_BOOT, _M_INT31, phase=1), _Row("seed", "seed", _seed32, phase=1))),
    _Analysis("qtrait", qtrait_opt, "pg_write_qtrait", "--qtrait=FILE", None, None, True, (_ints("perm", "n_perm", 0, TRAIT_MAX_PERM, _M_PERM, extra=True), _Row("seed", "seed", int, extra=True))),
    _Analysis("cluster", cluster_opt, "pg_write_cluster", "--cluster=INT[-INT]", None, _Row(None, ("k_lo", "k_hi"), _k_range), False,
              (_words("type", "type", DIST_TYPES, _M_TYPE, extra=True), _words("metric", "metric", TREE_METRICS, _M_METRIC, extra=True),
               _ints("iter", "max_iter", 0, TREE_MAX_BOOT, _M_INT31, extra=True)), strict=True),
    _Analysis("permanova", permanova_opt, "pg_write_permanova", "--permanova=FILE", None, None, True,
              (_words("type", "type", DIST_TYPES, _M_TYPE, extra=True), _words("metric", "metric", TREE_METRICS, _M_METRIC, extra=True),
               _ints("perm", "n_perm", 0, TRAIT_MAX_PERM, _M_PERM, extra=True), _Row("seed", "seed", int, extra=True)), strict=True),
    _Analysis("mantel", mantel_opt, "pg_write_mantel", "--mantel", {}, None, True,
              (_Row("x", "x", str, _spec_ok, "must be gene|adj:jaccard|diff", extra=True),
               _Row("y", "y", str, _spec_ok, "must be gene|adj:jaccard|diff", extra=True, no_file=True),  # (-y and the file both name the second matrix)
               _ints("perm", "n_perm", 0, TRAIT_MAX_PERM, _M_PERM, extra=True), _Row("seed", "seed", int, extra=True)), strict=True),
    _Analysis("gainloss", gainloss_opt, "pg_write_gainloss", "--gainloss", {}, _Row(None, "out"), False, _RECON + (_Row("min", "min_changes", int, extra=True),), strict=True),
    _Analysis("coevo", coevo_opt, "pg_write_coevo", "--coevo", {}, _Row(None, "min_r", float), False,
              _RECON + (_Row("min", "min_events", int, extra=True), _Row("sign", "sign", extra=True), _Row("max", "max_pair", int, extra=True)), strict=True),
    _Analysis("phylosig", phylosig_opt, "pg_write_phylosig", "--phylosig", {}, _ints(None, "n_perm", 0, TRAIT_MAX_PERM, _M_PERM), False,
              _RECON[:5] + (_Row("seed", "seed", int, extra=True), _Row("min", "min_count", int, extra=True), _Row("max-p", "max_p", float, extra=True)), strict=True),
    _Analysis("pcoa", pcoa_opt, "pg_write_pcoa", "--pcoa", {}, _ints(None, "n_axis", 1, PCOA_MAX_AXIS, "must be in [1, 16]"), False,
              (_words("type", "type", DIST_TYPES, _M_TYPE, extra=True), _words("metric", "metric", TREE_METRICS, _M_METRIC, extra=True), _Row("seed", "seed", int, extra=True)),
              strict=True),
    _Analysis("glm", glm_opt, "pg_write_glm", "--glm=FILE", None, None, True,
              (_words("family", "family", GLM_FAMILIES, "must be binary or quant", extra=True), _ints("axes", "n_axis", 0, GLM_MAX_AXIS, "must be in [0, 13]", extra=True),
               _words("type", "type", DIST_TYPES, _M_TYPE, extra=True), _words("metric", "metric", TREE_METRICS, _M_METRIC, extra=True), _Row("seed", "seed", int, extra=True),
               _Row("min", "min_count", int, extra=True), _Row("max-p", "max_p", float, extra=True)), strict=True),
    _Analysis("rates", rates_opt, "pg_write_rates", "--rates", {}, _Row(None, "out"), False,
              (_Row("type", "type", extra=True), _Row("metric", "metric", extra=True), _Row("method", "method", extra=True), _Row("gain", "gain", float, extra=True),
               _Row("loss", "loss", float, extra=True), _Row("min", "min_changes", float, extra=True)), strict=True),  # rates_opt() tests the values
)
_HEADS = tuple("--" + a.name for a in _ANALYSES)


def _join(words, last):
    return ", ".join(words[:-1]) + last + words[-1] if len(words) > 1 else words[0]


def _one_analysis_args(a: _Analysis, argv: Sequence[str]):
    """(asked for, keywords of NAME_opt(), side file) of --NAME[=VALUE] and the --NAME-suffix=VALUE of one analysis in argv"""
    on, extra, side, no_file, kw = False, False, None, None, {}
    head, rows = "--" + a.name, {"--%s-%s=" % (a.name, r.suffix): r for r in a.rows}

    def put(r, v):
        v = r.conv(v)
        kw.update(zip(r.kw, v) if isinstance(r.kw, tuple) else ((r.kw, v),))

    for phase in range(1 + max(r.phase for r in a.rows)):
        for x in argv:
            r = rows.get(x[:x.find("=") + 1])
            if x == head and a.bare is not None:
                on = True
                if phase == 0: kw.update(a.bare)
            elif x.startswith(head + "="):
                on = True
                if a.head is None: side = x.split("=", 1)[1]
                elif phase == 0: put(a.head, x.split("=", 1)[1])
            elif r is not None:
                if r.phase == phase:
                    put(r, x.split("=", 1)[1])
                    extra, no_file = extra or r.extra, r if r.no_file else no_file
            elif a.strict and x.startswith(head):  # a bare --NAME that needs a value, --NAME-suffix without one, an unknown --NAME... word
                raise ValueError("unknown option or missing value: " + x)
        for r in ((a.head,) if a.head else ()) + a.rows:
            if r.phase == phase and r.ok is not None and r.kw in kw and not (r.ok(kw[r.kw]) and (on or not r.needs_head)):
                raise ValueError("%s%s %s" % (head, "-" + r.suffix if r.suffix else "", r.msg))
    names = [head + "-" + r.suffix for r in a.rows if r.extra]
    if extra and not on:
        raise ValueError("%s %s %s" % (_join(names, " and "), "needs" if len(names) == 1 else "need", a.form))
    if no_file is not None and side is not None:
        raise ValueError("%s-%s cannot be combined with %s=FILE" % (head, no_file.suffix, head))
    if a.zero_off and not kw.get(a.head.kw):
        on = False
    return on, kw, side


def _analysis_args(argv: Sequence[str], lib: C.CDLL | None = None):
    """The analysis argv asks for: (its table entry, the keywords of its NAME_opt(), its side file, NAME_opt(lib, **keywords) when lib is
    given), or None.  Every analysis is read and checked in the table's order, and --X is refused when anything before it was asked for."""
    before = ["--matrix", "--call"]
    any_before = any(x.startswith("--matrix") for x in argv) or "--call" in argv
    found = None
    for a in _ANALYSES:
        on, kw, side = _one_analysis_args(a, argv)
        if on and any_before:
            raise ValueError("--%s cannot be combined with %s" % (a.name, _join(before, " or ")))
        if on:
            found, any_before = (a, kw, side, a.opt(lib, **kw) if lib is not None else None), True
        before.append("--" + a.name)
    return found


def _tree_boot_args(argv: Sequence[str]):
    """(replicates, seed) of --tree-boot=INT / --tree-seed=INT in argv"""
    kw = _one_analysis_args(next(a for a in _ANALYSES if a.name == "tree"), argv)[1]
    return kw.get("n_boot", 0), kw.get("seed", 0)


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
    "pg_rates_opt_init": (None, [C.c_void_p]),
    "pg_rates_file": (C.c_int, [C.c_char_p, C.c_void_p]),
    "pg_write_rates": (None, [C.c_void_p, C.c_void_p]),
    "pg_pan_rates": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                               C.POINTER(C.c_double)]),
    "pg_pan_gainloss": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "pg_coevo_opt_init": (None, [C.c_void_p]),
    "pg_coevo_file": (C.c_int, [C.c_char_p, C.c_void_p]),
    "pg_write_coevo": (None, [C.c_void_p, C.c_void_p]),
    "pg_pan_coevo": (C.c_int64, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int64]),
    "pg_phylosig_opt_init": (None, [C.c_void_p]),
    "pg_phylosig_file": (C.c_int, [C.c_char_p, C.c_void_p]),
    "pg_write_phylosig": (None, [C.c_void_p, C.c_void_p]),
    "pg_pan_phylosig": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "pg_pcoa_opt_init": (None, [C.c_void_p]),
    "pg_pcoa_file": (C.c_int, [C.c_char_p, C.c_void_p]),
    "pg_write_pcoa": (None, [C.c_void_p, C.c_void_p]),
    "pg_pan_pcoa": (C.c_int, [C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                              C.POINTER(C.c_int32)]),
    "pg_pan_pcoa_presence": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "pg_glm_opt_init": (None, [C.c_void_p]),
    "pg_glm_file": (C.c_int, [C.c_char_p, C.c_char_p, C.c_void_p]),
    "pg_write_glm": (None, [C.c_void_p, C.c_char_p, C.c_void_p]),
    "pg_pan_glm": (C.c_int, [C.POINTER(C.c_uint8), C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_void_p,
                             C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
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
        elif a in ("--matrix", "--matrix=presence", "--matrix=count", "--call") or a.startswith(_HEADS): pass  # handled by run()
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
    what = _analysis_args(argv, lib)
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
            elif what is not None:
                a, _, side, o = what
                file_arg = (side.encode() if side is not None else None,) if a.side else ()  # (pg_write_NAME(g, [file,] options))
                getattr(lib, a.write)(g, *file_arg, C.byref(o))
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
