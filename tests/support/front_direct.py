"""TEST INFRASTRUCTURE: k_post_count + k_post_rep of the HIP backend (pga_selftest_post_rep, pga_host_selftest.hpp) on given protein sums,
for tests/test_front_gpu.py: what pga_post_front leaves for k_post_apply and for the host."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from pangene_amd import capi  # noqa: E402

_lib = None


def post_rep(sums, max_ori, prot_gid, Q, min_cnt, joint_pseudo, drop_sgl_exon):
    """-> dict: tie (the flag word), max_ori, n, avg (per protein, the host's words), rep_pid (per gene, -1: none), rep, pj (per protein, the
    bytes k_post_apply reads))"""
    global _lib
    if _lib is None:
        _lib = C.CDLL(capi.LIB_HIP)
        _lib.pga_selftest_post_rep.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                               C.c_void_p, C.c_void_p, C.c_void_p]
    sums = np.ascontiguousarray(sums, dtype=np.int64)
    P = sums.shape[1]
    max_ori, prot_gid = np.ascontiguousarray(max_ori, dtype=np.int32), np.ascontiguousarray(prot_gid, dtype=np.int32)
    words = np.full(16 + 3 * P + Q, 0x5a5a5a5a, dtype=np.int32)
    rep, pj = np.full(P, 0x5a, np.uint8), np.full(P, 0x5a, np.uint8)
    rc = _lib.pga_selftest_post_rep(sums.ctypes.data, max_ori.ctypes.data, prot_gid.ctypes.data, P, Q, float(min_cnt), int(joint_pseudo), int(drop_sgl_exon),
                                    words.ctypes.data, rep.ctypes.data, pj.ctypes.data)
    assert rc == 0, rc
    assert not words[1:16].any()
    return {"tie": int(words[0]), "max_ori": words[16:16 + P], "n": words[16 + P:16 + 2 * P], "avg": words[16 + 2 * P:16 + 3 * P], "rep_pid": words[16 + 3 * P:],
            "rep": rep, "pj": pj}
