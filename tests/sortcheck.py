"""ctypes binding of ksql_amd/libkhip_sortcheck.so (tools/sort_check.hip): test-only entry points
for the sort / scan / run-length primitives of ksql_amd/csrc/khip_sort.hpp, which have no entry in
the ABI.  Used by test_gpu_sort.py only."""
import ctypes
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "ksql_amd", "libkhip_sortcheck.so")

E_GUARD, E_INPUT = 100, 101  # sort_check.hip: a guard byte changed / a read-only input changed
FILL = 0xA5                  # what the helper leaves where the primitive did not write
TILE = 8192                  # pairs per sort tile, both tile shapes (1024 x 8, 512 x 16)
SORT_HEAD = 8 * 256 * 4 + 64  # sort_run's scratch: histograms + tickets, then passes x tiles x 256 x 8 B

SCAN_TYPES = {"int64": (0, np.int64), "int32": (1, np.int32), "uint32": (2, np.uint32)}

_dll = None


def load():
    """The helper library; a missing one fails the calling test (no skip)."""
    global _dll
    if _dll is None:
        if not os.path.exists(LIB):
            pytest.fail("%s is missing: build it with `make -C ksql_amd sortcheck` (or build())" % LIB)
        d = ctypes.CDLL(LIB)
        vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
        d.khip_sortcheck_sort.argtypes = [i32, i32, vp, vp, i64, i32, vp, vp, vp]
        d.khip_sortcheck_scan.argtypes = [i32, vp, i64, i32, i32, i32, vp, vp]
        d.khip_sortcheck_rle.argtypes = [vp, i64, vp, vp, vp, vp, vp]
        for f in (d.khip_sortcheck_sort, d.khip_sortcheck_scan, d.khip_sortcheck_rle):
            f.restype = i32
        d.khip_last_error.restype = ctypes.c_char_p
        _dll = d
    return _dll


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _check(rc, what):
    if rc:
        kind = {E_GUARD: "out-of-range store", E_INPUT: "input modified"}.get(rc, "status %d" % rc)
        raise AssertionError("%s: %s: %s" % (what, kind, load().khip_last_error().decode()))


def sort(cfg, keys, vals, end_bit):
    """(sorted keys, sorted values, pass count, third buffer used)."""
    keys = np.ascontiguousarray(keys, np.uint64)
    assert vals.dtype in (np.uint32, np.uint64) and vals.flags.c_contiguous and len(vals) == len(keys)
    n = len(keys)
    ko, vo = np.empty_like(keys), np.empty_like(vals)
    info = np.zeros(2, np.int64)
    _check(load().khip_sortcheck_sort(cfg, vals.dtype.itemsize, _ptr(keys), _ptr(vals), n, end_bit, _ptr(ko), _ptr(vo),
                                      _ptr(info)), "sort cfg=%d n=%d end_bit=%d" % (cfg, n, end_bit))
    tiles = -(-n // TILE)
    status_bytes = int(info[0]) - SORT_HEAD
    assert status_bytes > 0 and status_bytes % (tiles * 256 * 8) == 0, info
    return ko, vo, status_bytes // (tiles * 256 * 8), bool(info[1])


def scan(kind, x, with_total, alias, want_host):
    """(out[0..n (+1)], the host total or None)."""
    code, dt = SCAN_TYPES[kind]
    x = np.ascontiguousarray(x, dt)
    n = len(x)
    out = np.empty(n + (1 if with_total else 0), dt)
    unset = -0x5A5A5A5A5A5A5A5A
    total = np.array([unset], np.int64)
    _check(load().khip_sortcheck_scan(code, _ptr(x), n, int(with_total), int(alias), int(want_host), _ptr(out),
                                      _ptr(total)),
           "scan %s n=%d with_total=%d alias=%d host=%d" % (kind, n, with_total, alias, want_host))
    if not want_host:
        assert total[0] == unset, "total_host written without being asked for"
        return out, None
    return out, int(total[0])


def rle(keys):
    """dict(ukeys[n], cnt[n], start[n + 1], nseg_dev, nseg_host); unwritten entries keep FILL bytes."""
    keys = np.ascontiguousarray(keys, np.uint64)
    n = len(keys)
    uk, cnt, start = np.empty(n, np.uint64), np.empty(n, np.int32), np.empty(n + 1, np.int64)
    nd, nh = np.zeros(1, np.int32), np.zeros(1, np.int64)
    _check(load().khip_sortcheck_rle(_ptr(keys), n, _ptr(uk), _ptr(cnt), _ptr(start), _ptr(nd), _ptr(nh)),
           "rle n=%d" % n)
    return dict(ukeys=uk, cnt=cnt, start=start, nseg_dev=int(nd[0]), nseg_host=int(nh[0]))
