"""What the expansion tests share: the host side of term expansion through its test C ABI (lib/libslg_plan.so,
csrc/slg_expand_capi.cpp), requests as the library takes them, and hand-made device rows (what the scan owes
the host merge: per segment the first R passing keys of the request's range, in dictionary order) computed with
tests/expand_ref.py's own predicates."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from searchlite_amd import _native as N
from tests import expand_ref as R

FUZZY, PREFIX, WILDCARD = N.EXPAND_FUZZY, N.EXPAND_PREFIX, N.EXPAND_WILDCARD


def fuzzy(field, term, max_edits=1, prefix_length=1, max_expansions=50, min_length=3):
    return dict(kind=FUZZY, field=field, term=term, max_expansions=max_expansions, max_edits=max_edits,
                prefix_length=prefix_length, min_length=min_length)


def prefix(field, term, max_expansions=50):
    return dict(kind=PREFIX, field=field, term=term, max_expansions=max_expansions, max_edits=0, prefix_length=0,
                min_length=0)


def wildcard(field, term, max_expansions=50):
    return dict(kind=WILDCARD, field=field, term=term, max_expansions=max_expansions, max_edits=0, prefix_length=0,
                min_length=0)


def c_req(req: dict, keep: list) -> "N.ExpandReq":
    f, t = req["field"].encode("utf-8"), req["term"].encode("utf-8")
    keep += [f, t]
    return N.ExpandReq(C.sizeof(N.ExpandReq), req["kind"], f, t, len(f), len(t), req["max_expansions"],
                       req["max_edits"], req["prefix_length"], req["min_length"])


_lib = None


def host_lib():
    global _lib
    if _lib is None:
        from searchlite_amd import build
        L = C.CDLL(build.build_plan_lib())
        vp, u32 = C.c_void_p, C.c_uint32
        L.slgx_dict_build.restype = vp
        L.slgx_dict_build.argtypes = [u32, vp, vp, C.c_char_p, u32, vp]
        L.slgx_dict_free.restype = None
        L.slgx_dict_free.argtypes = [vp]
        L.slgx_dict_tables.restype = u32
        L.slgx_dict_tables.argtypes = [vp, vp, vp]
        L.slgx_prefix_range.restype = None
        L.slgx_prefix_range.argtypes = [vp, C.c_char_p, u32, vp, vp]
        L.slgx_check_request.restype = C.c_int
        L.slgx_check_request.argtypes = [vp, vp, vp, vp, u32, vp, C.c_char_p, u32]
        L.slgx_rows_needed.restype = u32
        L.slgx_rows_needed.argtypes = [vp, u32]
        L.slgx_merge.restype = C.c_int
        L.slgx_merge.argtypes = [vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, C.c_char_p, u32]
        L.slgx_banded_distance.restype = u32
        L.slgx_banded_distance.argtypes = [vp, u32, C.c_char_p, u32, u32]
        L.slgx_glob_match.restype = C.c_int
        L.slgx_glob_match.argtypes = [vp, u32, C.c_char_p, u32]
        L.slgx_reference_expand.restype = C.c_int
        L.slgx_reference_expand.argtypes = [vp, u32, vp, u32, u32, vp, u32, vp, vp, C.c_char_p, u32]
        _lib = L
    return _lib


def key_arrays(keys):
    raw = [k.encode("utf-8") if isinstance(k, str) else k for k in keys]
    offs = np.zeros(len(raw) + 1, dtype=np.uint32)
    np.cumsum([len(r) for r in raw], out=offs[1:])
    return np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8), offs


class HostDict:
    """a segment's dictionary built by the library's host code from keys in term-id order"""

    def __init__(self, keys):
        L = host_lib()
        blob, offs = key_arrays(keys)
        self.err = C.create_string_buffer(256)
        self.code = C.c_int(0)
        self.h = L.slgx_dict_build(len(keys), blob.ctypes.data, offs.ctypes.data, self.err, 256, C.addressof(self.code))
        self.keys = list(keys)
        if self.h:
            self.map = np.zeros(len(keys), dtype=np.uint32)
            self.nchars = np.zeros(len(keys), dtype=np.uint8)
            L.slgx_dict_tables(self.h, self.map.ctypes.data, self.nchars.ctypes.data)

    def __del__(self):
        if getattr(self, "h", None):
            host_lib().slgx_dict_free(self.h)
            self.h = None


def passes(req: dict, key: str):
    """the request's predicate on a key of its range -> distance, or None (tests/expand_ref.py's own pieces)"""
    field, term = req["field"], req["term"]
    if len(key) <= len(field) + 1:
        return None
    cand = key[len(field) + 1:]
    if req["kind"] == PREFIX:
        return 0
    if req["kind"] == WILDCARD:
        return 0 if R.build_wildcard_regex(term).fullmatch(cand) is not None else None
    me = min(req["max_edits"], 2)
    if cand == term or abs(len(cand) - len(term)) > me:
        return None
    d = R.bounded_levenshtein(term, cand, me)
    return d if d else None


def range_key(req: dict) -> str:
    term = req["term"]
    if req["kind"] == FUZZY:
        term = term[:min(req["prefix_length"], len(term))]
    elif req["kind"] == WILDCARD:
        term = re.split(r"[*?]", term)[0]
    return req["field"] + ":" + term


def scans(req: dict) -> bool:
    if req["kind"] == FUZZY:
        return len(req["term"]) >= req["min_length"] and req["max_expansions"] > 0 and min(req["max_edits"], 2) > 0
    return req["max_expansions"] > 0


def device_rows(seg_sorted_keys, req: dict):
    """per segment (positions, distances) of the first R passing keys of the range, R as the library states it"""
    L = host_lib()
    keep = []
    cr = c_req(req, keep)
    out = []
    for s, keys in enumerate(seg_sorted_keys):
        need = L.slgx_rows_needed(C.addressof(cr), s) if scans(req) else 0
        pos, dist = [], []
        pre = range_key(req)
        for i, k in enumerate(keys):
            if len(pos) >= need:
                break
            if not k.startswith(pre):
                continue
            d = passes(req, k)
            if d is not None:
                pos.append(i)
                dist.append(d)
        out.append((pos, dist))
    return out


def host_merge(req: dict, dicts, rows):
    """slgx_merge -> (term ids [n, n_segs], distances [n])"""
    L = host_lib()
    keep = []
    cr = c_req(req, keep)
    n_segs = len(dicts)
    offs = np.zeros(n_segs + 1, dtype=np.uint32)
    np.cumsum([len(p) for p, _ in rows], out=offs[1:])
    pos = np.array([x for p, _ in rows for x in p] + [0], dtype=np.uint32)
    dist = np.array([x for _, d in rows for x in d] + [0], dtype=np.uint8)
    hs = (C.c_void_p * n_segs)(*[d.h for d in dicts])
    cap = 4096
    ids = np.zeros((cap, n_segs), dtype=np.uint32)
    od = np.zeros(cap, dtype=np.uint8)
    n = C.c_uint32(0)
    err = C.create_string_buffer(256)
    rc = L.slgx_merge(C.addressof(cr), hs, n_segs, offs.ctypes.data, pos.ctypes.data, dist.ctypes.data, cap,
                      ids.ctypes.data, od.ctypes.data, C.addressof(n), err, 256)
    assert rc == 0, err.value
    return ids[:n.value].copy(), od[:n.value].copy()


def reference_loop(reqs, dicts, n_threads=1):
    """slgx_reference_expand (the C++ restatement of the reference's loop) -> per request (ids, distances)"""
    L = host_lib()
    keep = []
    arr = (N.ExpandReq * max(len(reqs), 1))(*[c_req(r, keep) for r in reqs])
    n_segs = len(dicts)
    hs = (C.c_void_p * n_segs)(*[d.h for d in dicts])
    offs = np.zeros(len(reqs) + 1, dtype=np.uint32)
    cap = 1 << 16
    ids = np.zeros((cap, n_segs), dtype=np.uint32)
    od = np.zeros(cap, dtype=np.uint8)
    err = C.create_string_buffer(256)
    rc = L.slgx_reference_expand(hs, n_segs, arr, len(reqs), n_threads, offs.ctypes.data, cap, ids.ctypes.data,
                                 od.ctypes.data, err, 256)
    assert rc == 0, err.value
    return [(ids[offs[i]:offs[i + 1]].copy(), od[offs[i]:offs[i + 1]].copy()) for i in range(len(reqs))]


class World:
    """segments given as lists of keys in TERM-ID order (any order); the reference sees them byte-sorted"""

    def __init__(self, seg_keys):
        self.seg_keys = [list(k) for k in seg_keys]
        self.sorted = [R.sorted_keys(k) for k in self.seg_keys]
        self.ids = [{k: i for i, k in enumerate(keys)} for keys in self.seg_keys]

    def want(self, req: dict):
        """(term ids, distances) as tests/expand_ref.py expands the request"""
        return R.term_rows(self.ids, R.expand(self.sorted, req))
