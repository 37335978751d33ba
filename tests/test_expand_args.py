"""Every SLG_ERR_INVALID / SLG_ERR_UNSUPPORTED case of slg_index_set_terms and slg_expand_batch, each leaving
slg_last_error set, and the limits' last good values."""
import ctypes as C

import numpy as np
import pytest

from tests import expand_util as U
from tests import expand_worlds as W


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def last(lib):
    return lib.slg_last_error_code(), lib.slg_last_error()


def test_null_index_fails_cleanly(lib):
    from searchlite_amd import _native as N
    offs = np.zeros(2, np.uint32)
    assert lib.slg_index_set_terms(None, 0, b"a:b", offs.ctypes.data) == N.ERR_INVALID
    assert last(lib) == (N.ERR_INVALID, b"index is NULL")
    assert lib.slg_expand_batch(None, None, 0, offs.ctypes.data, 0, None, None) == N.ERR_INVALID
    assert last(lib) == (N.ERR_INVALID, b"index is NULL")
    assert lib.slg_expand_phase_ms(None, None, None) == N.ERR_INVALID


@pytest.fixture(scope="module")
def ix():
    import searchlite_amd as sa
    keys = ["body:rust", "body:rusk", "body:" + "a" * 128, "title:x"]
    with sa.GpuIndex([W.dict_segment(keys)]) as index:
        index.set_terms(0, keys)
        yield index


SET_TERMS_ERRORS = [
    ("seg out of range", dict(seg=1), b"no such segment"),
    ("NULL bytes", dict(bytes=None), b"key_bytes is NULL"),
    ("NULL offsets", dict(offs=None), b"key_offsets is NULL"),
    ("decreasing offsets", dict(offs=[0, 9, 8, 12, 16]), b"decrease"),
    ("duplicate keys", dict(keys=[b"body:a", b"body:b", b"body:a", b"body:c"]), b"are equal"),
    ("a key without ':'", dict(keys=[b"body:a", b"bodyb", b"body:c", b"body:d"]), b"has no ':'"),
    ("invalid UTF-8", dict(keys=[b"body:a", b"body:\xe9", b"body:c", b"body:d"]), b"not valid UTF-8"),
    ("truncated UTF-8", dict(keys=[b"body:a", b"body:b", b"body:c", b"body:\xf0\x9f\x98"]), b"not valid UTF-8"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(SET_TERMS_ERRORS)), ids=[c[0] for c in SET_TERMS_ERRORS])
def test_set_terms_errors(lib, ix, case):
    from searchlite_amd import _native as N
    _, change, word = SET_TERMS_ERRORS[case]
    blob, offs = U.key_arrays(change.get("keys", [b"body:a", b"body:b", b"body:c", b"body:d"]))
    if "offs" in change:
        offs = None if change["offs"] is None else np.array(change["offs"], np.uint32)
    bp = None if change.get("bytes", 0) is None else blob.ctypes.data
    op = None if offs is None else offs.ctypes.data
    want = ix.expand([U.prefix("body", "r", 5)])
    assert lib.slg_index_set_terms(ix._h, change.get("seg", 0), bp, op) == N.ERR_INVALID
    code, msg = last(lib)
    assert code == N.ERR_INVALID and word in msg
    got = ix.expand([U.prefix("body", "r", 5)])          # the index is as it was
    assert got[0][0].tolist() == want[0][0].tolist() == [[1], [0]]


def call(lib, ix, reqs_ptr, n, offs_ptr, cap, ids_ptr, dist_ptr):
    return lib.slg_expand_batch(ix._h, reqs_ptr, n, offs_ptr, cap, ids_ptr, dist_ptr)


EXPAND_ERRORS = [
    ("struct_size", dict(struct_size=12), "ERR_INVALID", b"struct_size"),
    ("unknown kind", dict(kind=3), "ERR_INVALID", b"unknown kind"),
    ("negative kind", dict(kind=-1), "ERR_INVALID", b"unknown kind"),
    ("NULL term with a length", dict(term=None, term_len=3), "ERR_INVALID", b"term is NULL"),
    ("NULL field with a length", dict(field=None, field_len=3), "ERR_INVALID", b"field is NULL"),
    ("term not UTF-8", dict(term=b"ru\xff"), "ERR_INVALID", b"term is not valid UTF-8"),
    ("field not UTF-8", dict(field=b"\xe4\xba"), "ERR_INVALID", b"field is not valid UTF-8"),
    ("129 chars", dict(term=("é" * 129).encode()), "ERR_UNSUPPORTED", b"SLG_MAX_EXPAND_CHARS"),
    ("129-char pattern", dict(kind=2, term=b"*" * 129), "ERR_UNSUPPORTED", b"SLG_MAX_EXPAND_CHARS"),
    ("max_expansions 1025", dict(max_expansions=1025), "ERR_UNSUPPORTED", b"SLG_MAX_EXPANSIONS"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(EXPAND_ERRORS)), ids=[c[0] for c in EXPAND_ERRORS])
def test_expand_request_errors(lib, ix, case):
    from searchlite_amd import _native as N
    _, change, code, word = EXPAND_ERRORS[case]
    keep = []
    reqs = (N.ExpandReq * 2)(U.c_req(U.fuzzy("body", "rust"), keep), U.c_req(U.fuzzy("body", "rusk"), keep))
    for k, v in change.items():
        setattr(reqs[1], k, v)
        if k in ("term", "field") and v is not None:
            setattr(reqs[1], k + "_len", len(v))
    offs = np.zeros(3, np.uint32)
    assert call(lib, ix, reqs, 2, offs.ctypes.data, 0, None, None) == getattr(N, code)
    got_code, msg = last(lib)
    assert got_code == getattr(N, code) and word in msg and b"request 1" in msg


@pytest.mark.gpu
def test_expand_call_errors_and_the_size_query(lib, ix):
    from searchlite_amd import _native as N
    keep = []
    reqs = (N.ExpandReq * 1)(U.c_req(U.fuzzy("body", "rust"), keep))
    offs, ids, dist = np.zeros(2, np.uint32), np.zeros((4, 1), np.uint32), np.zeros(4, np.uint8)
    assert call(lib, ix, reqs, 1, None, 0, None, None) == N.ERR_INVALID and b"out_offsets" in last(lib)[1]
    assert call(lib, ix, None, 1, offs.ctypes.data, 0, None, None) == N.ERR_INVALID and b"reqs is NULL" in last(lib)[1]
    assert call(lib, ix, reqs, 1, offs.ctypes.data, 4, ids.ctypes.data, None) == N.ERR_INVALID and b"both" in last(lib)[1]
    assert call(lib, ix, reqs, 1, offs.ctypes.data, 4, None, dist.ctypes.data) == N.ERR_INVALID and b"both" in last(lib)[1]
    assert call(lib, ix, reqs, 1, offs.ctypes.data, 0, None, None) == N.OK and offs.tolist() == [0, 2]   # the size query
    assert call(lib, ix, reqs, 1, offs.ctypes.data, 1, ids.ctypes.data, dist.ctypes.data) == N.ERR_INVALID
    assert last(lib)[0] == N.ERR_INVALID and b"key_capacity" in last(lib)[1]
    assert call(lib, ix, reqs, 1, offs.ctypes.data, 2, ids.ctypes.data, dist.ctypes.data) == N.OK
    assert ids[:2, 0].tolist() == [0, 1] and dist[:2].tolist() == [0, 1] and last(lib) == (N.OK, b"")
    assert call(lib, ix, None, 0, offs.ctypes.data, 0, None, None) == N.OK and offs[0] == 0              # no requests


@pytest.mark.gpu
def test_the_limits_last_good_values_and_embedded_nul(ix):
    """128 chars and max_expansions 1024 are taken; the strings carry lengths, so a NUL is a byte like any other"""
    got = ix.expand([U.fuzzy("body", "a" * 127 + "b", 1, 1, 1024, 3), U.wildcard("body", "a" * 127 + "?", 1024),
                     dict(U.fuzzy("body", "ru\0t", 1, 1, 50, 3)), dict(U.prefix("bo\0dy", "", 5))])
    assert got[0][0].tolist() == [[0xFFFFFFFF], [2]] and got[0][1].tolist() == [0, 1]
    assert got[1][0].tolist() == [[2]]
    assert got[2][0].tolist() == [[0xFFFFFFFF], [0]] and got[2][1].tolist() == [0, 1]    # "ru\0t" is one edit from "rust"
    assert got[3][0].tolist() == []
