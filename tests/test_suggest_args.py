"""Every SLG_ERR_INVALID / SLG_ERR_UNSUPPORTED case of slg_suggest_batch, each with its error text, and the limits'
last good values.  The request checks are one function (csrc/slg_suggest_host.cpp), reached here without a device
through the test ABI and, in the tests marked gpu, through slg_suggest_batch itself with slg_last_error set."""

import numpy as np
import pytest

from searchlite_amd import _native as N
from searchlite_amd.searcher import suggest_request as req
from tests import suggest_worlds as W

FZ = dict(max_edits=1, prefix_length=1, max_expansions=50, min_length=3)

REQUEST_ERRORS = [
    ("struct_size", dict(struct_size=12), "ERR_INVALID", b"struct_size"),
    ("NULL term with a length", dict(term=None, term_len=3), "ERR_INVALID", b"term is NULL"),
    ("NULL field with a length", dict(field=None, field_len=3), "ERR_INVALID", b"field is NULL"),
    ("term not UTF-8", dict(term=b"ru\xff"), "ERR_INVALID", b"term is not valid UTF-8"),
    ("field not UTF-8", dict(field=b"\xe4\xba"), "ERR_INVALID", b"field is not valid UTF-8"),
    ("129 chars", dict(term=("é" * 129).encode()), "ERR_UNSUPPORTED", b"SLG_MAX_EXPAND_CHARS"),
    ("fuzzy size 257", dict(size=257), "ERR_UNSUPPORTED", b"SLG_MAX_SUGGEST_CANDIDATES"),
]
IDS = [c[0] for c in REQUEST_ERRORS]


@pytest.fixture(scope="module")
def lib():
    return N.load()


def last(lib):
    return lib.slg_last_error_code(), lib.slg_last_error()


def test_null_index_fails_cleanly(lib):
    offs = np.zeros(3, np.uint32)
    assert lib.slg_suggest_batch(None, None, 0, offs.ctypes.data, 0, None, None, None, 0, None) == N.ERR_INVALID
    assert last(lib) == (N.ERR_INVALID, b"index is NULL")
    assert lib.slg_suggest_phase_ms(None, None, None) == N.ERR_INVALID


@pytest.mark.parametrize("case", range(len(REQUEST_ERRORS)), ids=IDS)
def test_request_checks_on_the_host(case):
    _, change, code, word = REQUEST_ERRORS[case]
    keep = []
    rc, msg, _ = W.check(W.c_req(req("body", "rust", 5, FZ), keep, **change))
    assert rc == getattr(N, code) and word in msg and b"suggest: request 0" in msg


def test_what_a_good_request_derives():
    keep = []
    ok = lambda r, **ch: W.check(W.c_req(r, keep, **ch))
    rc, _, d = ok(req("body", "rust", 5, FZ))
    assert rc == N.OK and d == dict(scan=1, fuzzy=1, cap=50, max_edits=1, range_key=b"body:r")
    assert ok(req("body", "éa", 5, dict(FZ, prefix_length=1, min_length=0)))[2]["range_key"] == "body:é".encode()
    assert ok(req("body", "rust", 5, dict(FZ, prefix_length=9, max_edits=3)))[2] == \
        dict(scan=1, fuzzy=1, cap=50, max_edits=2, range_key=b"body:rust")
    assert ok(req("body", "rust", 256, dict(FZ, max_expansions=300)))[2]["cap"] == 256          # the last good size
    assert ok(req("body", "rust", 60, FZ))[2]["cap"] == 60 and ok(req("body", "rust", 5, dict(FZ, max_expansions=2)))[2]["cap"] == 5
    for off in (dict(max_edits=0), dict(max_expansions=0), dict(min_length=5)):
        assert ok(req("body", "rust", 5, dict(FZ, **off)))[2]["scan"] == 0
    assert ok(req("body", "rust", 0, FZ))[2]["scan"] == 0 and ok(req("body", "rust", 0))[2]["scan"] == 0
    for size, cap in ((1, 64), (12, 64), (13, 65), (51, 255), (52, 256), (300, 256), (0xFFFFFFFF, 256)):
        rc, _, d = ok(req("body", "ru", size))                       # a plain request may have any size
        assert rc == N.OK and d == dict(scan=1, fuzzy=0, cap=cap, max_edits=0, range_key=b"body:ru")
    assert ok(req("body", "a" * 128, 5))[0] == N.OK and ok(req("bo\0dy", "r\0", 5))[2]["range_key"] == b"bo\0dy:r\0"
    assert ok(req("", "", 5))[2]["range_key"] == b":"


# ---- through slg_suggest_batch ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ix():
    import searchlite_amd as sa
    keys = [("body:rust", 2), ("body:rusk", 1), ("body:" + "a" * 128, 1), ("title:x", 1)]
    with sa.GpuIndex([W.df_segment(keys)]) as index:
        index.set_terms_from_segments()
        yield index


def call(lib, ix, reqs, n, offs, cap=0, score=None, df=None, toffs=None, tcap=0, text=None):
    p = lambda a: None if a is None else a.ctypes.data
    return lib.slg_suggest_batch(ix._h, reqs, n, p(offs), cap, p(score), p(df), p(toffs), tcap, p(text))


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(REQUEST_ERRORS)), ids=IDS)
def test_suggest_request_errors(lib, ix, case):
    _, change, code, word = REQUEST_ERRORS[case]
    keep = []
    reqs = (N.SuggestReq * 2)(W.c_req(req("body", "rust", 5, FZ), keep), W.c_req(req("body", "rusk", 5, FZ), keep, **change))
    offs = np.zeros(4, np.uint32)
    assert call(lib, ix, reqs, 2, offs) == getattr(N, code)
    got_code, msg = last(lib)
    assert got_code == getattr(N, code) and word in msg and b"request 1" in msg


@pytest.mark.gpu
def test_suggest_call_errors_and_the_size_query(lib, ix):
    keep = []
    reqs = (N.SuggestReq * 1)(W.c_req(req("body", "rus", 5), keep))
    offs, score, df = np.zeros(3, np.uint32), np.zeros(4, np.float32), np.zeros(4, np.uint64)
    toffs, text = np.zeros(5, np.uint32), np.zeros(16, np.uint8)
    assert call(lib, ix, reqs, 1, None) == N.ERR_INVALID and b"out_offsets" in last(lib)[1]
    assert call(lib, ix, None, 1, offs) == N.ERR_INVALID and b"reqs is NULL" in last(lib)[1]
    arrays = dict(score=score, df=df, toffs=toffs, text=text)
    for missing in arrays:                                            # some but not all output arrays
        some = dict(arrays, **{missing: None})
        assert call(lib, ix, reqs, 1, offs, 4, tcap=16, **some) == N.ERR_INVALID and b"all NULL" in last(lib)[1], missing
    assert call(lib, ix, reqs, 1, offs) == N.OK and offs.tolist() == [0, 2, 8]      # the size query: 2 options, 8 bytes
    assert call(lib, ix, reqs, 1, offs, 1, score, df, toffs, 16, text) == N.ERR_INVALID
    assert last(lib)[0] == N.ERR_INVALID and b"option_capacity" in last(lib)[1]
    assert call(lib, ix, reqs, 1, offs, 2, score, df, toffs, 7, text) == N.ERR_INVALID
    assert last(lib)[0] == N.ERR_INVALID and b"text_capacity" in last(lib)[1]
    assert call(lib, ix, reqs, 1, offs, 2, score, df, toffs, 8, text) == N.OK and last(lib) == (N.OK, b"")
    assert offs[:2].tolist() == [0, 2] and toffs[:3].tolist() == [0, 4, 8] and text[:8].tobytes() == b"rustrusk"
    assert score[:2].tolist() == [2.0, 1.0] and df[:2].tolist() == [2, 1]
    assert call(lib, ix, None, 0, offs) == N.OK and offs[:2].tolist() == [0, 0]     # no requests


@pytest.mark.gpu
def test_the_limits_last_good_values_and_embedded_nul(ix):
    got = ix.suggest([req("body", "a" * 127 + "b", 256, dict(FZ, max_expansions=1024)), req("body", "a" * 128, 0xFFFFFFFF),
                      req("body", "ru\0t", 5, FZ), req("bo\0dy", "", 5)])
    assert got[0] == [("a" * 128, np.float32(0.5), 1)] and got[1] == [("a" * 128, np.float32(1.0), 1)]
    assert got[2] == [("rust", np.float32(1.0), 2)] and got[3] == []


@pytest.mark.gpu
def test_a_segment_without_a_dictionary(lib):
    import searchlite_amd as sa
    with sa.GpuIndex([W.df_segment([("body:rust", 2)])]) as index:
        with pytest.raises(N.SlgError) as e:
            index.suggest([req("body", "r", 5)])
        assert e.value.code == N.ERR_INVALID and "has no term dictionary" in str(e.value)
