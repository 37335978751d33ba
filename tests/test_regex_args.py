"""Every SLG_ERR_INVALID / SLG_ERR_UNSUPPORTED case of a regex request (include/searchlite_gpu.h, "REGEX"), one
parametrised case each: through slgx_check_request on the CPU and through slg_expand_batch on the device, each
leaving a message that names the request and the construct, each also with max_expansions = 0 (the reference's
planner compiles the pattern before anything else, query/planner.rs:599).  Kind 3 stays an unknown kind."""
import ctypes as C

import numpy as np
import pytest

from searchlite_amd import _native as N
from tests import expand_util as U
from tests import expand_worlds as W
from tests import regex_ref as RR
from tests import regex_util as X

CASES = [(p, w, "ERR_INVALID") for p, w in X.INVALID] + [(p, w, "ERR_UNSUPPORTED") for p, w in X.UNSUPPORTED]
IDS = [f"{code[4:].lower()}-{i}-{p[:16]!r}" for i, (p, _, code) in enumerate(CASES)]


def check(req):
    keep = []
    cr = U.c_req(req, keep)
    scan, me, rl = C.c_uint32(9), C.c_uint32(9), C.c_uint32(0)
    key, err = C.create_string_buffer(1024), C.create_string_buffer(512)
    rc = U.host_lib().slgx_check_request(C.addressof(cr), C.addressof(scan), C.addressof(me), key, 1024, C.addressof(rl), err, 512)
    return rc, err.value.decode("utf-8", "replace")


def test_the_cases_cover_the_headers_lists():
    words = " ".join(w for _, w, _ in CASES)
    for must in (r"\d", r"\D", r"\w", r"\W", r"\s", r"\S", r"\p", r"\P", r"\b", r"\B", r"\x", r"\u", "flag group", "'[' inside a class",
                 "'&&'", "'--'", "'~~'", "{,m}", "quantifier applied to a quantifier", "SLG_MAX_REGEX_STATES", "unbalanced '('",
                 "unbalanced ')'", "unclosed '['", "reversed range", "nothing to repeat", "'{'", "n > m", "trailing lone"):
        assert must in words, must
    for flag in ("(?i)a", "(?s).", "(?x)a b", "(?-u)a"):
        assert flag in [p for p, _, _ in CASES]
    for stacked in ("a**", "a+*", "a{2}{3}", "a?+"):
        assert stacked in [p for p, _, _ in CASES]


@pytest.mark.parametrize("pattern,word,code", CASES, ids=IDS)
def test_refusal_on_the_host(pattern, word, code):
    for mx in (50, 0):
        rc, msg = check(X.regex("body", pattern, mx))
        assert rc == getattr(N, code), (mx, msg)
        assert "request 0" in msg and "regex" in msg and word in msg, msg
        assert "at byte" in msg or "SLG_MAX_REGEX" in msg, msg
    # the restatement's tokenizer sorts the pattern the same way (the DFA's size is not its business)
    if "SLG_MAX_REGEX" not in word and "nested deeper" not in word:
        assert RR.classify(pattern) == (RR.INVALID if code == "ERR_INVALID" else RR.UNSUPPORTED)


def test_a_table_above_the_limit_is_unsupported_on_the_host():
    # (127 distinct literals are more than SLG_MAX_EXPAND_CHARS once escaped; 64 and a count are not)
    p = "".join(chr(ord("0") + i) for i in range(10)) + "".join(chr(ord("A") + i) for i in range(26)) + \
        "".join(chr(ord("a") + i) for i in range(26)) + "_-" + "{192}"
    rc, msg = check(X.regex("body", p))
    assert rc == N.ERR_UNSUPPORTED and "request 0" in msg and "SLG_MAX_REGEX_STATES" in msg
    p = p[:64] + "{190}"                                         # 255 states x 65 classes
    d = X.Dfa(p)
    assert d.code == N.ERR_UNSUPPORTED and "SLG_MAX_REGEX_TABLE" in d.msg, (d.msg, d.n_states, d.n_classes)
    rc, msg = check(X.regex("body", p))
    assert rc == N.ERR_UNSUPPORTED and "request 0" in msg and "SLG_MAX_REGEX_TABLE" in msg and len(p) <= N.MAX_EXPAND_CHARS


def test_kind_3_is_still_an_unknown_kind_on_the_host():
    rc, msg = check(dict(X.regex("body", "a"), kind=3))
    assert rc == N.ERR_INVALID and "unknown kind 3" in msg
    assert check(X.regex("body", "a"))[0] == N.OK and N.EXPAND_REGEX == 4


# ---- through slg_expand_batch ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return N.load()


@pytest.fixture(scope="module")
def ix():
    import searchlite_amd as sa
    keys = ["body:rust", "body:rusk", "title:x"]
    with sa.GpuIndex([W.dict_segment(keys)]) as index:
        index.set_terms(0, keys)
        yield index


def batch(lib, ix, second):
    keep = []
    reqs = (N.ExpandReq * 2)(U.c_req(X.regex("body", "rus."), keep), U.c_req(second, keep))
    offs = np.zeros(3, np.uint32)
    rc = lib.slg_expand_batch(ix._h, reqs, 2, offs.ctypes.data, 0, None, None)
    return rc, lib.slg_last_error_code(), lib.slg_last_error().decode("utf-8", "replace"), offs


@pytest.mark.gpu
@pytest.mark.parametrize("pattern,word,code", CASES, ids=IDS)
def test_refusal_through_the_batch(lib, ix, pattern, word, code):
    for mx in (50, 0):
        rc, last, msg, _ = batch(lib, ix, X.regex("body", pattern, mx))
        assert rc == last == getattr(N, code), (mx, msg)
        assert "request 1" in msg and word in msg, msg


@pytest.mark.gpu
def test_a_large_batch_reports_its_first_bad_request(lib, ix):
    """a batch with many regex requests is checked on several threads: the error is still the lowest request's"""
    keep = []
    reqs = [X.regex("body", "ru[a-z]%d*" % i) for i in range(120)]
    reqs[70], reqs[75], reqs[119] = X.regex("body", "(a", 0), X.regex("body", r"\d"), dict(X.regex("body", "a"), kind=3)
    arr = (N.ExpandReq * len(reqs))(*[U.c_req(r, keep) for r in reqs])
    offs = np.zeros(len(reqs) + 1, np.uint32)
    for _ in range(3):
        assert lib.slg_expand_batch(ix._h, arr, len(reqs), offs.ctypes.data, 0, None, None) == N.ERR_INVALID
        msg = lib.slg_last_error().decode()
        assert "request 70:" in msg and "unbalanced '('" in msg
    arr[70] = U.c_req(X.regex("body", "rus[kt]"), keep)
    assert lib.slg_expand_batch(ix._h, arr, len(reqs), offs.ctypes.data, 0, None, None) == N.ERR_UNSUPPORTED
    assert "request 75:" in lib.slg_last_error().decode() and r"\d" in lib.slg_last_error().decode()
    arr[75] = U.c_req(X.regex("body", "rus[kt]"), keep)
    assert lib.slg_expand_batch(ix._h, arr, len(reqs), offs.ctypes.data, 0, None, None) == N.ERR_INVALID
    assert "request 119:" in lib.slg_last_error().decode() and "unknown kind" in lib.slg_last_error().decode()
    arr[119] = U.c_req(X.regex("body", "rus."), keep)
    assert lib.slg_expand_batch(ix._h, arr, len(reqs), offs.ctypes.data, 0, None, None) == N.OK
    assert offs[70] + 2 == offs[71] and offs[75] + 2 == offs[76] and offs[120] == 6 and offs[119] == 4


@pytest.mark.gpu
def test_kind_3_is_still_an_unknown_kind_and_a_good_batch_passes(lib, ix):
    rc, last, msg, _ = batch(lib, ix, dict(X.regex("body", "a"), kind=3))
    assert rc == last == N.ERR_INVALID and "unknown kind" in msg and "request 1" in msg
    rc, last, msg, offs = batch(lib, ix, X.regex("body", "ru(st|sk)", 1))
    assert (rc, last, msg) == (N.OK, N.OK, "") and offs.tolist() == [0, 2, 3]
