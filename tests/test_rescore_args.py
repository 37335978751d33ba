"""slg_batch_prepare_rescore / slg_batch_fetch_rescore / slg_search_batch_rescore argument checks that need no
device: the spec is checked before the index is looked at, a NULL index fails with SLG_ERR_INVALID and a
message, before anything touches a GPU; the header, the ctypes binding and the Rust mirror agree on the
argument counts and the spec's fields."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"slg_batch_prepare_rescore": 10, "slg_batch_fetch_rescore": 4, "slg_search_batch_rescore": 17}


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def spec_of(nq=2, n_terms=2, **over):
    """a well-formed spec of nq queries with n_terms terms each over one segment; over: fields replaced (None:
    a NULL pointer) -> (N.RescoreSpec, the arrays it points into)"""
    from searchlite_amd import _native as N
    a = dict(q_offsets=(np.arange(nq + 1) * n_terms).astype(np.uint32),
             q_term_ids=np.zeros(nq * n_terms, np.uint32), q_weights=np.ones(nq * n_terms, np.float32),
             q_leaf=None, q_plan=None, q_tie=None, q_nleaves=None, q_min_match=None,
             q_window=np.full(nq, 10, np.uint32), q_mode=None)
    a.update(over)
    return N.RescoreSpec(*[None if a[n] is None else a[n].ctypes.data for n, _ in N.RescoreSpec._fields_]), a


def prepare(lib, spec, nq=2, k=11):
    offs = np.zeros(nq + 1, np.uint32)
    return lib.slg_batch_prepare_rescore(None, nq, offs.ctypes.data, None, None, None, None,
                                         None if spec is None else C.addressof(spec), k, 1)


def rejected(lib, spec, code, word, **kw):
    from searchlite_amd import _native as N
    sp, keep = spec if spec is not None else (None, None)
    assert prepare(lib, sp, **kw) is None
    assert lib.slg_last_error_code() == getattr(N, code), lib.slg_last_error()
    assert word.encode() in lib.slg_last_error(), lib.slg_last_error()


def _n_args(text, pattern):
    m = re.search(pattern, text, re.S)
    assert m, pattern
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_export_and_argument_counts(lib, name):
    assert hasattr(lib, name), f"{name} is not exported"
    assert len(getattr(lib, name).argtypes) == EXPORTS[name]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "searchlite_gpu.h")).read(), flags=re.S)
    assert _n_args(header, r"\b%s\s*\((.*?)\)\s*;" % name) == EXPORTS[name]
    rs = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    assert _n_args(rs, r"pub fn %s\((.*?)\)\s*->" % name) == EXPORTS[name]


def test_spec_layout_matches_the_header_and_the_rust_mirror(tmp_path):
    import subprocess
    from searchlite_amd import _native as N
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %u %d\\n", sizeof(slg_rescore_spec), offsetof(slg_rescore_spec, q_window),\n'
                   '         offsetof(slg_rescore_spec, q_mode), SLG_MAX_RESCORE_WINDOW, SLG_RESCORE_MIN);\n  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_window, o_mode, max_window, mode_min = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(N.RescoreSpec)
    assert o_window == N.RescoreSpec.q_window.offset and o_mode == N.RescoreSpec.q_mode.offset
    assert max_window == N.MAX_RESCORE_WINDOW == 1024 and mode_min == N.RESCORE_MIN
    assert (N.RESCORE_TOTAL, N.RESCORE_MULTIPLY, N.RESCORE_SUM, N.RESCORE_MAX, N.RESCORE_MIN) == (0, 1, 2, 3, 4)
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    body = re.search(r"pub struct slg_rescore_spec \{(.*?)\}", ffi, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", body) == [n for n, _ in N.RescoreSpec._fields_]


def test_null_spec_and_null_index(lib):
    rejected(lib, None, "ERR_INVALID", "rescore spec is NULL")
    rejected(lib, spec_of(), "ERR_INVALID", "index is NULL")  # a valid spec: the index is looked at next
    rejected(lib, spec_of(nq=0), "ERR_INVALID", "index is NULL", nq=0)


def test_null_arrays(lib):
    rejected(lib, spec_of(q_offsets=None), "ERR_INVALID", "q_offsets")
    rejected(lib, spec_of(q_window=None), "ERR_INVALID", "q_window")
    rejected(lib, spec_of(q_term_ids=None), "ERR_INVALID", "q_term_ids")
    rejected(lib, spec_of(q_weights=None), "ERR_INVALID", "q_weights")
    # a spec without a single term needs neither
    rejected(lib, spec_of(q_offsets=np.zeros(3, np.uint32), q_term_ids=None, q_weights=None), "ERR_INVALID", "index is NULL")


def test_inconsistent_offsets(lib):
    rejected(lib, spec_of(q_offsets=np.array([0, 3, 2], np.uint32)), "ERR_INVALID", "monotone")
    rejected(lib, spec_of(q_offsets=np.array([0, 5, 4], np.uint32), q_term_ids=np.zeros(5, np.uint32),
                          q_weights=np.ones(5, np.float32)), "ERR_INVALID", "monotone")


def test_too_many_terms(lib):
    from searchlite_amd import _native as N
    rejected(lib, spec_of(n_terms=N.MAX_QUERY_TERMS), "ERR_INVALID", "index is NULL")
    rejected(lib, spec_of(n_terms=N.MAX_QUERY_TERMS + 1), "ERR_INVALID", "terms")


@pytest.mark.parametrize("mode", [-1, 5, 100])
def test_mode_out_of_range(lib, mode):
    rejected(lib, spec_of(q_mode=np.array([0, mode], np.int32)), "ERR_INVALID", "score mode")


def test_every_mode_is_accepted(lib):
    for mode in range(5):
        rejected(lib, spec_of(q_mode=np.full(2, mode, np.int32)), "ERR_INVALID", "index is NULL")


@pytest.mark.parametrize("tie", [-0.01, 1.01, float("inf"), float("nan")])
def test_bad_tie(lib, tie):
    rejected(lib, spec_of(q_plan=np.array([0, 1], np.int32), q_tie=np.array([0.3, tie], np.float32)),
             "ERR_INVALID", "tie breaker")


def test_unknown_plan(lib):
    rejected(lib, spec_of(q_plan=np.array([0, 2], np.int32)), "ERR_INVALID", "score plan")


@pytest.mark.parametrize("w", [float("inf"), float("-inf"), float("nan")])
def test_non_finite_weight(lib, w):
    rejected(lib, spec_of(q_weights=np.array([1.0, 1.0, w, 1.0], np.float32)), "ERR_INVALID", "weight")


def test_window_limit(lib):
    """a window reaches no further than the k rows: min(window, k) is what must fit the widest register top-k"""
    from searchlite_amd import _native as N
    big = N.MAX_RESCORE_WINDOW
    rejected(lib, spec_of(q_window=np.array([big, 0], np.uint32)), "ERR_INVALID", "index is NULL", k=big + 1)
    rejected(lib, spec_of(q_window=np.array([0, big + 1], np.uint32)), "ERR_UNSUPPORTED", "SLG_MAX_RESCORE_WINDOW", k=big + 1)
    rejected(lib, spec_of(q_window=np.array([5000, 5000], np.uint32)), "ERR_UNSUPPORTED", "SLG_MAX_RESCORE_WINDOW", k=2000)
    rejected(lib, spec_of(q_window=np.array([5000, 5000], np.uint32)), "ERR_INVALID", "index is NULL", k=big)
    # an invalid argument is reported before an unsupported one
    rejected(lib, spec_of(q_window=np.array([big + 1, 0], np.uint32), q_mode=np.array([0, 9], np.int32)),
             "ERR_INVALID", "score mode", k=big + 1)


def test_other_entries_null_arguments(lib):
    from searchlite_amd import _native as N
    assert lib.slg_batch_fetch_rescore(None, None, None, None) == N.ERR_INVALID
    assert b"batch" in lib.slg_last_error()
    sp, keep = spec_of()
    assert lib.slg_search_batch_rescore(None, 0, None, None, None, None, None, C.addressof(sp), 11, 1, None, None,
                                        None, None, None, None, None) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error()
    assert lib.slg_search_batch_rescore(None, 0, None, None, None, None, None, None, 11, 1, None, None,
                                        None, None, None, None, None) == N.ERR_INVALID
    assert b"rescore spec is NULL" in lib.slg_last_error()
