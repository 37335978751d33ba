"""slg_batch_prepare_aggs / slg_index_add_agg_field_* argument checks that need no device: the spec is
checked before the index is looked at, a NULL index fails with SLG_ERR_INVALID and a message, before
anything touches a GPU (searchlite-ffi conventions, searchlite-ffi/src/lib.rs:24-43)."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def spec_of(*nodes):
    """nodes: dicts of slg_agg_node fields"""
    from searchlite_amd import _native as N
    sp = N.AggSpec()
    sp.n_nodes = len(nodes)
    for i, nd in enumerate(nodes[:N.MAX_AGGS]):
        for name, val in nd.items():
            if name in ("from_", "to"):
                for r, x in enumerate(val):
                    getattr(sp.nodes[i], name)[r] = x
            else:
                setattr(sp.nodes[i], name, val)
    return sp


def prepare(lib, spec):
    offs = np.zeros(1, np.uint32)
    return lib.slg_batch_prepare_aggs(None, 0, offs.ctypes.data, None, None, None, None, None,
                                      None if spec is None else C.addressof(spec), 11, 1)


def rejected(lib, spec, code, word):
    from searchlite_amd import _native as N
    assert prepare(lib, spec) is None
    assert lib.slg_last_error_code() == getattr(N, code), lib.slg_last_error()
    assert word.encode() in lib.slg_last_error(), lib.slg_last_error()


TERMS = dict(kind=0, field=0, parent=-1)
STATS = dict(kind=3, field=1, parent=-1)
HIST = dict(kind=1, field=1, parent=-1, interval=5.0)


def test_null_spec_and_null_index(lib):
    rejected(lib, None, "ERR_INVALID", "aggs is NULL")
    rejected(lib, spec_of(TERMS), "ERR_INVALID", "index is NULL")  # a valid spec: the index is looked at next


def test_node_count(lib):
    from searchlite_amd import _native as N
    rejected(lib, spec_of(), "ERR_INVALID", "at least one node")
    sp = spec_of(*([STATS] * N.MAX_AGGS))
    rejected(lib, sp, "ERR_INVALID", "index is NULL")  # SLG_MAX_AGGS nodes are fine
    sp.n_nodes = N.MAX_AGGS + 1
    rejected(lib, sp, "ERR_UNSUPPORTED", "SLG_MAX_AGGS")


def test_unknown_kind(lib):
    rejected(lib, spec_of(dict(kind=7, field=0, parent=-1)), "ERR_INVALID", "unknown kind")


def test_parent_must_be_an_earlier_bucket_root(lib):
    child = lambda p: dict(kind=3, field=1, parent=p)
    rejected(lib, spec_of(child(1), TERMS), "ERR_INVALID", "earlier")         # a later node
    rejected(lib, spec_of(child(0)), "ERR_INVALID", "earlier")                # itself
    rejected(lib, spec_of(TERMS, child(-2)), "ERR_INVALID", "earlier")
    rejected(lib, spec_of(STATS, child(0)), "ERR_INVALID", "not a bucket")    # a child of a stats node
    rejected(lib, spec_of(TERMS, dict(kind=0, field=0, parent=0), child(1)), "ERR_INVALID", "not a root")  # three levels
    rejected(lib, spec_of(TERMS, child(0)), "ERR_INVALID", "index is NULL")   # the well-formed one


@pytest.mark.parametrize("interval", [0.0, -1.0, float("inf"), float("nan")])
def test_bad_interval(lib, interval):
    rejected(lib, spec_of(dict(HIST, interval=interval)), "ERR_INVALID", "interval")


def test_bad_numbers(lib):
    nan = float("nan")
    rejected(lib, spec_of(dict(HIST, offset=nan)), "ERR_INVALID", "offset")
    rejected(lib, spec_of(dict(HIST, has_missing=1, missing=float("inf"))), "ERR_INVALID", "missing")
    rejected(lib, spec_of(dict(HIST, has_hard_bounds=1, hard_min=nan, hard_max=1.0)), "ERR_INVALID", "hard bound")
    rng = dict(kind=2, field=1, parent=-1)
    rejected(lib, spec_of(dict(rng, n_ranges=0)), "ERR_INVALID", "at least one range")
    rejected(lib, spec_of(dict(rng, n_ranges=17)), "ERR_UNSUPPORTED", "SLG_MAX_AGG_RANGES")
    rejected(lib, spec_of(dict(rng, n_ranges=1, from_=[nan], to=[1.0])), "ERR_INVALID", "range bound")
    ok = dict(rng, n_ranges=2, from_=[float("-inf"), 2.0], to=[2.0, float("inf")])  # absent bounds are infinities
    rejected(lib, spec_of(ok), "ERR_INVALID", "index is NULL")


@pytest.mark.parametrize("name", ["slg_index_add_agg_field_f64", "slg_index_add_agg_field_i64"])
def test_add_field_null_index(lib, name):
    from searchlite_amd import _native as N
    assert getattr(lib, name)(None, None, None) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error() and lib.slg_last_error_code() == N.ERR_INVALID


def test_other_entries_null_arguments(lib):
    from searchlite_amd import _native as N
    assert lib.slg_index_add_agg_field_ord(None, None, None, 8) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error()
    assert lib.slg_index_remove_agg_field(None, 0) == N.ERR_INVALID
    assert lib.slg_batch_agg_layout(None, None) == N.ERR_INVALID
    assert b"batch" in lib.slg_last_error()
    assert lib.slg_batch_fetch_aggs(None, None, None) == N.ERR_INVALID
    sp = spec_of(TERMS)
    assert lib.slg_search_batch_aggs(None, None, 0, None, None, None, C.addressof(sp), 11, 1, None, None, None,
                                     None, None, None, None) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error()
