"""The argument checks of the value nodes (cardinality, percentiles, percentile_ranks) that need no index or
device: the spec is checked before the index is looked at (tests/test_agg_args.py's conventions)."""
import ctypes as C

import pytest

from tests.test_agg_args import prepare, rejected, spec_of

TERMS = dict(kind=0, field=0, parent=-1)
CARD = dict(kind=4, field=1, parent=-1)
PCT = dict(kind=5, field=1, parent=-1, n_ranges=2, from_=[50.0, 99.0])
RANKS = dict(kind=6, field=1, parent=-1, n_ranges=1, from_=[3.0])


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def test_the_three_kinds_are_known_and_kind_7_is_not(lib):
    from searchlite_amd import _native as N
    assert (N.AGG_CARDINALITY, N.AGG_PERCENTILES, N.AGG_PERCENTILE_RANKS) == (4, 5, 6)
    for node in (CARD, PCT, RANKS):
        rejected(lib, spec_of(node), "ERR_INVALID", "index is NULL")  # well-formed: the index is looked at next
    rejected(lib, spec_of(dict(kind=7, field=0, parent=-1)), "ERR_INVALID", "unknown kind")
    rejected(lib, spec_of(dict(kind=-1, field=0, parent=-1)), "ERR_INVALID", "unknown kind")


@pytest.mark.parametrize("node,word", [(PCT, "percent"), (RANKS, "target")])
def test_percents_and_targets(lib, node, word):
    rejected(lib, spec_of(dict(node, n_ranges=0)), "ERR_INVALID", "at least one " + word)
    rejected(lib, spec_of(dict(node, n_ranges=17)), "ERR_UNSUPPORTED", "SLG_MAX_AGG_RANGES")
    rejected(lib, spec_of(dict(node, n_ranges=2, from_=[1.0, float("nan")])), "ERR_INVALID", word + " is NaN")
    ok = dict(node, n_ranges=16, from_=[float(i) for i in range(16)])
    rejected(lib, spec_of(ok), "ERR_INVALID", "index is NULL")
    # out-of-range and infinite percents are clamped, not refused (pct.clamp(0, 100), aggs/mod.rs:530)
    rejected(lib, spec_of(dict(node, n_ranges=3, from_=[-5.0, 250.0, float("inf")])), "ERR_INVALID", "index is NULL")


def test_missing_must_be_finite_for_the_quantile_kinds(lib):
    for node in (PCT, RANKS):
        rejected(lib, spec_of(dict(node, has_missing=1, missing=float("nan"))), "ERR_INVALID", "missing")
    # a cardinality node's f64 `missing` is read for a numeric field only: the index decides
    rejected(lib, spec_of(dict(CARD, has_missing=1, missing=float("nan"))), "ERR_INVALID", "index is NULL")


def test_parents(lib):
    rejected(lib, spec_of(TERMS, dict(CARD, parent=0)), "ERR_INVALID", "index is NULL")
    rejected(lib, spec_of(TERMS, dict(RANKS, parent=0)), "ERR_INVALID", "index is NULL")
    rejected(lib, spec_of(TERMS, dict(PCT, parent=0)), "ERR_UNSUPPORTED", "percentiles node is a root")
    rejected(lib, spec_of(CARD, dict(kind=3, field=1, parent=0)), "ERR_INVALID", "not a bucket")  # no children
    rejected(lib, spec_of(dict(CARD, parent=1), TERMS), "ERR_INVALID", "earlier")


def test_new_entry_points_null_arguments(lib):
    from searchlite_amd import _native as N
    assert lib.slg_index_rank_agg_field(None, 0) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error() and lib.slg_last_error_code() == N.ERR_INVALID
    assert lib.slg_batch_fetch_agg_values(None, None) == N.ERR_INVALID
    assert b"batch" in lib.slg_last_error()
    sp = spec_of(CARD)
    args = (None, None, 0, None, None, None, C.addressof(sp), 11, 1, None, None, None, None, None, None, None)
    assert lib.slg_search_batch_agg_values(*args, None) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error()


def test_the_old_one_shot_refuses_value_nodes(lib):
    """slg_search_batch_aggs has nowhere to put a value table: SLG_ERR_INVALID, nothing dropped silently"""
    from searchlite_amd import _native as N
    for node in (CARD, PCT, RANKS):
        sp = spec_of(TERMS, dict(node, parent=-1))
        assert lib.slg_search_batch_aggs(None, None, 0, None, None, None, C.addressof(sp), 11, 1, None, None, None,
                                         None, None, None, None) == N.ERR_INVALID
        assert b"slg_search_batch_agg_values" in lib.slg_last_error(), lib.slg_last_error()
