"""slg_batch_prepare_aggs spec checks of the date_histogram and filter kinds that need no device, in the manner of
tests/test_agg_args.py: the spec is checked before the index is looked at, so a valid spec gets as far as
"index is NULL"; what the spec alone decides fails with its code and a message before that."""
import ctypes as C

import numpy as np
import pytest

TWO53 = 1 << 53


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def spec_of(*nodes):
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
    return lib.slg_batch_prepare_aggs(None, 0, offs.ctypes.data, None, None, None, None, None, C.addressof(spec), 11, 1)


def rejected(lib, spec, code, word):
    from searchlite_amd import _native as N
    assert prepare(lib, spec) is None
    assert lib.slg_last_error_code() == getattr(N, code), lib.slg_last_error()
    assert word.encode() in lib.slg_last_error(), lib.slg_last_error()


def valid(lib, *nodes):
    rejected(lib, spec_of(*nodes), "ERR_INVALID", "index is NULL")


DATE = dict(kind=8, field=1, parent=-1, calendar_unit=0, date_step=1000)
MONTH = dict(kind=8, field=1, parent=-1, calendar_unit=3)
FILTER = dict(kind=9, parent=-1, filter=0)
TERMS = dict(kind=0, field=0, parent=-1)
STATS = dict(kind=3, field=1, parent=-1)


def test_constants_and_struct():
    from searchlite_amd import _native as N
    assert (N.AGG_DATE_HISTOGRAM, N.AGG_FILTER) == (8, 9)
    assert (N.DATE_FIXED, N.DATE_DAY, N.DATE_WEEK, N.DATE_MONTH, N.DATE_QUARTER, N.DATE_YEAR) == (0, 1, 2, 3, 4, 5)
    # the new members are appended: the old ones keep their offsets
    assert (N.AggNode.kind.offset, N.AggNode.missing.offset, N.AggNode.n_ranges.offset, N.AggNode.to.offset) == \
        (0, 16, 64, 200)
    assert N.AggNode.calendar_unit.offset == 328 and C.sizeof(N.AggNode) == 368


def test_seven_is_still_no_kind(lib):
    """7 stays unassigned between the value kinds and the two new ones; 10 is the first unknown kind above them"""
    rejected(lib, spec_of(dict(kind=7, field=0, parent=-1)), "ERR_INVALID", "unknown kind")
    rejected(lib, spec_of(dict(kind=10, field=0, parent=-1)), "ERR_INVALID", "unknown kind")
    valid(lib, DATE)
    valid(lib, FILTER)


def test_valid_specs_as_root_child_and_parent(lib):
    child = lambda nd, p=0: dict(nd, parent=p)
    valid(lib, DATE)
    valid(lib, MONTH)
    valid(lib, FILTER)
    valid(lib, FILTER, dict(FILTER, filter=3))                       # two root filters
    valid(lib, TERMS, child(DATE), child(MONTH), child(FILTER))       # as children of an older bucket kind
    for root in (DATE, MONTH, FILTER):                                # as parents of every kind that can be a child
        valid(lib, root, child(STATS), child(TERMS), child(dict(kind=1, field=1, interval=5.0)),
              child(dict(kind=2, field=1, n_ranges=1, from_=[0.0], to=[1.0])), child(dict(kind=4, field=0)),
              child(dict(kind=6, field=1, n_ranges=1, from_=[0.5])), child(DATE))
        valid(lib, root, child(FILTER), child(MONTH))
    for unit in range(1, 6):
        valid(lib, dict(MONTH, calendar_unit=unit, date_step=0))     # a calendar unit reads no step
    valid(lib, dict(DATE, date_step=1))
    valid(lib, dict(DATE, date_offset=-3, has_hard_bounds=1, date_hard_min=5, date_hard_max=-5))  # bounds that leave nothing
    valid(lib, dict(DATE, date_offset=TWO53, has_missing=1, missing=-float(TWO53), has_hard_bounds=1,
                    date_hard_min=-TWO53, date_hard_max=TWO53))        # +-2^53 itself is within the limits


def test_invalid(lib):
    for step in (0, -1, -(1 << 40)):
        rejected(lib, spec_of(dict(DATE, date_step=step)), "ERR_INVALID", "at least 1 ms")
    for unit in (6, 7, 0xFFFFFFFF):
        rejected(lib, spec_of(dict(MONTH, calendar_unit=unit)), "ERR_INVALID", "calendar unit")
    for f in (-1, -(1 << 31)):
        rejected(lib, spec_of(dict(FILTER, filter=f)), "ERR_INVALID", "filter id is negative")
    rejected(lib, spec_of(dict(DATE, has_missing=1, missing=float("nan"))), "ERR_INVALID", "missing")
    # a parent that is not an earlier bucket root: the new kinds count as bucket roots
    child = lambda nd, p: dict(nd, parent=p)
    rejected(lib, spec_of(child(STATS, 1), DATE), "ERR_INVALID", "earlier")
    rejected(lib, spec_of(child(FILTER, 0)), "ERR_INVALID", "earlier")
    rejected(lib, spec_of(STATS, child(DATE, 0)), "ERR_INVALID", "not a bucket")
    rejected(lib, spec_of(STATS, child(FILTER, 0)), "ERR_INVALID", "not a bucket")
    rejected(lib, spec_of(FILTER, child(DATE, 0), child(STATS, 1)), "ERR_INVALID", "not a root")     # three levels
    rejected(lib, spec_of(DATE, child(FILTER, 0), child(STATS, 1)), "ERR_INVALID", "not a root")
    # an invalid node is reported before an unsupported one
    rejected(lib, spec_of(dict(DATE, date_offset=TWO53 + 1), dict(DATE, date_step=0)), "ERR_INVALID", "at least 1 ms")


def test_unsupported(lib):
    rejected(lib, spec_of(dict(DATE, date_offset=TWO53 + 1)), "ERR_UNSUPPORTED", "offset")
    rejected(lib, spec_of(dict(MONTH, date_offset=-TWO53 - 1)), "ERR_UNSUPPORTED", "offset")
    rejected(lib, spec_of(dict(DATE, has_missing=1, missing=float(TWO53) * 2)), "ERR_UNSUPPORTED", "missing")
    rejected(lib, spec_of(dict(DATE, has_missing=1, missing=-float(TWO53 + 2))), "ERR_UNSUPPORTED", "missing")
    rejected(lib, spec_of(dict(DATE, has_hard_bounds=1, date_hard_min=0, date_hard_max=TWO53 + 1)),
             "ERR_UNSUPPORTED", "hard bound")
    rejected(lib, spec_of(dict(DATE, has_hard_bounds=1, date_hard_min=-TWO53 - 1, date_hard_max=0)),
             "ERR_UNSUPPORTED", "hard bound")
    valid(lib, dict(DATE, date_hard_min=-TWO53 - 1, date_hard_max=TWO53 + 1))  # (not read without has_hard_bounds)
    # a percentiles node stays root-only under the new parents too
    rejected(lib, spec_of(FILTER, dict(kind=5, field=1, parent=0, n_ranges=1, from_=[50.0])), "ERR_UNSUPPORTED", "root")
