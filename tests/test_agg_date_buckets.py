"""The bucket function of a date_histogram node (slg::date_bucket_id, csrc/slg_date.hpp: what the planner's row
range and the aggregation kernels run), swept on the CPU through slgp_date_buckets of lib/libslg_plan.so: the
calendar path against `datetime` over the whole supported range 0001-01-01 .. 9999-12-31, the fixed path against
math.ceil of the one f64 quotient.  No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import agg_date_ref as D

UNITS = {1: "day", 2: "week", 3: "month", 4: "quarter", 5: "year"}
TWO53 = 1 << 53


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import build
    L = C.CDLL(build.build_plan_lib())
    L.slgp_date_buckets.restype = C.c_int
    L.slgp_date_buckets.argtypes = [C.c_uint32, C.c_int64, C.c_int64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    return L


def buckets(lib, unit, step, offset, vals):
    vals = np.ascontiguousarray(vals, dtype=np.int64)
    ids, ymd = np.zeros(len(vals), np.int64), np.zeros((len(vals), 3), np.int32)
    assert lib.slgp_date_buckets(unit, step, offset, vals.ctypes.data, len(vals), ids.ctypes.data, ymd.ctypes.data) == 0
    return ids, ymd


@pytest.fixture(scope="module")
def instants():
    """100 000 random instants over the supported range, the edge list, and the ms around 2 000 random midnights"""
    rng = np.random.default_rng(19700101)
    rand = rng.integers(D.MIN_MS, D.MAX_MS + 1, 100_000)
    nights = rng.integers(D.MIN_MS // 86_400_000, D.MAX_MS // 86_400_000, 2000) * 86_400_000
    near = np.concatenate([nights - 1, nights, nights + 1])
    vals = np.concatenate([rand, np.array(D.edge_instants(), np.int64), near[(near >= D.MIN_MS) & (near <= D.MAX_MS)]])
    dates = [D.day_of(int(t)) for t in vals]  # (datetime, once for every unit)
    return vals, dates


@pytest.mark.parametrize("unit", list(UNITS))
def test_calendar_ids_and_civil_dates_against_datetime(lib, instants, unit):
    vals, dates = instants
    ids, ymd = buckets(lib, unit, 0, 0, vals)
    assert ymd.tolist() == [[d.year, d.month, d.day] for d in dates]
    cfg = dict(unit=UNITS[unit], step=0, offset=0)
    assert ids.tolist() == [D.dense_id(int(t), cfg) for t in vals]
    # the ids are monotone in the value (the planner's row range rests on it) and dense: consecutive edge ids
    order = np.argsort(vals, kind="stable")
    assert (np.diff(ids[order]) >= 0).all()


@pytest.mark.parametrize("unit", list(UNITS))
def test_calendar_offset_shifts_the_instant(lib, unit):
    hour = 3_600_000
    vals = np.array([v for v in D.edge_instants() if v - hour >= D.MIN_MS] + [D.MIN_MS + hour, D.MAX_MS], np.int64)
    ids, ymd = buckets(lib, unit, 0, hour, vals)
    cfg = dict(unit=UNITS[unit], step=0, offset=hour)
    assert ids.tolist() == [D.dense_id(int(t), cfg) for t in vals]
    assert ymd.tolist() == [[d.year, d.month, d.day] for d in (D.day_of(int(t) - hour) for t in vals)]


@pytest.mark.parametrize("step", [1, 7, 1000, 86_400_000])
@pytest.mark.parametrize("offset", [0, 500, -3])
def test_fixed_ids_against_ceil_of_the_f64_quotient(lib, step, offset):
    rng = np.random.default_rng(step + 13)
    ks = np.concatenate([np.arange(-40, 41), rng.integers(-(TWO53 // step) + 2, TWO53 // step - 2, 400)])
    on = ks * step + offset  # on a boundary: its own bucket; one off: the next boundary
    vals = np.concatenate([on - 1, on, on + 1, rng.integers(-TWO53, TWO53, 20_000),
                           np.array([-TWO53, -TWO53 + 1, TWO53 - 1, TWO53, 0, -1, 1])])
    vals = vals[(vals >= -TWO53) & (vals <= TWO53)]
    ids, _ = buckets(lib, 0, step, offset, vals)
    want = [math.ceil(float(int(v) - offset) / float(step)) for v in vals]
    assert ids.tolist() == want
    small = np.abs(on) < (1 << 50)  # (where the quotient is exact: a value on k step + offset is bucket k)
    got_on, _ = buckets(lib, 0, step, offset, on[small])
    assert got_on.tolist() == ks[small].tolist()
    got_next, _ = buckets(lib, 0, step, offset, on[small] + 1)
    assert got_next.tolist() == (ks[small] + 1).tolist()
    if step > 1:
        got_prev, _ = buckets(lib, 0, step, offset, on[small] - 1)
        assert got_prev.tolist() == ks[small].tolist()


def test_the_reference_s_recorded_fixed_case(lib):
    ids, _ = buckets(lib, 0, 1000, 500, [0, 1000, 1600, 500, 3000])  # tests/aggregations.rs:840-952
    assert (ids * 1000 + 500).tolist() == [500, 1500, 2500, 500, 3500]


def test_arguments(lib):
    v = np.zeros(1, np.int64)
    call = lambda unit, step, n=1, p=v.ctypes.data: lib.slgp_date_buckets(unit, step, 0, p, n, None, None)
    assert call(0, 1) == 0 and call(5, 0) == 0 and call(3, 0, 0, None) == 0  # (either output may be NULL)
    assert call(6, 1) < 0 and call(0, 0) < 0 and call(0, -5) < 0 and call(1, 0, 1, None) < 0
