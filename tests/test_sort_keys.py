"""CPU tests of the host side of field-sorted search (slg_index_add_sort_field_i64 / _f64): the Min / Max
selection of a doc's values and the order-preserving key encoding, through the planner test library
(slgp_sort_keys in lib/libslg_plan.so).  Ordering docs by their encoded (presence, key) must be the
reference's SortKey::cmp on one field part (query/sort.rs:80-123, 300-345), in both orders."""
import ctypes as C
import functools
import math
import struct

import numpy as np
import pytest

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import build
    L = C.CDLL(build.build_plan_lib())
    L.slgp_sort_keys.restype = C.c_int
    L.slgp_sort_keys.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- a restatement of the reference, in Python ----------------------------------------------------
def partial_gt(a, b):
    """a.partial_cmp(b) == Some(Greater)"""
    return a > b  # (False when either is NaN: None -> Equal)


def pick(values, order):
    """pick_numeric: min_by (Asc) keeps the first of 'equal' elements, max_by (Desc) the last."""
    if not values:
        return None
    acc = values[0]
    for y in values[1:]:
        if order == "asc":
            if partial_gt(acc, y):
                acc = y
        else:
            if not partial_gt(acc, y):
                acc = y
    return acc


def total_key(x, is_float):
    if not is_float:
        return x
    b = bits(x)
    return b ^ 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)  # f64::total_cmp as an integer order


def sortkey_cmp(a, b, order, is_float):
    """SortKeyPart::cmp then doc id (one segment): a, b = (value or None, doc)"""
    va, vb = a[0], b[0]
    if va is None and vb is None:
        c = 0
    elif va is None:
        c = 1
    elif vb is None:
        c = -1
    else:
        ka, kb = total_key(va, is_float), total_key(vb, is_float)
        c = (ka > kb) - (ka < kb)
        if order == "desc":
            c = -c
    if c:
        return c
    return (a[1] > b[1]) - (a[1] < b[1])


def encode(lib, kind, docs_values):
    n = len(docs_values)
    offs = np.zeros(n + 1, np.uint32)
    for d, v in enumerate(docs_values):
        offs[d + 1] = offs[d] + len(v)
    flat = [x for v in docs_values for x in v]
    if kind == 1:
        vals = np.array(flat, dtype=np.int64) if flat else np.zeros(1, np.int64)
    else:
        vals = np.array([bits(x) for x in flat], dtype=np.uint64).view(np.float64) if flat else np.zeros(1)
    asc = np.zeros(max(n, 1), np.uint64)
    desc = np.zeros(max(n, 1), np.uint64)
    pres = np.zeros(max((n + 31) // 32, 1), np.uint32)
    rc = lib.slgp_sort_keys(kind, n, offs.ctypes.data, vals.ctypes.data, asc.ctypes.data, desc.ctypes.data,
                            pres.ctypes.data)
    assert rc == 0
    present = [(int(pres[d >> 5]) >> (d & 31)) & 1 for d in range(n)]
    return asc[:n], desc[:n], present


def check_order(lib, kind, docs_values):
    is_float = kind == 2
    asc, desc, present = encode(lib, kind, docs_values)
    for order, col in (("asc", asc), ("desc", desc)):
        want = sorted(range(len(docs_values)),
                      key=functools.cmp_to_key(lambda x, y: sortkey_cmp(
                          (pick(docs_values[x], order), x), (pick(docs_values[y], order), y), order, is_float)))
        got = sorted(range(len(docs_values)), key=lambda d: (1 - present[d], int(col[d]), d))
        assert got == want, (order, got, want)
        for d, v in enumerate(docs_values):
            assert present[d] == (1 if v else 0)
            if not v:
                assert int(col[d]) == 0  # Missing docs carry no value: they tie among themselves


NAN_PAYLOADS = [f64(0x7FF8000000000000), f64(0x7FF0000000000001), f64(0x7FFFFFFFFFFFFFFF),
                f64(0xFFF8000000000000), f64(0xFFFFFFFFFFFFFFFF), f64(0xFFF0000000000001)]


def test_i64_extremes_and_missing(lib):
    docs = [[0], [I64_MIN], [I64_MAX], [], [-1], [1], [I64_MAX, I64_MIN], [], [5, 5, 5], [3, -7, 12], [-7, 3]]
    check_order(lib, 1, docs)


def test_i64_extremes_keep_their_own_code_points(lib):
    """i64::MAX under Asc and i64::MIN under Desc map to the extreme u64: only the presence bit tells them
    from Missing."""
    asc, desc, present = encode(lib, 1, [[I64_MAX], [I64_MIN], []])
    assert int(asc[0]) == 0xFFFFFFFFFFFFFFFF and int(desc[1]) == 0xFFFFFFFFFFFFFFFF
    assert present == [1, 1, 0]


def test_f64_signed_zero_inf_and_nan_payloads(lib):
    docs = [[0.0], [-0.0], [math.inf], [-math.inf], [], [1.5], [-1.5]] + [[x] for x in NAN_PAYLOADS]
    check_order(lib, 2, docs)


def test_f64_largest_nan_is_the_extreme_key(lib):
    asc, desc, present = encode(lib, 2, [[f64(0x7FFFFFFFFFFFFFFF)], [f64(0xFFFFFFFFFFFFFFFF)]])
    assert int(asc[0]) == 0xFFFFFFFFFFFFFFFF and int(desc[1]) == 0xFFFFFFFFFFFFFFFF


def test_min_by_keeps_the_first_and_max_by_the_last_of_equals(lib):
    """partial_cmp(-0.0, 0.0) == Equal and NaN compares Equal to everything: which element is picked
    decides the total_cmp order afterwards."""
    nan, nnan = NAN_PAYLOADS[0], NAN_PAYLOADS[3]
    docs = [[0.0, -0.0], [-0.0, 0.0], [nan, 1.0], [1.0, nan], [2.0, nan, -3.0], [nan, nnan], [nnan, nan],
            [-0.0, -0.0, 0.0], [3.0, nan, 1.0, nan], [nan], [math.inf, nan, -math.inf], []]
    check_order(lib, 2, docs)
    asc, desc, _ = encode(lib, 2, docs)
    # min_by over [0.0, -0.0] keeps 0.0, max_by keeps -0.0
    assert int(asc[0]) == total_key(0.0, True) and int(~desc[0] & 0xFFFFFFFFFFFFFFFF) == total_key(-0.0, True)
    # [NaN, 1.0]: min_by keeps NaN (NaN vs anything = Equal), max_by takes the last: 1.0
    assert int(asc[2]) == total_key(nan, True) and int(~desc[2] & 0xFFFFFFFFFFFFFFFF) == total_key(1.0, True)


def test_random_multi_valued_docs(lib):
    rng = np.random.default_rng(5)
    pool_f = [0.0, -0.0, 1.0, -1.0, 2.5, math.inf, -math.inf] + NAN_PAYLOADS
    pool_i = [0, 1, -1, 7, -7, I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1]
    for kind, pool in ((1, pool_i), (2, pool_f)):
        docs = [[pool[i] for i in rng.integers(0, len(pool), int(rng.integers(0, 5)))] for _ in range(300)]
        check_order(lib, kind, docs)


def test_no_offsets_means_every_doc_missing(lib):
    asc = np.ones(5, np.uint64)
    desc = np.ones(5, np.uint64)
    pres = np.full(1, 0xFFFFFFFF, np.uint32)
    assert lib.slgp_sort_keys(1, 5, None, None, asc.ctypes.data, desc.ctypes.data, pres.ctypes.data) == 0
    assert int(pres[0]) == 0 and not asc.any() and not desc.any()


def test_unknown_kind_is_rejected(lib):
    asc = np.zeros(1, np.uint64)
    pres = np.zeros(1, np.uint32)
    assert lib.slgp_sort_keys(3, 1, None, None, asc.ctypes.data, asc.ctypes.data, pres.ctypes.data) == -1
