"""CPU tests of the host side of cursor pagination (slg_batch_prepare_after): the cursor's key words the select
kernels compare, through the planner test library (slgp_cursor_key in lib/libslg_plan.so).

A field part's cursor value is the value the reference already picked for the page's last hit, so encoded
directly it must give exactly that doc's column key and presence (slgp_sort_keys), in both orders.  A score
encodes as the ordered u32 the scoring kernels write into a candidate (f32::total_cmp order).  Malformed
cursors are rejected with SLG_ERR_INVALID."""
import ctypes as C
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests.test_sort_keys import I64_MAX, I64_MIN, NAN_PAYLOADS, bits, encode, f64, pick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -1
WORDS = 14  # 3 * SLG_MAX_SORT_PARTS + 2
ASC, DESC = 0, 1


class Cursor(C.Structure):
    _fields_ = [("has_cursor", C.c_uint32), ("segment_ord", C.c_uint32), ("doc_id", C.c_uint32),
                ("missing_mask", C.c_uint32), ("value_bits", C.c_uint64 * 4)]


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import build
    L = C.CDLL(build.build_plan_lib())
    L.slgp_sort_keys.restype = C.c_int
    L.slgp_sort_keys.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.slgp_cursor_key.restype = C.c_int
    L.slgp_cursor_key.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def cursor(values, seg=0, doc=0, kinds=None):
    """values: per part an int (i64), a float (f64; a score part's value is taken as f32 bits when kinds[i] is
    0), None (Missing)"""
    c = Cursor()
    c.has_cursor, c.segment_ord, c.doc_id = 1, seg, doc
    for i, v in enumerate(values):
        if v is None:
            c.missing_mask |= 1 << i
        elif kinds is not None and kinds[i] == 0:
            c.value_bits[i] = f32_bits(v)
        elif isinstance(v, float):
            c.value_bits[i] = bits(v)
        else:
            c.value_bits[i] = v & 0xFFFFFFFFFFFFFFFF
    return c


def key_words(lib, kinds, orders, c):
    """-> (rc, words); kinds == None: score order (3 words)"""
    out = np.zeros(WORDS, np.uint32)
    if kinds is None:
        rc = lib.slgp_cursor_key(0, None, None, C.addressof(c), out.ctypes.data)
        return rc, [int(x) for x in out[:3]]
    k = np.array(kinds, np.int32)
    o = np.array(orders, np.int32)
    rc = lib.slgp_cursor_key(len(kinds), k.ctypes.data, o.ctypes.data, C.addressof(c), out.ctypes.data)
    return rc, [int(x) for x in out]


def check_field_docs(lib, kind, docs_values):
    asc, desc, present = encode(lib, kind, docs_values)
    for order, col in ((ASC, asc), (DESC, desc)):
        for d, vals in enumerate(docs_values):
            v = pick(vals, "asc" if order == ASC else "desc")
            rc, w = key_words(lib, [kind], [order], cursor([v], seg=3, doc=d))
            assert rc == 0
            assert w[0] == 1 - present[d], (d, vals)
            assert (w[1] << 32 | w[2]) == int(col[d]), (d, vals, order)
            assert w[3:12] == [0] * 9  # parts beyond the spec
            assert w[12:] == [3, d]


def test_i64_cursor_is_the_docs_own_column_key(lib):
    docs = [[0], [1], [-1], [I64_MIN], [I64_MAX], [I64_MAX, I64_MIN], [5, -5, 5], [], [7, 7], [I64_MIN + 1]]
    check_field_docs(lib, 1, docs)


def test_f64_cursor_is_the_docs_own_column_key(lib):
    docs = [[0.0], [-0.0], [0.0, -0.0], [-0.0, 0.0], [math.inf], [-math.inf], [1.5, -1.5], [], [5e-324],
            [-5e-324], [1.0, math.nan], [math.nan, 1.0]] + [[n] for n in NAN_PAYLOADS] + \
           [[NAN_PAYLOADS[0], NAN_PAYLOADS[3]], [NAN_PAYLOADS[4], 2.0, NAN_PAYLOADS[2]]]
    check_field_docs(lib, 2, docs)


def test_random_multi_valued_docs(lib):
    rng = np.random.default_rng(5)
    pool_f = [0.0, -0.0, 1.0, -1.0, math.inf, -math.inf, 2.5] + NAN_PAYLOADS
    docs = [[pool_f[j] for j in rng.integers(0, len(pool_f), int(rng.integers(0, 4)))] for _ in range(300)]
    check_field_docs(lib, 2, docs)
    docs = [[int(x) for x in rng.integers(-3, 3, int(rng.integers(0, 4)))] for _ in range(300)]
    check_field_docs(lib, 1, docs)


F32_EDGES = [0.0, -0.0, 1.0, -1.0, math.inf, -math.inf, 1e-45, -1e-45, 1.1754942e-38, 3.4028235e38, -3.4028235e38]
F32_NAN_BITS = [0x7FC00000, 0x7F800001, 0x7FFFFFFF, 0xFFC00000, 0xFF800001, 0xFFFFFFFF]


def total_cmp_key(b):
    """f32::total_cmp as an integer order of the bits"""
    s = b - (1 << 32) if b >> 31 else b
    return s ^ 0x7FFFFFFF if s < 0 else s


def test_score_encoding_orders_like_total_cmp(lib):
    rng = np.random.default_rng(9)
    pool = [f32_bits(x) for x in F32_EDGES] + F32_NAN_BITS + [int(x) for x in rng.integers(0, 1 << 32, 200)]
    got = {}
    for b in pool:
        c = Cursor()
        c.has_cursor, c.segment_ord, c.doc_id, c.value_bits[0] = 1, 2, 9, b
        rc, w = key_words(lib, None, None, c)
        assert rc == 0
        assert w[1:] == [0xFFFFFFFD, 0xFFFFFFF6]  # ~segment, ~doc: the descending key of select_topk_kernel
        assert w[0] == (total_cmp_key(b) + (1 << 31)) & 0xFFFFFFFF  # ordered score = total_cmp key, unsigned
        got[b] = w[0]
    assert sorted(pool, key=lambda b: got[b]) == sorted(pool, key=total_cmp_key)
    assert got[f32_bits(-0.0)] < got[f32_bits(0.0)]


def test_score_part_of_a_field_sort(lib):
    for b in [f32_bits(x) for x in F32_EDGES] + F32_NAN_BITS:
        c = Cursor()
        c.has_cursor, c.value_bits[1] = 1, b
        c.value_bits[0] = 42
        a = (total_cmp_key(b) + (1 << 31)) & 0xFFFFFFFF
        for order in (ASC, DESC):
            rc, w = key_words(lib, [1, 0], [ASC, order], c)
            assert rc == 0
            assert w[3:6] == [0, 0, a if order == ASC else a ^ 0xFFFFFFFF]
            assert w[0:3] == [0, 1 << 31, 42]  # i64 42: the sign bit flipped


def test_four_parts_and_missing(lib):
    kinds, orders = [2, 1, 0, 1], [DESC, ASC, DESC, DESC]
    rc, w = key_words(lib, kinds, orders, cursor([None, -7, 1.5, None], seg=1, doc=77, kinds=kinds))
    assert rc == 0
    k_i64 = (-7 & 0xFFFFFFFFFFFFFFFF) ^ (1 << 63)
    a = (total_cmp_key(f32_bits(1.5)) + (1 << 31)) & 0xFFFFFFFF
    assert w == [1, 0, 0, 0, k_i64 >> 32, k_i64 & 0xFFFFFFFF, 0, 0, a ^ 0xFFFFFFFF, 1, 0, 0, 1, 77]


@pytest.mark.parametrize("case", ["missing_score", "missing_score_order", "missing_beyond", "value_beyond",
                                  "value_beyond_score_order", "score_high_bits", "unknown_kind"])
def test_malformed_cursors_are_rejected(lib, case):
    c = Cursor()
    c.has_cursor = 1
    kinds, orders = [1, 0], [ASC, DESC]
    if case == "missing_score":
        c.missing_mask = 2
    elif case == "missing_score_order":
        c.missing_mask = 1
        kinds = None
    elif case == "missing_beyond":
        c.missing_mask = 4
    elif case == "value_beyond":
        c.value_bits[2] = 1
    elif case == "value_beyond_score_order":
        c.value_bits[1] = 1
        kinds = None
    elif case == "score_high_bits":
        c.value_bits[1] = 1 << 32
    elif case == "unknown_kind":
        kinds = [3, 0]
    rc, _ = key_words(lib, kinds, orders, c)
    assert rc == ERR_INVALID
    # the same cursor with the offending field cleared is accepted
    ok = Cursor()
    ok.has_cursor = 1
    assert key_words(lib, None if kinds is None else [1, 0], orders, ok)[0] == 0


def test_cursor_struct_layout_matches_the_header(tmp_path):
    """slg_sort_cursor: the ctypes mirror (searchlite_amd/_native.py) and the Rust mirror (gpu/ffi.rs) against
    sizes and offsets from a C program compiled against include/searchlite_gpu.h."""
    from searchlite_amd import _native as N
    src = tmp_path / "cur.c"
    fields = ["has_cursor", "segment_ord", "doc_id", "missing_mask", "value_bits"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(slg_sort_cursor));\n' +
                   "".join(f'  printf("{f} %zu\\n", offsetof(slg_sort_cursor, {f}));\n' for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "cur"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(N.SortCursor) == C.sizeof(Cursor) == 48
    for f in fields:
        assert int(got[f]) == getattr(N.SortCursor, f).offset, f
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    m = re.search(r"pub struct slg_sort_cursor \{(.*?)\}", ffi, re.S)
    assert m is not None
    assert re.findall(r"pub\s+(\w+)\s*:", m.group(1)) == fields
