"""The argument checks of slg_batch_explain (csrc/slg_explain_host.hpp: what the entry point runs before any device
work) through its test C ABI (slgx_explain_check in lib/libslg_plan.so), against hand-made batch facts: every
SLG_ERR_INVALID and SLG_ERR_UNSUPPORTED of searchlite_gpu.h that needs no device, each limit at its value and one
above; the struct's layout against the header and the Rust mirror; the NULL batch through the library itself.  The
limits are read from the header.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from searchlite_amd import _native as N
from searchlite_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "searchlite_gpu.h")
FFI = os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")

NULL_BATCH, DETACHED, LAUNCHED, SCAN, HYBRID, NESTED, DEEP, RESCORE, SHARDED = (1 << i for i in range(9))
FIELDS = ("base_score", "final_score", "n_functions", "fn_type", "fn_field", "fn_value", "rescored", "rescore_score",
          "combined_score")
REQUIRED, RESCORE_ONLY = FIELDS[:6], FIELDS[6:]


def header_limit(name):
    m = re.search(r"#define\s+%s\s+(\d+)u" % name, open(HEADER).read())
    assert m, name
    return int(m.group(1))


MAX_ROWS, MAX_FUNCS = header_limit("SLG_MAX_EXPLAIN_ROWS"), header_limit("SLG_MAX_EXPLAIN_FUNCS")
MAX_TABLE = 2048  # rescore's LDS table (slg::kRescoreMaxTable): the issue's bound


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(build.build_plan_lib())


def out_with(names=REQUIRED):
    keep = np.zeros(16, np.uint32)
    return N.ExplainOut(**{n: keep.ctypes.data for n in names}), keep


def check(lib, flags=LAUNCHED, max_table=6, rows=10, out="default"):
    if out == "default":
        out, keep = out_with(FIELDS if flags & RESCORE else REQUIRED)
    err = C.create_string_buffer(512)
    rc = lib.slgx_explain_check(C.c_uint32(flags), C.c_uint32(max_table), C.c_uint32(rows),
                                None if out is None else C.byref(out), err, C.c_uint32(512))
    return rc, err.value.decode()


def test_the_limits_are_the_ones_the_issue_names_and_python_mirrors_them():
    assert (MAX_ROWS, MAX_FUNCS) == (1024, 9) and MAX_FUNCS == header_limit("SLG_MAX_FSCORE_FUNCS") + 1
    assert (N.MAX_EXPLAIN_ROWS, N.MAX_EXPLAIN_FUNCS) == (MAX_ROWS, MAX_FUNCS)
    text = open(HEADER).read()
    enum = re.search(r"enum \{ (SLG_EXPLAIN_WEIGHT = 0.*?) \};", text, re.S).group(1)
    values = dict(re.findall(r"(SLG_EXPLAIN_\w+) = (\d+)", enum))
    assert values == {"SLG_EXPLAIN_WEIGHT": "0", "SLG_EXPLAIN_FIELD_VALUE_FACTOR": "1", "SLG_EXPLAIN_DECAY_EXP": "2",
                      "SLG_EXPLAIN_DECAY_GAUSS": "3", "SLG_EXPLAIN_DECAY_LINEAR": "4", "SLG_EXPLAIN_SCRIPT_SCORE": "5"}
    assert (N.EXPLAIN_WEIGHT, N.EXPLAIN_FIELD_VALUE_FACTOR, N.EXPLAIN_DECAY_EXP, N.EXPLAIN_DECAY_GAUSS,
            N.EXPLAIN_DECAY_LINEAR, N.EXPLAIN_SCRIPT_SCORE) == (0, 1, 2, 3, 4, 5)
    ffi = open(FFI).read()
    for name, v in list(values.items()) + [("SLG_MAX_EXPLAIN_ROWS", "1024"), ("SLG_MAX_EXPLAIN_FUNCS", "9")]:
        assert re.search(r"pub const %s: u32 = %s;" % (name, v), ffi), name


def test_struct_layout_against_the_header_and_the_rust_mirror(tmp_path):
    """slg_explain_out as a C compiler lays it out: size and every field's offset; the field list of the header, of
    _native.py and of ffi.rs in one order"""
    body = re.search(r"typedef struct slg_explain_out \{(.*?)\} slg_explain_out;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    header_fields = re.findall(r"\*\s*(\w+)\s*;", body)
    assert tuple(header_fields) == FIELDS == tuple(n for n, _ in N.ExplainOut._fields_)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(slg_explain_out));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(slg_explain_out, {n}));\n' for n in FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    nums = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert nums[0] == C.sizeof(N.ExplainOut) == 72
    assert nums[1:] == [getattr(N.ExplainOut, n).offset for n in FIELDS]
    m = re.search(r"pub struct slg_explain_out \{(.*?)\}", open(FFI).read(), re.S)
    rust = re.findall(r"pub\s+(\w+)\s*:\s*\*mut\s+(\w+)", re.sub(r"//[^\n]*", "", m.group(1)))
    assert [n for n, _ in rust] == list(FIELDS)
    assert [t for _, t in rust] == ["c_float", "c_float", "u32", "u32", "i32", "c_float", "u32", "c_float", "c_float"]
    assert re.search(r"pub fn slg_batch_explain\(batch: \*mut slg_batch, rows: u32, out: \*const slg_explain_out\) -> c_int;",
                     open(FFI).read())


def test_a_valid_call(lib):
    assert check(lib) == (N.OK, "")
    assert check(lib, LAUNCHED | RESCORE) == (N.OK, "")
    assert check(lib, rows=MAX_ROWS, max_table=MAX_TABLE) == (N.OK, "")
    o, keep = out_with(FIELDS)  # the rescore arrays of a batch without rescore are left alone, given or not
    assert check(lib, out=o) == (N.OK, "")


@pytest.mark.parametrize("flags, what", [
    (NULL_BATCH | LAUNCHED, "batch is NULL or its index was destroyed"),
    (DETACHED | LAUNCHED, "batch is NULL or its index was destroyed"),
    (0, "the batch has not run"),
])
def test_invalid_batches(lib, flags, what):
    rc, msg = check(lib, flags)
    assert rc == N.ERR_INVALID and what in msg and msg.startswith("explain: ")


def test_null_out_and_zero_rows(lib):
    rc, msg = check(lib, out=None)
    assert rc == N.ERR_INVALID and "out is NULL" in msg
    rc, msg = check(lib, rows=0)
    assert rc == N.ERR_INVALID and "rows is 0" in msg


@pytest.mark.parametrize("missing", REQUIRED)
def test_every_required_array(lib, missing):
    o, keep = out_with([n for n in REQUIRED if n != missing])
    rc, msg = check(lib, out=o)
    assert rc == N.ERR_INVALID and missing in msg, msg


@pytest.mark.parametrize("missing", RESCORE_ONLY)
def test_a_rescore_batch_needs_its_three_arrays(lib, missing):
    o, keep = out_with([n for n in FIELDS if n != missing])
    rc, msg = check(lib, LAUNCHED | RESCORE, out=o)
    assert rc == N.ERR_INVALID and missing in msg, msg
    assert check(lib, LAUNCHED, out=o) == (N.OK, "")


@pytest.mark.parametrize("kwargs, what", [
    (dict(rows=MAX_ROWS + 1), "SLG_MAX_EXPLAIN_ROWS"),
    (dict(flags=LAUNCHED | SCAN), "scan batch"),
    (dict(flags=LAUNCHED | HYBRID), "hybrid batch"),
    (dict(flags=LAUNCHED | NESTED), "two-level or deeper score plan"),
    (dict(flags=LAUNCHED | DEEP), "two-level or deeper score plan"),
    (dict(max_table=MAX_TABLE + 1), "2049 term rows"),
    (dict(flags=LAUNCHED | SHARDED), "sharded"),
])
def test_unsupported_batches_name_the_reason(lib, kwargs, what):
    rc, msg = check(lib, **kwargs)
    assert rc == N.ERR_UNSUPPORTED and what in msg and "CPU scorer" in msg and msg.startswith("explain: "), msg


def test_an_invalid_argument_comes_before_an_unsupported_batch(lib):
    rc, msg = check(lib, SCAN, rows=MAX_ROWS + 1)  # not run, and unsupported twice over
    assert rc == N.ERR_INVALID and "has not run" in msg
    rc, msg = check(lib, LAUNCHED | SCAN, rows=0)
    assert rc == N.ERR_INVALID and "rows is 0" in msg


def test_the_library_refuses_a_null_batch_without_a_device():
    L = N.load()
    o, keep = out_with()
    assert L.slg_batch_explain(None, 10, C.addressof(o)) == N.ERR_INVALID
    assert b"batch is NULL" in L.slg_last_error() and L.slg_last_error_code() == N.ERR_INVALID
