"""slg_index_train_vector_field: the export, its ctypes signature against the header and the Rust mirror, the two
structs and the two constants in header, mirror and Python, the Python wrapper, and the argument errors that need no
device: iters is checked before the index is looked at, and a NULL index fails with SLG_ERR_INVALID and a message
before anything touches a GPU (as tests/test_vector_ivf_args.py does for the calls it trains centroids for)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "slg_index_train_vector_field"
vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
SIG = [vp, u32, vp, u32, vp]


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    lib = _native.load()
    assert hasattr(lib, NAME), f"{NAME} is not exported"
    return lib


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _read("include", "searchlite_gpu.h"), flags=re.S)


def _rs():
    return _read("integration", "searchlite-core", "src", "gpu", "ffi.rs")


def _n_args(text, pattern):
    m = re.search(pattern, text, re.S)
    assert m, pattern
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_export_and_signature(lib):
    fn = getattr(lib, NAME)
    assert fn.restype is i32 and list(fn.argtypes) == SIG
    assert _n_args(_header(), r"\b%s\s*\((.*?)\)\s*;" % NAME) == len(SIG)
    assert _n_args(_rs(), r"pub fn %s\((.*?)\)\s*->" % NAME) == len(SIG)
    args = re.search(r"\b%s\s*\((.*?)\)\s*;" % NAME, _header(), re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["index", "field", "per_segment", "n_segs",
                                                                    "out_stats"]


def test_structs_and_constants_in_the_header_the_mirror_and_python():
    from searchlite_amd import _native as N
    header, rs = _read("include", "searchlite_gpu.h"), _rs()
    for name, value in (("MAX_VECTOR_TRAIN_ITERS", 256), ("VECTOR_TRAIN_CHUNK", 256)):
        h = re.search(r"#define\s+SLG_%s\s+(\w+)u\b" % name, header)
        assert h and int(h.group(1), 0) == value
        r = re.search(r"pub const SLG_%s: u32 = ([\w_]+);" % name, rs)
        assert r and int(r.group(1).replace("_", ""), 0) == value
        assert getattr(N, name) == value
    assert C.sizeof(N.VectorTrainDesc) == 16 and C.sizeof(N.VectorTrainStats) == 16
    assert [(n, getattr(N.VectorTrainDesc, n).offset) for n, _ in N.VectorTrainDesc._fields_] == \
        [("n_lists", 0), ("iters", 4), ("init", 8)]
    assert [n for n, _ in N.VectorTrainStats._fields_] == ["iters_run", "moved", "empty_lists", "max_len"]
    assert re.search(r"typedef struct \{\s*uint32_t n_lists;.*?uint32_t iters;.*?const float \*init;.*?\}\s*"
                     r"slg_vector_train_desc;", header, re.S)
    assert re.search(r"typedef struct \{ uint32_t iters_run, moved, empty_lists, max_len; \} slg_vector_train_stats;",
                     header)
    assert re.search(r"struct slg_vector_train_desc\s*\{\s*pub n_lists: u32,\s*pub iters: u32,\s*"
                     r"pub init: \*const c_float\s*\}", rs)
    assert re.search(r"struct slg_vector_train_stats\s*\{\s*pub iters_run: u32,\s*pub moved: u32,\s*"
                     r"pub empty_lists: u32,\s*pub max_len: u32\s*\}", rs)


def test_python_wrapper_exists_and_the_host_helper_points_to_it():
    from searchlite_amd import GpuIndex, ivf
    assert callable(getattr(GpuIndex, "train_vector_field"))
    assert "train_vector_field" in ivf.__doc__ and callable(ivf.train_centroids)


def _call(lib, descs, n_segs, with_stats=True):
    from searchlite_amd import _native as N
    stats = (N.VectorTrainStats * max(n_segs, 1))()
    C.memset(C.addressof(stats), 7, C.sizeof(stats))
    before = bytes(stats)
    rc = getattr(lib, NAME)(None, 0, C.addressof(descs) if descs is not None else None, n_segs,
                            C.addressof(stats) if with_stats else None)
    assert bytes(stats) == before, "out_stats was written on an error"
    return rc


def _descs(*rows):
    from searchlite_amd import _native as N
    d = (N.VectorTrainDesc * len(rows))()
    keep = np.zeros((4, 4), np.float32)
    for i, (n_lists, iters, init) in enumerate(rows):
        d[i].n_lists, d[i].iters, d[i].init = n_lists, iters, keep.ctypes.data if init else None
    return d, keep


@pytest.mark.parametrize("rows", [[(3, 257, True)], [(3, 257, False)], [(3, 0xFFFFFFFF, True)],
                                  [(0, 0, False), (4, 300, True)], [(65537, 257, True)]])
def test_iters_above_the_limit_is_unsupported_before_the_index_is_looked_at(lib, rows):
    """with a NULL index: the iters check comes first, also where n_lists is over its own limit"""
    from searchlite_amd import _native as N
    d, keep = _descs(*rows)
    for with_stats in (True, False):
        assert _call(lib, d, len(rows), with_stats) == N.ERR_UNSUPPORTED
        assert b"iters" in lib.slg_last_error() and lib.slg_last_error_code() == N.ERR_UNSUPPORTED


@pytest.mark.parametrize("rows", [[(3, 256, True)], [(3, 0, False)], [(0, 0, False)], [(0xFFFFFFFF, 0, False)],
                                  [(65537, 4, True)], [(0, 999, False), (0xFFFFFFFF, 999, False)]])
def test_a_null_index_is_invalid_otherwise(lib, rows):
    """iters within the limit (or on a segment that is not trained): the next check is the index"""
    from searchlite_amd import _native as N
    d, keep = _descs(*rows)
    assert _call(lib, d, len(rows)) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error() and lib.slg_last_error_code() == N.ERR_INVALID


def test_null_per_segment_with_a_null_index(lib):
    from searchlite_amd import _native as N
    assert _call(lib, None, 2) == N.ERR_INVALID and b"index" in lib.slg_last_error()
    assert _call(lib, None, 0) == N.ERR_INVALID and b"index" in lib.slg_last_error()
