"""slg_index_quantize_vector_field / slg_index_fetch_vector_copy / slg_vector_search_batch_approx[_device]: the
exports, their ctypes signatures against the header and the Rust mirror, the Python wrappers, and the argument
errors that need no device: refine is checked against cand_size and SLG_MAX_VECTOR_CANDIDATES before the index is
looked at, and a NULL index or NULL clause_field fails with SLG_ERR_INVALID and a message before anything touches a
GPU (as tests/test_vector_search_args.py does for the exact call)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCH = ["slg_vector_search_batch_approx", "slg_vector_search_batch_approx_device"]
vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
SIGS = {
    "slg_index_quantize_vector_field": [vp, u32],
    "slg_index_fetch_vector_copy": [vp, u32, u32, vp, vp, u32],
    SEARCH[0]: [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp],
    SEARCH[1]: [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp],
}


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def _n_args(text, pattern):
    m = re.search(pattern, text, re.S)
    assert m, pattern
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(SIGS))
def test_exports_and_signatures(lib, name):
    assert hasattr(lib, name), f"{name} is not exported"
    fn = getattr(lib, name)
    assert fn.restype is i32 and list(fn.argtypes) == SIGS[name]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "searchlite_gpu.h")).read(), flags=re.S)
    assert _n_args(header, r"\b%s\s*\((.*?)\)\s*;" % name) == len(SIGS[name])
    rs = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    assert _n_args(rs, r"pub fn %s\((.*?)\)\s*->" % name) == len(SIGS[name])


def test_refine_follows_cand_size_in_the_header(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "searchlite_gpu.h")).read(), flags=re.S)
    for name in SEARCH:
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, header, re.S).group(1)
        names = [a.split()[-1].lstrip("*") for a in args.split(",")]
        assert names[8:11] == ["cand_size", "refine", "k_out"]


def test_python_wrappers_exist():
    from searchlite_amd import GpuIndex
    for m in ("quantize_vector_field", "fetch_vector_copy", "vector_search_approx", "vector_search_approx_device"):
        assert callable(getattr(GpuIndex, m))


def _args(cand=5, refine=8):
    nq, dim, k = 2, 4, 3
    keep = dict(cf=np.zeros(1, np.uint32), q=np.zeros((nq, dim), np.float32), a=np.zeros((nq, 1), np.float32),
                doc=np.full((nq, k), 7, np.uint32), seg=np.full((nq, k), 7, np.uint32),
                sc=np.full((nq, k), 7, np.float32), vs=np.full((nq, k), 7, np.float32),
                cnt=np.full(nq, 7, np.uint32), tot=np.full(nq, 7, np.uint64))
    p = {n: a.ctypes.data for n, a in keep.items()}
    return keep, [nq, 1, p["cf"], p["q"], p["a"], None, None, cand, refine, k, p["doc"], p["seg"], p["sc"], p["vs"],
                  p["cnt"], p["tot"]]


def _untouched(keep):
    return all((keep[n] == 7).all() for n in ("doc", "seg", "sc", "vs", "cnt", "tot"))


@pytest.mark.parametrize("name", SEARCH)
@pytest.mark.parametrize("cand,refine", [(5, 4), (1, 0), (5, 10001), (10000, 10001), (5, 0xFFFFFFFF)])
def test_refine_outside_its_range_is_unsupported(lib, name, cand, refine):
    """refine < cand_size and refine above the cap: SLG_ERR_UNSUPPORTED, checked before the index (NULL here)"""
    from searchlite_amd import _native as N
    keep, args = _args(cand, refine)
    assert getattr(lib, name)(None, *args) == N.ERR_UNSUPPORTED
    assert b"refine" in lib.slg_last_error() and lib.slg_last_error_code() == N.ERR_UNSUPPORTED
    assert _untouched(keep)


@pytest.mark.parametrize("name", SEARCH)
@pytest.mark.parametrize("cand,refine", [(5, 5), (5, 8), (1, 10000), (10000, 10000)])
def test_valid_refine_reaches_the_index_check(lib, name, cand, refine):
    from searchlite_amd import _native as N
    keep, args = _args(cand, refine)
    assert getattr(lib, name)(None, *args) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error() and lib.slg_last_error_code() == N.ERR_INVALID
    assert _untouched(keep)


@pytest.mark.parametrize("name", SEARCH)
def test_null_clause_field_is_invalid(lib, name):
    from searchlite_amd import _native as N
    keep, args = _args()
    args[2] = None
    assert getattr(lib, name)(None, *args) == N.ERR_INVALID
    assert lib.slg_last_error() != b""


def test_quantize_and_fetch_on_a_null_index(lib):
    from searchlite_amd import _native as N
    assert lib.slg_index_quantize_vector_field(None, 0) == N.ERR_INVALID
    assert b"index is NULL" in lib.slg_last_error()
    assert lib.slg_index_fetch_vector_copy(None, 0, 0, None, None, 0) == N.ERR_INVALID
    assert b"index is NULL" in lib.slg_last_error()
