"""slg_vector_search_batch / _device argument checks that need no device: a NULL index fails with
SLG_ERR_INVALID and a message, before anything touches a GPU (searchlite-ffi conventions,
searchlite-ffi/src/lib.rs:24-43)."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def _args():
    nq, dim, k = 2, 4, 3
    keep = dict(cf=np.zeros(1, np.uint32), q=np.zeros((nq, dim), np.float32), a=np.zeros((nq, 1), np.float32),
                doc=np.zeros((nq, k), np.uint32), seg=np.zeros((nq, k), np.uint32),
                sc=np.zeros((nq, k), np.float32), vs=np.zeros((nq, k), np.float32),
                cnt=np.zeros(nq, np.uint32), tot=np.zeros(nq, np.uint64))
    p = {n: a.ctypes.data for n, a in keep.items()}
    return keep, (nq, 1, p["cf"], p["q"], p["a"], None, None, 5, k, p["doc"], p["seg"], p["sc"], p["vs"],
                  p["cnt"], p["tot"])


@pytest.mark.parametrize("name", ["slg_vector_search_batch", "slg_vector_search_batch_device"])
def test_null_index_is_invalid(lib, name):
    from searchlite_amd import _native as N
    keep, args = _args()
    assert getattr(lib, name)(None, *args) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error()
    assert lib.slg_last_error_code() == N.ERR_INVALID


@pytest.mark.parametrize("name", ["slg_vector_search_batch", "slg_vector_search_batch_device"])
def test_null_clause_field_is_invalid(lib, name):
    from searchlite_amd import _native as N
    keep, args = _args()
    args = list(args)
    args[2] = None
    assert getattr(lib, name)(None, *args) == N.ERR_INVALID
    assert lib.slg_last_error() != b""
