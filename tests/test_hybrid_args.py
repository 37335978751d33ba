"""The hybrid text + vector exports exist in the built library and the header, and the header, the ctypes
binding (searchlite_amd/_native.py) and the Rust mirror (integration/.../gpu/ffi.rs) agree on their
argument counts."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"slg_batch_prepare_hybrid": 9, "slg_batch_hybrid_device": 14, "slg_search_batch_hybrid": 22}


def _n_args(text, pattern):
    m = re.search(pattern, text, re.S)
    assert m, pattern
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    if not os.path.exists(_native.lib_path()):
        from searchlite_amd import build
        build.build_gpu()
    return _native.load()


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_export_and_argument_counts(lib, name):
    assert hasattr(lib, name), f"{name} is not exported"
    assert len(getattr(lib, name).argtypes) == EXPORTS[name]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "searchlite_gpu.h")).read(), flags=re.S)
    assert _n_args(header, r"\b%s\s*\((.*?)\)\s*;" % name) == EXPORTS[name]
    rs = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    assert _n_args(rs, r"pub fn %s\((.*?)\)\s*->" % name) == EXPORTS[name]


def test_null_handles_fail_cleanly(lib):
    from searchlite_amd import _native as N
    assert lib.slg_batch_prepare_hybrid(None, 0, None, None, None, None, None, 11, 1) is None
    assert lib.slg_last_error_code() == N.ERR_INVALID
    assert lib.slg_batch_hybrid_device(None, 1, None, None, None, None, 10, 10, None, None, None, None, None,
                                       None) == N.ERR_INVALID
    assert lib.slg_search_batch_hybrid(None, 0, None, None, None, None, None, 11, 1, 1, None, None, None, None,
                                       10, 10, None, None, None, None, None, None) == N.ERR_INVALID
