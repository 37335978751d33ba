"""slg_batch_prepare_collapse / slg_batch_fetch_collapse / slg_search_batch_collapse argument checks that need no
device: the spec is checked before the index is looked at, a NULL index fails with SLG_ERR_INVALID and a message,
before anything touches a GPU; the header, the ctypes binding and the Rust mirror agree on the argument counts and
the spec's fields."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = {"slg_batch_prepare_collapse": 12, "slg_batch_fetch_collapse": 15, "slg_search_batch_collapse": 30}


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


def spec_of(field=0, group_limit=5, inner_from=0, inner_size=0, inner_sort=None):
    """-> (N.CollapseSpec, the inner sort spec it points to); inner_sort: None or (n_parts, fields, orders)"""
    from searchlite_amd import _native as N
    keep = None
    if inner_sort is not None:
        keep = N.SortSpec()
        keep.n_parts = inner_sort[0]
        for i, (f, o) in enumerate(zip(inner_sort[1], inner_sort[2])):
            keep.field[i], keep.order[i] = f, o
    return N.CollapseSpec(field, group_limit, inner_from, inner_size, None if keep is None else C.addressof(keep)), keep


def prepare(lib, spec, nq=2, k=11):
    offs = np.zeros(nq + 1, np.uint32)
    return lib.slg_batch_prepare_collapse(None, nq, offs.ctypes.data, None, None, None, None, None, None,
                                          None if spec is None else C.addressof(spec), k, 1)


def rejected(lib, spec, code, word, **kw):
    from searchlite_amd import _native as N
    sp, keep = spec if spec is not None else (None, None)
    assert prepare(lib, sp, **kw) is None
    assert lib.slg_last_error_code() == getattr(N, code), lib.slg_last_error()
    assert word.encode() in lib.slg_last_error(), lib.slg_last_error()


def _n_args(text, pattern):
    m = re.search(pattern, text, re.S)
    assert m, pattern
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(EXPORTS))
def test_export_and_argument_counts(lib, name):
    assert hasattr(lib, name), f"{name} is not exported"
    assert len(getattr(lib, name).argtypes) == EXPORTS[name]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "searchlite_gpu.h")).read(), flags=re.S)
    assert _n_args(header, r"\b%s\s*\((.*?)\)\s*;" % name) == EXPORTS[name]
    rs = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    assert _n_args(rs, r"pub fn %s\((.*?)\)\s*->" % name) == EXPORTS[name]


def test_spec_layout_matches_the_header_and_the_rust_mirror(tmp_path):
    import subprocess
    from searchlite_amd import _native as N
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %u %u\\n", sizeof(slg_collapse_spec),\n'
                   '         offsetof(slg_collapse_spec, field), offsetof(slg_collapse_spec, group_limit),\n'
                   '         offsetof(slg_collapse_spec, inner_from), offsetof(slg_collapse_spec, inner_size),\n'
                   '         offsetof(slg_collapse_spec, inner_sort), SLG_MAX_COLLAPSE_ROWS, SLG_MAX_INNER_HITS);\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, *offsets, max_rows, max_inner = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(N.CollapseSpec)
    assert offsets == [getattr(N.CollapseSpec, n).offset for n, _ in N.CollapseSpec._fields_]
    assert max_rows == N.MAX_COLLAPSE_ROWS == 4096 and max_inner == N.MAX_INNER_HITS == 64
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    body = re.search(r"pub struct slg_collapse_spec \{(.*?)\}", ffi, re.S).group(1)
    assert re.findall(r"pub\s+(\w+)\s*:", body) == [n for n, _ in N.CollapseSpec._fields_]
    assert "pub const SLG_MAX_COLLAPSE_ROWS: u32 = 4096;" in ffi and "pub const SLG_MAX_INNER_HITS: u32 = 64;" in ffi


def test_null_spec_and_null_index(lib):
    rejected(lib, None, "ERR_INVALID", "collapse spec is NULL")
    rejected(lib, spec_of(), "ERR_INVALID", "index is NULL")  # a valid spec: the index is looked at next
    rejected(lib, spec_of(), "ERR_INVALID", "index is NULL", nq=0)
    rejected(lib, spec_of(inner_size=3, inner_sort=(1, [-1], [1])), "ERR_INVALID", "index is NULL")


def test_group_limit(lib):
    rejected(lib, spec_of(group_limit=0), "ERR_INVALID", "group_limit")
    rejected(lib, spec_of(group_limit=12), "ERR_INVALID", "group_limit", k=11)
    rejected(lib, spec_of(group_limit=11), "ERR_INVALID", "index is NULL", k=11)
    rejected(lib, spec_of(group_limit=1), "ERR_INVALID", "index is NULL", k=1)


def test_k_limit(lib):
    from searchlite_amd import _native as N
    big = N.MAX_COLLAPSE_ROWS
    rejected(lib, spec_of(group_limit=big), "ERR_INVALID", "index is NULL", k=big)
    rejected(lib, spec_of(), "ERR_UNSUPPORTED", "SLG_MAX_COLLAPSE_ROWS", k=big + 1)
    # an invalid argument is reported before an unsupported one
    rejected(lib, spec_of(group_limit=0), "ERR_INVALID", "group_limit", k=big + 1)


def test_inner_hits_limit(lib):
    from searchlite_amd import _native as N
    m = N.MAX_INNER_HITS
    rejected(lib, spec_of(inner_from=0, inner_size=m), "ERR_INVALID", "index is NULL")
    rejected(lib, spec_of(inner_from=m - 1, inner_size=1), "ERR_INVALID", "index is NULL")
    rejected(lib, spec_of(inner_from=0, inner_size=m + 1), "ERR_UNSUPPORTED", "SLG_MAX_INNER_HITS")
    rejected(lib, spec_of(inner_from=m, inner_size=1), "ERR_UNSUPPORTED", "SLG_MAX_INNER_HITS")
    rejected(lib, spec_of(inner_from=0xFFFFFFFF, inner_size=2), "ERR_UNSUPPORTED", "SLG_MAX_INNER_HITS")
    rejected(lib, spec_of(inner_from=1000, inner_size=0), "ERR_INVALID", "index is NULL")  # no inner hits: no limit


def test_inner_sort(lib):
    from searchlite_amd import _native as N
    n = N.MAX_SORT_PARTS
    rejected(lib, spec_of(inner_size=2, inner_sort=(n, [0, 1, 2, -1], [0, 1, 0, 1])), "ERR_INVALID", "index is NULL")
    rejected(lib, spec_of(inner_size=2, inner_sort=(0, [], [])), "ERR_INVALID", "index is NULL")  # `_score` desc
    rejected(lib, spec_of(inner_size=2, inner_sort=(n + 1, [0] * n, [0] * n)), "ERR_UNSUPPORTED", "inner sort parts")
    rejected(lib, spec_of(inner_size=2, inner_sort=(2, [0, 0], [0, 2])), "ERR_INVALID", "sort order")
    rejected(lib, spec_of(inner_size=2, inner_sort=(1, [0], [-1])), "ERR_INVALID", "sort order")
    rejected(lib, spec_of(inner_size=2, inner_sort=(2, [0, -2], [0, 0])), "ERR_INVALID", "sort field")
    # an invalid argument is reported before an unsupported one
    rejected(lib, spec_of(inner_size=2, inner_sort=(n + 1, [0] * n, [0, 0, 7, 0])), "ERR_INVALID", "sort order")


def test_other_entries_null_arguments(lib):
    from searchlite_amd import _native as N
    assert lib.slg_batch_fetch_collapse(*[None] * 15) == N.ERR_INVALID
    assert b"batch" in lib.slg_last_error()
    sp, keep = spec_of()
    tail = [None] * 18
    assert lib.slg_search_batch_collapse(None, 0, None, None, None, None, None, None, None, C.addressof(sp), 11, 1,
                                         *tail) == N.ERR_INVALID
    assert b"index" in lib.slg_last_error()
    assert lib.slg_search_batch_collapse(None, 0, None, None, None, None, None, None, None, None, 11, 1,
                                         *tail) == N.ERR_INVALID
    assert b"collapse spec is NULL" in lib.slg_last_error()


def test_python_layer_refuses_the_kinds_collapse_is_not_built_on():
    """the library's other prepare calls take no collapse spec: PreparedBatch refuses the combination itself,
    before it touches the index"""
    from searchlite_amd import _native as N
    from searchlite_amd.searcher import PreparedBatch

    class NoIndex:
        _lib = None
    offs = np.zeros(2, np.uint32)
    for kind in ("hybrid", "aggs", "rescore", "clauses", "phrases", "fscore"):
        with pytest.raises(N.SlgError) as ei:
            PreparedBatch(NoIndex(), offs, np.zeros(0, np.uint32), np.zeros(0, np.float32), 11, 1,
                          collapse=dict(field=0, group_limit=5), **{kind: True if kind == "hybrid" else {}})
        assert ei.value.code == N.ERR_UNSUPPORTED and "collapse" in ei.value.msg
