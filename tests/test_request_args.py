"""slg_batch_prepare_request argument checks that need no device: the struct and the request are checked before
the index is looked at; every combination the header lists as refused comes back with SLG_ERR_UNSUPPORTED and a
message that names the pair; each kind's own malformed spec reports through the new entry what it reports through its
own; the header, the ctypes binding and the Rust mirror agree on the struct and the argument count.  (That a request
with one kind set is that kind's legacy batch is shown on the device, byte for byte:
tests/test_gpu_request.py::test_one_kind_through_the_request_is_the_legacy_batch.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import bool_ref as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NQ = 2


@pytest.fixture(scope="module")
def lib():
    from searchlite_amd import _native
    return _native.load()


class Specs:
    """one valid spec per kind for a batch of NQ queries without scored terms, and everything they point into"""

    def __init__(self):
        from searchlite_amd import _native as N, searcher as S
        from searchlite_amd.script import compile_script, script_spec
        self.keep = []
        self.offs = np.zeros(NQ + 1, np.uint32)
        cl = B.clauses_of([([(B.MUST, [0]), (B.SHOULD, [1, 2])], 1)] * NQ, 1)
        self.sort = S.sort_spec([(0, "asc"), ("_score", "desc")])
        self.q_cursor = (N.SortCursor * NQ)()
        self.bool_spec = self.made(S.bool_spec(cl, NQ))
        self.term_groups = self.made(S.bool_spec({n: v for n, v in cl.items() if n != "q_min_should"}, NQ))  # of a phrase batch
        from tests.phrase_ref import phrases_of
        self.phrase_spec = self.made(S.phrase_spec(phrases_of([([(B.MUST, 0, [[0, 1]])], 0)] * NQ, 1), NQ))
        from searchlite_amd.booltree import compile_matchers
        self.bool_tree_spec = self.made(S.bool_tree_spec(compile_matchers([{"bool": {"must": [{"term": [1]}]}}] * NQ, 1), NQ))
        self.fscore_spec = self.made(S.fscore_spec([dict(functions=[dict(kind="weight", weight=2.0)])] * NQ, NQ))
        self.script_spec = self.made(script_spec([dict(program=compile_script("_score * 2", None, {}), boost=1.0)] * NQ, NQ))
        from searchlite_amd import aggs as A
        fields = {"tag": {"id": 0, "keys": ["a", "b"]}, "x": {"id": 1}}
        self.plans = {n: A.agg_spec(req, fields) for n, req in {
            "aggs": {"t": {"type": "terms", "field": "tag"}},
            "top_hits": {"h": {"type": "top_hits", "size": 2}},
            "composite": {"c": {"type": "composite", "size": 2, "sources": [{"type": "terms", "name": "tag", "field": "tag"}]}},
            "term_buckets": {"s": {"type": "significant_terms", "field": "tag", "size": 2}}}.items()}
        self.aggs = self.plans["aggs"].spec
        self.top_hits = self.plans["top_hits"].top_hits
        self.composite = self.plans["composite"].composite["spec"]
        self.term_buckets = self.plans["term_buckets"].term_buckets["spec"]
        rs_offs = np.zeros(NQ + 1, np.uint32)
        self.rescore = self.made(S.rescore_spec(dict(q_offsets=rs_offs, q_terms=np.zeros((0, 1), np.uint32),
                                                     q_weights=np.zeros(0, np.float32), window=3), NQ))
        self.collapse = self.made(S.collapse_spec(dict(field=0, group_limit=5)))

    def made(self, pair):
        self.keep.append(pair[1])
        return pair[0]

    def request(self, *kinds, **over):
        from searchlite_amd import _native as N
        r = N.Request()
        r.struct_size, r.nq, r.q_offsets, r.k, r.strategy = C.sizeof(N.Request), NQ, self.offs.ctypes.data, 11, 1
        for name in kinds:
            setattr(r, name, C.addressof(getattr(self, name)))
        for name, v in over.items():
            setattr(r, name, v)
        return r


@pytest.fixture(scope="module")
def SP():
    return Specs()


def refused(lib, req, code, *words):
    from searchlite_amd import _native as N
    assert lib.slg_batch_prepare_request(None, None if req is None else C.addressof(req)) is None
    assert lib.slg_last_error_code() == getattr(N, code), lib.slg_last_error()
    for word in words:
        assert word.encode() in lib.slg_last_error(), (word, lib.slg_last_error())


def test_export_and_argument_count(lib):
    assert hasattr(lib, "slg_batch_prepare_request") and len(lib.slg_batch_prepare_request.argtypes) == 2
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "searchlite_gpu.h")).read(), flags=re.S)
    m = re.search(r"\bslg_batch_prepare_request\s*\((.*?)\)\s*;", header, re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 2
    rs = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    m = re.search(r"pub fn slg_batch_prepare_request\((.*?)\)\s*->", rs, re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 2


def test_struct_layout_matches_the_header_and_the_rust_mirror(tmp_path):
    from searchlite_amd import _native as N
    names = [n for n, _ in N.Request._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(slg_request));\n' +
                   "".join(f'  printf("%zu\\n", offsetof(slg_request, {n}));\n' for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, *offsets = map(int, subprocess.check_output([str(exe)], text=True).split())
    assert size == C.sizeof(N.Request)
    assert offsets == [getattr(N.Request, n).offset for n in names]
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    body = re.sub(r"//[^\n]*", "", re.search(r"pub struct slg_request \{(.*?)\}", ffi, re.S).group(1))
    assert re.findall(r"pub\s+(\w+)\s*:", body) == names
    # every pointer of the header's struct is a member the ctypes mirror has, in the header's order
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "searchlite_gpu.h")).read(), flags=re.S)
    members = re.search(r"typedef struct slg_request \{(.*?)\} slg_request;", header, re.S).group(1)
    assert re.findall(r"(\w+)\s*;", members) == names


def test_null_request_wrong_size_and_null_index(lib, SP):
    refused(lib, None, "ERR_INVALID", "req is NULL")
    for size in (0, 8, C.sizeof(SP.request()) - 8, C.sizeof(SP.request()) + 8):
        refused(lib, SP.request(struct_size=size), "ERR_INVALID", "struct_size")
    refused(lib, SP.request(reserved=1), "ERR_INVALID", "reserved")
    refused(lib, SP.request("q_cursor", "aggs", reserved=7), "ERR_INVALID", "reserved")  # before the combination
    refused(lib, SP.request(), "ERR_INVALID", "index is NULL")  # a plain request: the index is looked at next
    refused(lib, SP.request(nq=0), "ERR_INVALID", "index is NULL")
    every_legal = ("sort", "bool_spec", "fscore_spec", "script_spec", "aggs", "top_hits", "collapse")
    refused(lib, SP.request(*every_legal), "ERR_INVALID", "index is NULL")
    refused(lib, SP.request("phrase_spec", "q_cursor", "collapse", bool_spec=C.addressof(SP.term_groups)), "ERR_INVALID",
            "index is NULL")
    refused(lib, SP.request("bool_tree_spec", "rescore"), "ERR_INVALID", "index is NULL")
    refused(lib, SP.request("sort", "q_cursor", "script_spec", script_order=1), "ERR_INVALID", "index is NULL")


COLLECTORS = ("aggs", "top_hits", "composite", "term_buckets")
PAIRS = [("bool_tree_spec", "bool_spec"), ("bool_tree_spec", "phrase_spec"),
         ("top_hits", "composite"), ("top_hits", "term_buckets"), ("composite", "term_buckets")] + \
        [("q_cursor", c) for c in COLLECTORS] + \
        [("rescore", o) for o in ("sort", "q_cursor", "fscore_spec", "script_spec", "collapse") + COLLECTORS]


@pytest.mark.parametrize("pair", PAIRS, ids="+".join)
def test_refused_combinations_name_the_pair(lib, SP, pair):
    refused(lib, SP.request(*pair), "ERR_UNSUPPORTED", *pair)
    # also beside other, legal kinds, and whatever the order of the struct's members
    if "rescore" not in pair and "fscore_spec" not in pair:
        refused(lib, SP.request("fscore_spec", *reversed(pair)), "ERR_UNSUPPORTED", *pair)


def test_phrase_with_its_bool_spec_is_one_clause_kind(lib, SP):
    groups = C.addressof(SP.term_groups)
    refused(lib, SP.request("phrase_spec", bool_spec=groups), "ERR_INVALID", "index is NULL")
    refused(lib, SP.request("phrase_spec", "bool_tree_spec", bool_spec=groups), "ERR_UNSUPPORTED", "bool_tree_spec", "phrase_spec")
    # (the phrase spec states minimum_should_match: the kind's own check, through the new entry as through its own)
    refused(lib, SP.request("phrase_spec", "bool_spec"), "ERR_INVALID", "q_min_should")


def test_script_order_is_read_only_with_a_script(lib, SP):
    refused(lib, SP.request("fscore_spec", script_order=7), "ERR_INVALID", "index is NULL")
    refused(lib, SP.request("script_spec", script_order=7), "ERR_INVALID", "script")


def test_each_kinds_malformed_spec_reports_its_own_error(lib, SP):
    """the same code and message as the kind's own prepare call, also beside other kinds; an invalid argument is
    reported before an unsupported combination"""
    from searchlite_amd import _native as N

    def legacy(entry, *args):
        assert getattr(lib, entry)(None, NQ, SP.offs.ctypes.data, None, None, None, None, *args, 11, 1) is None
        return lib.slg_last_error_code(), lib.slg_last_error()

    def through_request(req):
        assert lib.slg_batch_prepare_request(None, C.addressof(req)) is None
        return lib.slg_last_error_code(), lib.slg_last_error()

    bad_bool = N.BoolSpec()                                    # every array NULL
    bad_collapse = N.CollapseSpec(0, 0, 0, 0, None)            # group_limit 0
    bad_aggs = N.AggSpec()
    bad_aggs.n_nodes = 99
    bad_fscore, bad_rescore, bad_phrase, bad_tree, bad_script = N.FscoreSpec(), N.RescoreSpec(), N.PhraseSpec(), N.BoolTreeSpec(), N.ScriptSpec()
    bad_top_hits = N.TopHitsSpec()                             # no node
    bad_composite, bad_buckets = N.CompositeSpec(), N.TermBucketSpec()  # no source, no node
    a = C.addressof
    cases = [
        ("top_hits", bad_top_hits, legacy("slg_batch_prepare_top_hits", None, None, a(bad_top_hits))),
        ("composite", bad_composite, legacy("slg_batch_prepare_composite", None, None, a(bad_composite))),
        ("term_buckets", bad_buckets, legacy("slg_batch_prepare_term_buckets", None, None, a(bad_buckets))),
        ("bool_spec", bad_bool, legacy("slg_batch_prepare_bool", None, a(bad_bool))),
        ("collapse", bad_collapse, legacy("slg_batch_prepare_collapse", None, None, a(bad_collapse))),
        ("aggs", bad_aggs, legacy("slg_batch_prepare_aggs", None, a(bad_aggs))),
        ("fscore_spec", bad_fscore, legacy("slg_batch_prepare_fscore", None, a(bad_fscore))),
        ("rescore", bad_rescore, legacy("slg_batch_prepare_rescore", a(bad_rescore))),
        ("phrase_spec", bad_phrase, legacy("slg_batch_prepare_phrase", None, None, a(bad_phrase))),
        ("bool_tree_spec", bad_tree, legacy("slg_batch_prepare_bool_tree", None, a(bad_tree))),
        ("script_spec", bad_script, legacy("slg_batch_prepare_script", None, a(bad_script), None, 0)),
    ]
    for name, spec, (code, msg) in cases:
        assert code in (N.ERR_INVALID, N.ERR_UNSUPPORTED) and msg and b"index is NULL" not in msg, (name, msg)
        assert through_request(SP.request(**{name: a(spec)})) == (code, msg), name
        if name not in ("rescore", "bool_tree_spec"):  # beside another kind
            assert through_request(SP.request("bool_tree_spec", **{name: a(spec)})) == (code, msg), name
    # (a sort spec and a cursor are checked against the index, behind the NULL-index check, here as in their own
    #  prepare calls: tests/test_gpu_request.py::test_sort_and_cursor_errors_behind_the_index)
    # an invalid spec beside an unsupported pair: the invalid argument is the one reported
    assert through_request(SP.request("q_cursor", "aggs", collapse=a(bad_collapse)))[0] == N.ERR_INVALID


def test_python_layer_passes_every_kind_and_leaves_the_refusals_to_the_library():
    """GpuIndex.prepare_request asks for every kind that is given; PreparedBatch refuses nothing itself there"""
    from searchlite_amd import _native as N
    from searchlite_amd.searcher import PreparedBatch

    class NoIndex:
        _lib, _h = N.load(), None
        _batches = set()
    offs = np.zeros(NQ + 1, np.uint32)
    cl = B.clauses_of([([(B.MUST, [0])], 0)] * NQ, 1)
    args = (NoIndex(), offs, np.zeros((0, 1), np.uint32), np.zeros(0, np.float32), 11, 1)
    with pytest.raises(N.SlgError) as ei:  # legal: reaches the index
        PreparedBatch(*args, clauses=cl, fscore=[None] * NQ, collapse=dict(field=0, group_limit=5), request=True)
    assert ei.value.code == N.ERR_INVALID and "index is NULL" in ei.value.msg
    with pytest.raises(N.SlgError) as ei:  # the legacy path still refuses the pair itself, with its own text
        PreparedBatch(*args, clauses=cl, collapse=dict(field=0, group_limit=5))
    assert ei.value.code == N.ERR_UNSUPPORTED and "collapse is not built on" in ei.value.msg
    with pytest.raises(N.SlgError) as ei:  # refused by the library, naming the pair
        PreparedBatch(*args, clauses=cl, cursors=[None] * NQ, aggs=Specs().aggs, request=True)
    assert ei.value.code == N.ERR_UNSUPPORTED and "q_cursor" in ei.value.msg and "aggs" in ei.value.msg
