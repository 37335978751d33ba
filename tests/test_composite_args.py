"""The composite aggregation's ABI and host mappings, without a device: the new structs against a compiled C probe,
every rejection of slg_batch_prepare_composite that needs no index with its error code, agg_spec's ValueErrors, and
composite_lower_bound against a brute-force tuple comparison, exhaustively over small layouts."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import composite_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def N():
    from searchlite_amd import _native
    return _native


@pytest.fixture(scope="module")
def lib(N):
    return N.load()


def test_structs_match_the_header(N, tmp_path):
    structs = {"slg_composite_source": N.CompositeSource, "slg_composite_spec": N.CompositeSpec,
               "slg_composite_source_layout": N.CompositeSourceLayout, "slg_composite_layout": N.CompositeLayout}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));\n')
        for f, _ in cls._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {f}));\n')
        lines.append('  printf("\\n");\n')
    lines.append('  printf("limits %u %u %d %d %zu\\n", SLG_MAX_COMPOSITE_SOURCES, SLG_MAX_COMPOSITE_SIZE, '
                 'SLG_COMPOSITE_TERMS, SLG_COMPOSITE_HISTOGRAM, sizeof(slg_agg_node));\n')
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "searchlite_gpu.h"\nint main(void) {\n' +
                   "".join(lines) + "  return 0;\n}\n")
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]]
           for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    ffi = open(os.path.join(ROOT, "integration", "searchlite-core", "src", "gpu", "ffi.rs")).read()
    for cname, cls in structs.items():
        size, *offsets = got[cname]
        assert size == C.sizeof(cls), cname
        assert offsets == [getattr(cls, f).offset for f, _ in cls._fields_], cname
        body = re.search(r"pub struct %s \{(.*?)\}" % cname, ffi, re.S).group(1)  # (the Rust mirror: the same fields)
        assert re.findall(r"pub\s+(\w+)\s*:", body) == [f for f, _ in cls._fields_], cname
    assert got["limits"] == [N.MAX_COMPOSITE_SOURCES, N.MAX_COMPOSITE_SIZE, N.COMPOSITE_TERMS, N.COMPOSITE_HISTOGRAM, 368]


def test_set_capacity(N):
    # a power of two, at least twice size + 1, never below the smallest set
    for size in (1, 3, 254, 255, 256, 1023, 1024):
        cap = N.composite_cap(size)
        assert cap & (cap - 1) == 0 and cap >= max(N.COMPOSITE_MIN_CAP, 2 * (size + 1)) and \
            (cap == N.COMPOSITE_MIN_CAP or cap // 2 < 2 * (size + 1))


# ---- rejections without an index ------------------------------------------------------------------------------------
def spec_of(N, sources=((0, 0, 0.0),), size=10, children=()):
    s = N.CompositeSpec()
    s.n_sources, s.size = len(sources), size
    for i, (kind, field, interval) in enumerate(sources[:N.MAX_COMPOSITE_SOURCES]):
        s.sources[i].kind, s.sources[i].field, s.sources[i].interval = kind, field, interval
    s.n_children = len(children)
    for i, fill in enumerate(children[:N.MAX_AGGS]):
        s.children[i].parent = 99  # (not read)
        fill(s.children[i])
    return s


def prepare(lib, cp, aggs=None, nq=2, k=5):
    offs = np.zeros(nq + 1, np.uint32)
    return lib.slg_batch_prepare_composite(None, nq, offs.ctypes.data, None, None, None, None, None,
                                           None if aggs is None else C.addressof(aggs),
                                           None if cp is None else C.addressof(cp), k, 1)


def fails(lib, N, cp, code, word, aggs=None):
    assert not prepare(lib, cp, aggs)
    assert lib.slg_last_error_code() == getattr(N, code), lib.slg_last_error()
    assert word.encode() in lib.slg_last_error(), lib.slg_last_error()


def kind(k, **kw):
    def fill(n):
        n.kind = k
        for name, v in kw.items():
            setattr(n, name, v)
    return fill


def test_rejections_without_an_index(lib, N):
    T, H = N.COMPOSITE_TERMS, N.COMPOSITE_HISTOGRAM
    fails(lib, N, None, "ERR_INVALID", "composite spec is NULL")
    fails(lib, N, spec_of(N, sources=()), "ERR_INVALID", "at least one source")
    fails(lib, N, spec_of(N, sources=((2, 0, 1.0),)), "ERR_INVALID", "unknown kind")
    for bad in (0.0, -1.0, math.inf, math.nan):
        fails(lib, N, spec_of(N, sources=((T, 0, 0.0), (H, 1, bad))), "ERR_INVALID", "interval")
    fails(lib, N, spec_of(N, children=(kind(10),)), "ERR_INVALID", "unknown kind")  # (10 is no kind)
    fails(lib, N, spec_of(N, children=(kind(7),)), "ERR_INVALID", "unknown kind")
    # a child with a defect slg_batch_prepare_aggs rejects
    fails(lib, N, spec_of(N, children=(kind(N.AGG_HISTOGRAM, interval=0.0),)), "ERR_INVALID", "interval")
    fails(lib, N, spec_of(N, children=(kind(N.AGG_RANGE, n_ranges=0),)), "ERR_INVALID", "at least one range")
    fails(lib, N, spec_of(N, children=(kind(N.AGG_STATS, has_missing=1, missing=math.nan),)), "ERR_INVALID", "missing")
    fails(lib, N, spec_of(N, children=(kind(N.AGG_FILTER, filter=-1),)), "ERR_INVALID", "filter id")
    # unsupported comes behind invalid: both defects, the invalid one is reported
    fails(lib, N, spec_of(N, sources=((2, 0, 1.0),), size=0), "ERR_INVALID", "unknown kind")
    fails(lib, N, spec_of(N, sources=((T, 0, 0.0),) * 5), "ERR_UNSUPPORTED", "SLG_MAX_COMPOSITE_SOURCES")
    fails(lib, N, spec_of(N, size=0), "ERR_UNSUPPORTED", "size is 0")
    fails(lib, N, spec_of(N, size=N.MAX_COMPOSITE_SIZE + 1), "ERR_UNSUPPORTED", "SLG_MAX_COMPOSITE_SIZE")
    fails(lib, N, spec_of(N, children=(kind(N.AGG_STATS),) * (N.MAX_AGGS + 1)), "ERR_UNSUPPORTED", "SLG_MAX_AGGS")
    for k in (N.AGG_CARDINALITY, N.AGG_PERCENTILES, N.AGG_PERCENTILE_RANKS):
        fails(lib, N, spec_of(N, children=(kind(N.AGG_STATS), kind(k, n_ranges=1))), "ERR_UNSUPPORTED", "not built under")
    # the aggregation spec's own checks come first
    bad_aggs = N.AggSpec()
    bad_aggs.n_nodes = 1
    bad_aggs.nodes[0].kind, bad_aggs.nodes[0].parent = 10, -1
    fails(lib, N, None, "ERR_INVALID", "agg node 0", aggs=bad_aggs)
    # a valid spec gets as far as the index
    fails(lib, N, spec_of(N, sources=((T, 0, 0.0), (H, 1, 0.5)), size=N.MAX_COMPOSITE_SIZE,
                          children=(kind(N.AGG_STATS), kind(N.AGG_TERMS))), "ERR_INVALID", "index is NULL")


def test_other_kinds_refuse_the_calls(lib, N):
    lay = N.CompositeLayout()
    assert lib.slg_batch_composite_layout(None, C.addressof(lay)) == N.ERR_INVALID
    assert lib.slg_batch_set_composite_after(None, None) == N.ERR_INVALID
    assert lib.slg_batch_fetch_composite(None, None, None, None) == N.ERR_INVALID


# ---- agg_spec ---------------------------------------------------------------------------------------------------
FIELDS = {"tag": {"id": 0, "keys": ["b", "a", "é", "ab"]}, "x": {"id": 1}, "dup": {"id": 2, "keys": ["a", "b", "a"]}}
SRC_T = {"type": "terms", "name": "t", "field": "tag"}
SRC_H = {"type": "histogram", "name": "h", "field": "x", "interval": 0.5}


def test_agg_spec_builds_the_plan(N):
    from searchlite_amd import aggs as A
    plan = A.agg_spec({"cmp": {"type": "composite", "sources": [SRC_T, SRC_H], "size": 7, "after": {"t": "a"},
                               "aggs": {"s": {"type": "stats", "field": "x"}, "k": {"type": "terms", "field": "tag"}}},
                       "other": {"type": "stats", "field": "x"}}, FIELDS)
    cp = plan.composite
    assert plan.spec.n_nodes == 1 and cp["name"] == "cmp" and cp["size"] == 7 and cp["after"] == {"t": "a"}
    assert cp["spec"].n_sources == 2 and cp["spec"].size == 7 and cp["spec"].n_children == 2
    assert [s["name"] for s in cp["sources"]] == ["t", "h"]
    assert cp["sources"][0]["sorted_keys"] == ["a", "ab", "b", "é"] and cp["sources"][0]["rank"].tolist() == [2, 0, 3, 1]
    assert cp["spec"].sources[0].kind == N.COMPOSITE_TERMS and cp["spec"].sources[1].kind == N.COMPOSITE_HISTOGRAM
    assert cp["spec"].sources[1].interval == 0.5 and cp["spec"].sources[1].field == 1
    assert [n["name"] for n in cp["children"].nodes] == ["k", "s"]  # (name order, as any children)
    assert cp["spec"].children[0].kind == N.AGG_TERMS and cp["spec"].children[1].kind == N.AGG_STATS


def test_shape_renders_the_page(N):
    """a hand-made page through aggs.shape: keys unpacked (a terms slot through the byte order, a histogram slot to
    -0.0 or id * interval), children shaped as any bucket's, after_key only with has_more"""
    from searchlite_amd import aggs as A
    plan = A.agg_spec({"cmp": {"type": "composite", "sources": [SRC_T, SRC_H], "size": 3,
                               "aggs": {"s": {"type": "stats", "field": "x"}}}}, FIELDS)
    # h: ids -1 .. 1 and the -0.0 slot: slots 0 (-0.5), 1 (-0.0), 2 (0.0), 3 (0.5); t: 4 keys
    lay = dict(n_sources=2, size=3, key_bits=4, count_offset=0,
               sources=[dict(shift=2, bits=2, slots=4, first_id=0, zero_slot=-1),
                        dict(shift=0, bits=2, slots=4, first_id=-1, zero_slot=1)],
               children=[dict(parent_rows=3, rows=1, first_id=0, is_stats=True, is_values=False, offset=0)])
    stats = np.zeros((1, 3, 1), A.STATS_DTYPE)
    stats[0, 0, 0] = (2, 1.0, 3.0, 4.0)
    page = dict(keys=np.array([[(1 << 2) | 1, (1 << 2) | 2, (3 << 2) | 3]], np.uint64), n_buckets=np.array([3], np.uint32),
                has_more=np.array([1], np.uint32), counts=np.array([[5, 1, 2]], np.uint64), children=[stats])
    got = A.shape(plan, [], [], 0, composite=(lay, page))["cmp"]
    keys = [b["key"] for b in got["buckets"]]
    assert [k["t"] for k in keys] == ["ab", "ab", "é"] and [k["h"] for k in keys] == [0.0, 0.0, 0.5]
    assert math.copysign(1.0, keys[0]["h"]) == -1.0 and math.copysign(1.0, keys[1]["h"]) == 1.0
    assert [b["doc_count"] for b in got["buckets"]] == [5, 1, 2] and got["after_key"] == keys[2]
    assert got["buckets"][0]["aggregations"]["s"] == {"type": "stats", "count": 2, "min": 1.0, "max": 3.0, "sum": 4.0, "avg": 2.0}
    page["has_more"][0] = 0
    assert "after_key" not in A.shape(plan, [], [], 0, composite=(lay, page))["cmp"]
    # the bound behind the last key of the page is that key + 1; behind (é, 0.5), the last possible key, nothing
    assert A.composite_lower_bound(lay, plan, keys[1]) == ((1 << 2) | 2) + 1
    assert A.composite_lower_bound(lay, plan, {"t": "é", "h": 0.5}) == 1 << 4


@pytest.mark.parametrize("request_, word", [
    ({"c": {"type": "composite", "sources": [{"type": "terms", "name": "d", "field": "dup"}], "size": 3}}, "twice"),
    ({"p": {"type": "terms", "field": "tag", "aggs": {"c": {"type": "composite", "sources": [SRC_T], "size": 3}}}}, "below"),
    ({"a": {"type": "composite", "sources": [SRC_T], "size": 3},
      "b": {"type": "composite", "sources": [SRC_T], "size": 3}}, "second composite"),
    ({"c": {"type": "composite", "sources": [SRC_T], "size": 3, "sampling": {"probability": 0.5}}}, "sampling"),
    ({"c": {"type": "composite", "sources": [SRC_T], "size": 3,
            "aggs": {"d": {"type": "derivative", "buckets_path": "_count"}}}}, "not built"),
    ({"c": {"type": "composite", "sources": [SRC_T], "size": 3, "aggs": {"h": {"type": "top_hits", "size": 1}}}}, "top_hits"),
    ({"c": {"type": "composite", "sources": [SRC_T], "size": 3, "aggs": {"n": {"type": "cardinality", "field": "tag"}}}},
     "cardinality"),
    ({"c": {"type": "composite", "sources": [SRC_T], "size": 3,
            "aggs": {"n": {"type": "percentiles", "field": "x"}}}}, "percentiles"),
    ({"c": {"type": "composite", "sources": [SRC_T], "size": 3,
            "aggs": {"k": {"type": "terms", "field": "tag", "aggs": {"s": {"type": "stats", "field": "x"}}}}}}, "one level"),
    ({"c": {"type": "composite", "sources": [SRC_T], "size": 0}}, "size"),
    ({"c": {"type": "composite", "sources": [SRC_T], "size": 1025}}, "size"),
    ({"c": {"type": "composite", "sources": [SRC_T] * 5, "size": 3}}, "sources"),
    ({"c": {"type": "composite", "sources": [{"type": "date_histogram", "name": "d", "field": "x"}], "size": 3}}, "source type"),
])
def test_agg_spec_value_errors(request_, word):
    from searchlite_amd import aggs as A
    with pytest.raises(ValueError, match=word):
        A.agg_spec(request_, FIELDS)


# ---- composite_lower_bound, exhaustively -------------------------------------------------------------------------
TERM_KEYS = ["b", "d", "f", "h", "j"]  # between-slot strings exist on both sides of every key


def term_source(i, n):
    keys = TERM_KEYS[:n]
    return dict(name=f"s{i}", type="terms", field=f"f{i}", interval=None, keys=keys, rank=None, sorted_keys=keys)


def hist_source(i):
    return dict(name=f"s{i}", type="histogram", field=f"f{i}", interval=0.5, keys=None, rank=None, sorted_keys=None)


def hist_layout(first_id, n_ids):
    zero = first_id <= 0 <= first_id + n_ids - 1
    return dict(slots=n_ids + (1 if zero else 0), first_id=first_id, zero_slot=-first_id if zero else -1)


def finish_layout(parts):
    """shift / bits / key_bits as the library lays them out: source 0 in the most significant bits"""
    bits = [max(0, (p["slots"] - 1).bit_length()) for p in parts]
    lays, below = [], sum(bits)
    for p, b in zip(parts, bits):
        below -= b
        lays.append(dict(p, bits=b, shift=below))
    return dict(sources=lays, key_bits=sum(bits), size=1, n_sources=len(parts), count_offset=0, children=[])


def slot_keys(src, lay):
    from searchlite_amd import aggs as A
    if src["type"] == "terms":
        return list(src["sorted_keys"])
    return [A.composite_slot_value(lay, src["interval"], s) for s in range(lay["slots"])]


def probes(src, keys):
    """every slot's key, a value between each pair of neighbours, one below all and one above all"""
    if src["type"] == "terms":
        return ["a"] + [v for k in keys for v in (k, chr(ord(k) + 1))]  # "a" < "b"; "c" between "b" and "d"; "k" above "j"
    out = [min(keys + [0.0]) - 1.0]
    for k in keys:
        out += [k, float(np.nextafter(np.float64(k), np.inf))] if k != 0.0 or math.copysign(1, k) > 0 else [k]
    return out + [max(keys) + 1.0, 0.0, -0.0]


LAYOUTS = []
for n_src in (2, 3):
    for sizes in itertools.product((1, 2, 5), repeat=n_src):
        # the last source alternates between terms and a histogram whose ids straddle zero (a -0.0 slot) or do not
        for variant in range(3):
            srcs, parts = [], []
            for i, n in enumerate(sizes):
                if i == n_src - 1 and variant > 0:
                    first = -(n // 2) if variant == 1 else 3
                    srcs.append(hist_source(i))
                    parts.append(hist_layout(first, n))
                else:
                    srcs.append(term_source(i, n))
                    parts.append(dict(slots=n, first_id=0, zero_slot=-1))
            LAYOUTS.append((srcs, finish_layout(parts)))


def test_lower_bound_exhaustive():
    from searchlite_amd import aggs as A
    checked = 0
    for srcs, layout in LAYOUTS:
        plan = A.AggPlan(None, [], composite=dict(sources=srcs))
        lays = layout["sources"]
        keys = [slot_keys(s, L) for s, L in zip(srcs, lays)]
        tuples = {}  # packed -> the tuple's order
        for slots in itertools.product(*[range(L["slots"]) for L in lays]):
            packed = sum(s << L["shift"] for s, L in zip(slots, lays))
            tuples[packed] = tuple(R.part_order(src, k[s]) for src, k, s in zip(srcs, keys, slots))
        assert len(set(tuples.values())) == len(tuples)  # (integer order is tuple order only if keys are distinct)
        assert sorted(tuples) == [p for p, _ in sorted(tuples.items(), key=lambda kv: kv[1])]
        for after_parts in itertools.product(*[probes(s, k) for s, k in zip(srcs, keys)]):
            after = {s["name"]: v for s, v in zip(srcs, after_parts)}
            bound = A.composite_lower_bound(layout, plan, after)
            want_after = tuple(R.part_order(s, v) for s, v in zip(srcs, after_parts))
            assert {p for p in tuples if p >= bound} == {p for p, o in tuples.items() if o > want_after}, (after, bound)
            if not any(o > want_after for o in tuples.values()):
                assert bound == 1 << layout["key_bits"], (after, bound)
            checked += 1
        # what the reference ignores starts from the beginning
        first = srcs[0]["name"]
        good = {s["name"]: k[0] for s, k in zip(srcs, keys)}
        for bad in (None, "x", {}, {n: v for n, v in good.items() if n != first}, dict(good, **{first: 7}),
                    dict(good, **{srcs[-1]["name"]: None}), dict(good, **{srcs[-1]["name"]: True})):
            assert A.composite_lower_bound(layout, plan, bad) == 0, bad
    assert checked > 10000
