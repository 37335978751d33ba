"""Nested filters on the device (slg_index_add_nested_path, slg_index_add_nested_field_*,
slg_index_add_nested_filter_trees) through the C ABI against tests/nested_ref.py.  The rule throughout is equality,
tolerance 0 (everything is comparisons and bit operations):

  * fetch_filter of every tree equals nested_ref & ~deleted, bit for bit, for every segment;
  * one search per tree family under the trees' ids returns rows bit-identical to the same search under the ids of
    add_filter(reference mask).

The world is tests/nested_world.py's (its edges are asserted on the CPU in tests/test_nested_ref.py): segments of
1, 33, 64, 65 and 257 docs with tombstones, docs of 0, 1, 2, 5 and 70 objects, the 70-object docs starting at bits
31, 32 and 63 of a wave, an empty path, NULL counts, short / unbound / out-of-range / NULL parents, value columns
shorter than the count, objects of 0, 1 and 3 values, NaN and infinities, int64 edges."""
import copy

import numpy as np
import pytest

from searchlite_amd import _native as N
from tests import nested_ref as R
from tests import nested_world as NW
from tests.test_gpu_bool import same
from tests.util import random_queries, random_segment

pytestmark = pytest.mark.gpu
VOCAB = 24
PATHS = ("c", "c.r", "c.r.z", "e")
NESTED_FIELDS = ("c.author", "c.score", "c.stars", "c.r.tag", "c.r.n", "c.r.z.v", "e.k")
DTYPES = {"i64": np.int64, "f64": np.float64}


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


def tombstoned(seg, dead):
    s = copy.copy(seg)
    s.deleted = np.packbits(dead, bitorder="little") if dead.any() else None
    s.docs = float(seg.n_docs - int(dead.sum()))
    return s


class World:
    """an index over nested_world's segments with every path and column registered; the reference masks are
    computed once per filter and shared"""

    def __init__(self, sa, sizes=NW.SIZES, seed=NW.SEED):
        self.ws, self.dead = NW.build(sizes, seed)
        rng = np.random.default_rng(seed)
        self.segs = [tombstoned(random_segment(rng, w["n_docs"], VOCAB, 5), d) for w, d in zip(self.ws, self.dead)]
        self.ix = sa.GpuIndex(self.segs)
        self.path_ids, self.field_ids = {}, {}
        self._wants = {}
        self.register()

    def register(self, paths=PATHS, fields=NESTED_FIELDS + ("cat", "n")):
        for p in paths:
            parent = NW.PATH_PARENT[p]
            self.path_ids[p] = self.ix.add_nested_path([NW.path_arrays(w, p) for w in self.ws],
                                                       -1 if parent is None else self.path_ids[parent])
        for name in fields:
            kind, keys = NW.KINDS[name], NW.KEYS.get(name)
            if "." in name:
                cols = [NW.column_arrays(w, name, keys) for w in self.ws]
                pid = self.path_ids[name.rsplit(".", 1)[0]]
                self.field_ids[name] = (self.ix.add_nested_keyword_field(pid, cols, len(keys)) if kind == "keyword"
                                        else self.ix.add_nested_field(pid, cols, DTYPES[kind]))
            elif kind == "keyword":
                docs = [[np.asarray([keys.index(v) for v in vals], np.uint32) for vals in w["doc"][name]] for w in self.ws]
                self.field_ids[name] = self.ix.add_agg_keyword_field(docs, len(keys))
            else:
                docs = [[np.asarray(vals, DTYPES[kind]) for vals in w["doc"][name]] for w in self.ws]
                self.field_ids[name] = self.ix.add_agg_field(docs, DTYPES[kind])

    def compile(self, flt):
        from searchlite_amd.filters import compile_nested_filter
        fields, nested = NW.describe(self.path_ids, self.field_ids)
        return compile_nested_filter(flt, fields, nested)

    def want(self, flt):
        key = repr(flt)
        if key not in self._wants:
            self._wants[key] = [np.array(R.mask(w, flt), bool) & ~d for w, d in zip(self.ws, self.dead)]
        return self._wants[key]

    def check(self, filters, what, search=True):
        """register the filters' trees in one call; every bitmap against nested_ref; then one search under the
        trees' ids against the same search under the ids of add_filter(reference mask); all removed again"""
        ids = self.ix.add_nested_filter_trees([self.compile(f) for f in filters])
        assert len(ids) == len(filters) and len(set(ids)) == len(ids)
        wants = [self.want(f) for f in filters]
        for t, (i, want) in enumerate(zip(ids, wants)):
            got = self.ix.fetch_filter(i)
            for s in range(len(self.segs)):
                assert got[s].dtype == bool and got[s].shape == want[s].shape
                if not np.array_equal(got[s], want[s]):
                    d = int(np.argwhere(got[s] != want[s])[0, 0])
                    raise AssertionError(f"{what}: tree {t} segment {s} doc {d}: got {got[s][d]}, want {want[s][d]} "
                                         f"({filters[t]})")
        if search:
            part = list(range(min(len(filters), 16)))
            twins = [self.ix.add_filter(wants[j]) for j in part]
            qs = random_queries(np.random.default_rng(len(filters)), len(part), 2, VOCAB, len(self.segs))
            got = self.ix.search_batch(*qs, 600, q_filter=np.array([ids[j] for j in part], np.int32))
            ref = self.ix.search_batch(*qs, 600, q_filter=np.array(twins, np.int32))
            same(got, ref, f"{what}: search under the trees")
            for tw in twins:
                self.ix.remove_filter(tw)
        for i in ids:
            self.ix.remove_filter(i)


@pytest.fixture(scope="module")
def world(gpu):
    W = World(gpu)
    yield W
    W.ix.close()


@pytest.mark.parametrize("family", sorted(NW.FAMILIES))
def test_family_bitmaps_equal_the_reference_and_one_search_its_twin(world, family):
    world.check(NW.FAMILIES[family], family)


def test_every_family_in_one_call_shares_the_levels(world):
    """trees of depth 0 to 3 in one call: a level's scopes of all trees ride one launch"""
    world.check([f for fam in sorted(NW.FAMILIES) for f in NW.FAMILIES[fam]] + [NW.keq("cat", "news")], "all families",
                search=False)


def test_limits_16_scopes_depth_4_and_64_trees(gpu, world):
    W = world
    # a fourth level under c.r.z: one object per doc, bound to z object 0 (it has no column: its scope is NOT of OR of
    # nothing, so a z object passes iff it is object 0 of its doc)
    q = W.ix.add_nested_path([(np.ones(w["n_docs"], np.uint32), (np.arange(w["n_docs"] + 1, dtype=np.uint32),
                                                                np.zeros(w["n_docs"], np.uint32))) for w in W.ws],
                             W.path_ids["c.r.z"])
    W.path_ids["c.r.z.q"] = q
    for w in W.ws:
        w["counts"]["c.r.z.q"] = [1] * w["n_docs"]
        w["parents"]["c.r.z.q"] = [[0]] * w["n_docs"]
    try:
        deep = NW.nest("c", NW.nest("r", NW.nest("z", NW.nest("q", NW.NOT(NW.OR())))))
        W.check([deep, NW.NOT(deep)], "depth 4", search=False)
        # a hand-made fifth level (q under q): refused for its depth before the index is asked whether q lies under q
        c, r, z = (W.path_ids[p] for p in ("c", "c.r", "c.r.z"))
        five = ([(q, 0, 1), (q, 1, 1), (z, 2, 1), (r, 3, 1), (c, 4, 1), (-1, 5, 1)],
                [dict(kind=4, arity=0)] + [dict(kind=7, field=i) for i in range(5)], [])
        with pytest.raises(gpu.SlgError) as ei:
            W.ix.add_nested_filter_trees([five])
        assert ei.value.code == N.ERR_UNSUPPORTED and "SLG_MAX_NESTED_DEPTH" in str(ei.value)
    finally:
        for w in W.ws:
            del w["counts"]["c.r.z.q"], w["parents"]["c.r.z.q"]
        W.ix.remove_nested_path(q)
        del W.path_ids["c.r.z.q"]
    # 15 object scopes and the doc level: exactly SLG_MAX_NESTED_SCOPES; one more is refused
    lone = [NW.nest("c", NW.keq("author", f"a{i % 8}")) for i in range(16)]
    W.check([NW.OR(*lone[:15])], "16 scopes", search=False)
    with pytest.raises(gpu.SlgError) as ei:
        W.ix.add_nested_filter_trees([W.compile(NW.OR(*lone))])
    assert ei.value.code == N.ERR_UNSUPPORTED and "SLG_MAX_NESTED_SCOPES" in str(ei.value)
    # 64 trees in one call; 65 are refused
    many = [NW.nest("c", NW.AND(NW.keq("author", f"a{i % 8}"), NW.i64("stars", -3 - i, 7 + i))) for i in range(64)]
    W.check(many, "64 trees")
    with pytest.raises(gpu.SlgError) as ei:
        W.ix.add_nested_filter_trees([W.compile(f) for f in many + many[:1]])
    assert ei.value.code == N.ERR_UNSUPPORTED and "SLG_MAX_FILTER_TREES" in str(ei.value)


def test_all_or_nothing_and_the_checks_against_the_state(gpu, world):
    W = world
    base = W.ix.add_filter([None] * len(W.segs))
    gen = W.ix.generation
    good = [W.compile(f) for f in NW.FAMILIES["two levels"]]
    bad = ([(W.path_ids["c"], 0, 1), (-1, 1, 1)], [dict(kind=1, field=999, lo_f=0.0, hi_f=1.0), dict(kind=7, field=0)], [])
    with pytest.raises(gpu.SlgError) as ei:
        W.ix.add_nested_filter_trees(good + [bad])
    assert ei.value.code == N.ERR_INVALID and "unknown nested field id 999" in str(ei.value)
    assert W.ix.generation == gen
    with pytest.raises(gpu.SlgError):
        W.ix.fetch_filter(base + 1)
    assert W.ix.add_filter([None] * len(W.segs)) == base + 1   # no slot was taken
    W.ix.remove_filter(base + 1)
    W.ix.remove_filter(base)
    c, r, z = (W.path_ids[p] for p in ("c", "c.r", "c.r.z"))
    leaf = lambda kind, name, **kw_: dict(kind=kind, field=W.field_ids[name], **kw_)
    one = lambda path, node, ords=(): ([(path, 0, 1), (-1, 1, 1)], [node, dict(kind=7, field=0)], list(ords))
    for tree, word in ((one(77, dict(kind=5, arity=0)), "unknown nested path id 77"),
                       (one(c, leaf(0, "c.score")), "not a keyword field"),
                       (one(c, leaf(1, "c.stars", lo_f=0.0, hi_f=1.0)), "not an f64 field"),
                       (one(c, leaf(2, "c.score")), "not an i64 field"),
                       (one(c, leaf(0, "c.author", ord_begin=0, n_ords_in=1), [33]), "ordinal 33 >= n_ords"),
                       (one(c, dict(kind=3, filter_id=0)), "FILTER_ID in an object scope"),
                       # z lies under c.r, not under c
                       (([(z, 0, 1), (c, 1, 1), (-1, 2, 1)],
                         [dict(kind=5, arity=0), dict(kind=7, field=0), dict(kind=7, field=1)], []), "is not registered under path")):
        with pytest.raises(gpu.SlgError) as ei:
            W.ix.add_nested_filter_trees([tree])
        assert ei.value.code == N.ERR_INVALID and word in str(ei.value), (tree, str(ei.value))
    # a column of another path inside a scope: the reference looks up `c.tag`, which does not exist: nothing passes
    other = one(c, leaf(0, "c.r.tag", ord_begin=0, n_ords_in=1), [0])
    (fid,) = W.ix.add_nested_filter_trees([other])
    assert not any(m.any() for m in W.ix.fetch_filter(fid))
    W.ix.remove_filter(fid)
    # more than 2^32 - 1 objects in a segment are refused on the host, before anything is allocated
    huge = [None] * len(W.segs)
    huge[1] = np.full(W.ws[1]["n_docs"], 2**27, np.uint32)     # 33 docs x 2^27 objects = 2^32 + 2^27
    with pytest.raises(gpu.SlgError) as ei:
        W.ix.add_nested_path(huge)
    assert ei.value.code == N.ERR_UNSUPPORTED and "2^32 - 1" in str(ei.value)
    assert W.ix.generation == gen


def test_lifecycle(gpu):
    """update_deleted keeps the tables; a prepared batch survives remove_filter; add_segment leaves paths and fields
    without data for the new segment until they are registered again; remove_segment drops that segment's"""
    W = World(gpu, sizes=(65, 33), seed=7)
    try:
        flt = NW.nest("c", NW.AND(NW.keq("author", "a0"), NW.nest("r", NW.i64("n", -1, 2))))
        qs = random_queries(np.random.default_rng(5), 3, 2, VOCAB, 2)
        (before,) = W.ix.add_nested_filter_trees([W.compile(flt)])
        dead = W.dead[0].copy()
        dead[[0, 31, 32, 63]] = True
        W.ix.update_deleted(0, np.packbits(dead, bitorder="little"), float(65 - dead.sum()))
        W.dead[0] = dead
        W._wants.clear()
        (after,) = W.ix.add_nested_filter_trees([W.compile(flt)])
        want = W.want(flt)
        got = W.ix.fetch_filter(after)
        assert all(np.array_equal(got[s], want[s]) for s in range(2))
        # a batch prepared before slg_index_remove_filter still runs
        ref = W.ix.search_batch(*qs, 100, q_filter=np.full(3, after, np.int32))
        b = W.ix.prepare(*qs, 100, q_filter=np.full(3, after, np.int32))
        W.ix.remove_filter(after)
        b.run()
        same(b.fetch(), ref, "prepared before the removal")
        b.close()
        W.ix.remove_filter(before)
        # a new segment: paths and fields have nothing for it
        w2, d2 = NW._segment(np.random.default_rng(3), 64, 0)
        new = tombstoned(random_segment(np.random.default_rng(10), 64, VOCAB, 5), d2)
        assert W.ix.add_segment(new) == 2
        W.segs.append(new)
        W.ws.append(w2)
        W.dead.append(d2)
        with pytest.raises(gpu.SlgError) as ei:
            W.ix.add_nested_filter_trees([W.compile(flt)])
        assert ei.value.code == N.ERR_INVALID and "no tables for segment 2" in str(ei.value)
        old_paths, old_fields = dict(W.path_ids), dict(W.field_ids)
        W.register(paths=("c", "c.r"), fields=())
        with pytest.raises(gpu.SlgError) as ei:   # the new paths, the old fields
            W.ix.add_nested_filter_trees([W.compile(flt)])
        assert ei.value.code == N.ERR_INVALID and "no column for segment 2" in str(ei.value)
        W.register(paths=(), fields=("c.author", "c.r.n"))
        assert W.path_ids["c"] != old_paths["c"] and W.field_ids["c.author"] != old_fields["c.author"]   # ids are not reused
        W._wants.clear()
        W.check([flt, NW.NOT(flt)], "registered again")
        # the old registrations go; removing a path takes the fields under it along
        W.ix.remove_nested_field(old_fields["c.stars"])
        W.ix.remove_nested_path(old_paths["c"])
        with pytest.raises(gpu.SlgError):
            W.ix.remove_nested_field(old_fields["c.score"])
        with pytest.raises(gpu.SlgError):
            W.ix.remove_nested_path(old_paths["c"])
        # slg_index_remove_segment: the bitmaps and the tables of the segments left stay
        (again,) = W.ix.add_nested_filter_trees([W.compile(flt)])
        want = W.want(flt)
        W.ix.remove_segment(0)
        got = W.ix.fetch_filter(again)
        assert len(got) == 2 and np.array_equal(got[0], want[1]) and np.array_equal(got[1], want[2])
        del W.segs[0], W.ws[0], W.dead[0]
        W._wants.clear()
        W.check([flt], "after the segment left")
    finally:
        W.ix.close()
