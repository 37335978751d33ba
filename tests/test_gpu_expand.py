"""Term expansion on the device (slg_index_set_terms / slg_expand_batch): fuzzy, prefix and wildcard.

Expected: tests/expand_ref.py, the reference's expansion restated line for line and pinned to the reference's own
tests in tests/test_expand_ref.py.  Bar: exact equality of keys, order, distances and term-id rows; nothing here
is floating point but the end-to-end scores, and those are compared as f32 bit patterns.  The dictionaries
(tests/expand_worlds.py) are synthetic and tiny; every world's requests go to the device in ONE call.
"""
import ctypes as C

import numpy as np
import pytest

from tests import expand_ref as R
from tests import expand_util as U
from tests import expand_worlds as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


def open_world(gpu, seg_keys):
    ix = gpu.GpuIndex([W.dict_segment(k) for k in seg_keys])
    ix.set_terms_from_segments()
    return ix


def check_world(gpu, seg_keys, reqs):
    """one expand() call over reqs; every request's rows against tests/expand_ref.py"""
    world = U.World(seg_keys)
    with open_world(gpu, seg_keys) as ix:
        got = ix.expand(reqs)
        again = ix.expand(reqs)
    assert len(got) == len(reqs)
    for r, (ids, dist), (ids2, dist2) in zip(reqs, got, again):
        want_ids, want_dist = world.want(r)
        what = {k: (v if len(str(v)) < 40 else str(v)[:40] + "...") for k, v in r.items()}
        assert ids.shape == want_ids.shape, what
        assert ids.tolist() == want_ids.tolist(), what
        assert dist.tolist() == want_dist.tolist(), what
        assert ids.tolist() == ids2.tolist() and dist.tolist() == dist2.tolist(), what   # the same from run to run
    return got


def test_geometry_constants_are_the_headers():
    import os
    import re
    from searchlite_amd import _native as N
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "searchlite_gpu.h")).read()
    for name, val in (("WAVE", N.EXPAND_WAVE), ("WORKGROUP", N.EXPAND_WORKGROUP), ("CHUNK", N.EXPAND_CHUNK)):
        assert int(re.search(r"#define SLG_EXPAND_%s (\d+)u" % name, text).group(1)) == val
    assert W.CHUNK % W.GROUP == 0 and W.GROUP % W.WAVE == 0


def test_range_wave_and_chunk_edges(gpu):
    """ranges of 1, wave - 1 .. 2 x chunk + 1 keys; passing keys only first, only last, on both sides of every wave,
    workgroup and chunk boundary, exactly max_expansions of them and one more, max_expansions 0 / 1 / the limit;
    bare keys; sibling fields; empty ranges; the range that ends the dictionary"""
    got = check_world(gpu, W.range_world(), W.range_requests())
    assert sum(len(d) for _, d in got) > 5000    # (the world does produce keys)


def test_the_whole_dictionary_as_one_range(gpu):
    check_world(gpu, W.whole_world(), W.whole_requests())


def test_passing_keys_spread_over_many_chunks(gpu):
    """the first R of a range whose fuzzy matches lie all over it; every max_edits, prefix_length and cap"""
    check_world(gpu, W.dense_world(), W.dense_requests())


def test_distances_utf8_and_wildcards(gpu):
    """one and two edits of each kind, a transposition is two, max_edits 0 and 3, length differences of max_edits
    and one more, candidate == term, terms of 0 .. 3 and 128 chars, 2- / 3- / 4-byte chars in terms, candidates
    and fuzzy prefixes, keys whose byte and char lengths fall on different sides of the filter, saturated char
    counts; '*', leading and trailing '*', the back-up, '?' on a multi-byte char, no wildcard, U+000A"""
    seg_keys, reqs = W.words_world(), W.words_requests()
    got = check_world(gpu, seg_keys, reqs)
    ids = {k: i for i, k in enumerate(seg_keys[0])}

    def keys_of(req):
        rows, dist = got[reqs.index(req)]
        inv = {v: k for k, v in ids.items()}
        return [(inv.get(int(r[0])), int(d)) for r, d in zip(rows, dist)]
    # spot checks by hand, on top of the reference's restatement
    two = dict(keys_of(U.fuzzy("body", "rust", 2, 1, 50, 0)))
    assert two["body:rsut"] == 2 and two["body:rusk"] == 1 and two["body:rut"] == 1 and "body:rustabc" not in two
    assert "body:rustab" in two and "body:trust" not in two and two["body:rust"] == 0
    assert dict(keys_of(U.fuzzy("body", "rust", 2, 0, 50, 0)))["body:trust"] == 1
    assert dict(keys_of(U.fuzzy("body", "cafe", 1, 1, 50, 0)))["body:café"] == 1
    assert dict(keys_of(U.fuzzy("body", "東京", 1, 1, 50, 0))) == {"body:東京": 0, "body:東亰": 1, "body:東京都": 1}
    assert [k for k, _ in keys_of(U.wildcard("kw", "a*b*c", 50))] == ["kw:aXbXbc", "kw:abbc", "kw:abc", "kw:abcabc"]
    assert [k for k, _ in keys_of(U.wildcard("kw", "a?c", 50))] == ["kw:a*c", "kw:abc", "kw:aéc"]
    assert [k for k, _ in keys_of(U.wildcard("kw", "?", 50))] == ["kw:b", "kw:é"]


def test_three_segments(gpu):
    """overlapping and disjoint vocabularies, term ids against the byte order, NO_TERM holes, the global fuzzy cap
    reached inside a segment, the per-segment cap behind the duplicates of two earlier segments"""
    seg_keys, reqs = W.segments_world(), W.segments_requests()
    got = check_world(gpu, seg_keys, reqs)
    rows, _ = got[reqs.index(U.prefix("body", "r", 10))]
    assert len(rows) == 30 and (rows == R.NO_TERM).sum() == 0      # r000 .. r029, ten per segment, held by all
    assert rows[10].tolist() == [10, 89, 10]                       # (segment 1's ids run against the byte order)
    rows, _ = got[reqs.index(U.fuzzy("title", "rusx", 1, 1, 50, 3))]
    assert rows.tolist() == [[R.NO_TERM] * 3, [R.NO_TERM, R.NO_TERM, 102]]


def test_randomised_mixed_batch(gpu):
    seg_keys, vocab = W.random_world()
    assert 2000 <= sum(len(k) for k in seg_keys) <= 3000
    reqs = W.random_requests(vocab)
    got = check_world(gpu, seg_keys, reqs)
    # the C++ restatement of the reference's loop (what tools/expand_time.py times the scan against) agrees too
    ref = U.reference_loop(reqs, [U.HostDict(k) for k in seg_keys], 2)
    for (a, b), (c, d) in zip(got, ref):
        assert a.tolist() == c.tolist() and b.tolist() == d.tolist()


def test_index_states(gpu):
    from searchlite_amd import _native as N
    from tests.util import random_queries, random_segment
    rng = np.random.default_rng(5)
    seg0, seg1 = random_segment(rng, 300, 40, 12), random_segment(rng, 200, 40, 12)
    keys0 = [f"body:{W.word(i)}" for i in range(40)]
    keys1 = [f"body:{W.word(2 * i)}" for i in range(40)]
    offs, terms, w = random_queries(rng, 8, 3, 40, n_segs=2)
    req = U.prefix("body", "aaa", 50)
    with gpu.GpuIndex([seg0, seg1]) as ix:
        b = ix.prepare(offs, terms, w, 5)
        b.run()
        before = b.fetch()
        ix.set_terms(0, keys0)
        with pytest.raises(N.SlgError) as ei:                      # segment 1 has no dictionary yet
            ix.expand([req])
        assert ei.value.code == N.ERR_INVALID and "segment 1" in ei.value.msg
        ix.set_terms(1, keys1)
        b.run()                                                    # a batch prepared before keeps its state
        after = b.fetch()
        for x, y in zip(before, after):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        b.close()
        world = U.World([keys0, keys1])
        ids, dist = ix.expand([req])[0]
        assert ids.tolist() == world.want(req)[0].tolist() and len(dist) == 26
        ix.update_deleted(0, np.packbits(np.arange(300) < 7, bitorder="little"), 293.0)   # keeps the dictionaries
        assert ix.expand([req])[0][0].tolist() == ids.tolist()
        # a segment added later has none until it is set
        keys2 = ["body:aaaa", "body:zzzz", "title:aaab"]
        ix.add_segment(W.dict_segment(keys2))
        with pytest.raises(N.SlgError) as ei:
            ix.expand([req])
        assert ei.value.code == N.ERR_INVALID and "segment 2" in ei.value.msg
        ix.set_terms(2, keys2)
        world = U.World([keys0, keys1, keys2])
        assert ix.expand([req])[0][0].tolist() == world.want(req)[0].tolist()
        ix.remove_segment(0)                                       # its dictionary goes with it
        world = U.World([keys1, keys2])
        got = ix.expand([req, U.fuzzy("body", "zzzy", 1, 1, 50, 3)])
        assert got[0][0].tolist() == world.want(req)[0].tolist()
        assert got[1][0].tolist() == [[R.NO_TERM, R.NO_TERM], [R.NO_TERM, 1]] and got[1][1].tolist() == [0, 1]


def test_an_index_built_from_a_directory_has_its_dictionaries(gpu, tmp_path):
    """GpuIndex.from_directory: searchlite's files (restated writer, oracle/segfile_writer.py) -> segments staged
    with their term dictionaries, so expand() works with no set_terms call"""
    from oracle import segfile_writer
    segs = build_corpus(gpu)
    segfile_writer.write_index(str(tmp_path), segs, keep_positions=True)
    world = U.World([R.sorted_keys(s.term_dict) for s in segs])     # (the files' term ids are the byte order)
    reqs = [U.fuzzy("body", "rusk", 2, 1, 50, 3), U.prefix("body", "ru", 50), U.wildcard("body", "?us*", 50),
            U.fuzzy("body", "cafe", 1, 1, 50, 3)]
    from searchlite_amd.searcher import GpuIndex
    with GpuIndex.from_directory(str(tmp_path)) as ix:
        assert ix.n_segs == 2
        for r, (ids, dist) in zip(reqs, ix.expand(reqs)):
            want_ids, want_dist = world.want(r)
            assert len(dist) > 1 and ids.tolist() == want_ids.tolist() and dist.tolist() == want_dist.tolist(), r


# ---- end to end ---------------------------------------------------------------------------------------------
CORPUS = [
    [("d1", "Rust is fast and rusty systems trust it"), ("d2", "the dusk of a bust"), ("d3", "rush to the café"),
     ("d4", "systems programming in rust"), ("d5", "naïve cafe owners rest")],
    [("e1", "rusk and ruse"), ("e2", "system of a dusk"), ("e3", "fast fest fist"), ("e4", "cafés and caffe")],
]


def build_corpus(gpu):
    segs = []
    for docs in CORPUS:
        b = gpu.SegmentBuilder(["body"])
        for eid, text in docs:
            b.add_document(eid, {"body": text})
        segs.append(b.build())
    return segs


def reference_queries(segs, queries, fuzzy):
    """the arrays of search_plan from tests/expand_ref.py alone: one leaf per source term, keys folded by their
    bytes with their first leaf (api/reader.rs:2971-2983), weights boost * distance_weight in f32"""
    from searchlite_amd.segment import default_tokenize
    seg_sorted = [R.sorted_keys(s.term_dict) for s in segs]
    offs, rows, weights, leaves, nleaves = [0], [], [], [], []
    for q in queries:
        acc, order = {}, []
        for leaf, tok in enumerate(default_tokenize(q)):
            for key, dist in R.expand_term_fuzzy(seg_sorted, "body", tok, **fuzzy):
                if key not in acc:
                    acc[key] = [np.float32(0.0), leaf]
                    order.append(key)
                acc[key][0] = np.float32(acc[key][0] + np.float32(1.0) * R.distance_weight(dist))
        used = sorted({acc[k][1] for k in order})
        for k in order:
            rows.append([s.term_id(k) for s in segs])
            weights.append(acc[k][0])
            leaves.append(used.index(acc[k][1]))
        nleaves.append(len(used))
        offs.append(len(rows))
    nq = len(queries)
    return (np.array(offs, np.uint32), np.array(rows, np.uint32).reshape(-1, len(segs)), np.array(weights, np.float32),
            dict(q_leaf=np.array(leaves, np.uint32), q_plan=np.zeros(nq, np.uint32), q_tie=np.zeros(nq, np.float32),
                 q_nleaves=np.array(nleaves, np.uint32)))


def test_search_fuzzy_is_the_plain_batch_of_the_references_queries(gpu):
    segs = build_corpus(gpu)
    queries = ["rusk systms", "rust", "cafe fst", "dusk dusk rust", "zzzz", "naive programing", "ru of"]
    for fuzzy in (dict(max_edits=1, prefix_length=1, max_expansions=50, min_length=3),
                  dict(max_edits=2, prefix_length=0, max_expansions=4, min_length=3)):
        offs, terms, w, plans = reference_queries(segs, queries, fuzzy)
        with gpu.GpuIndex(segs) as ix:
            ix.set_terms_from_segments()
            g_offs, g_terms, g_w, g_plans = ix.expanded_queries(queries, "body", fuzzy)
            assert g_offs.tolist() == offs.tolist() and g_terms.tolist() == terms.tolist()
            assert g_w.view(np.uint32).tolist() == w.view(np.uint32).tolist()
            assert all(np.array_equal(g_plans[k], plans[k]) for k in plans)
            got = ix.search_fuzzy(queries, "body", 6, fuzzy)
            want = ix.search_plan(offs, terms, w, 6, **plans)
        for a, b in zip(got, want):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert got[3][0] > 0 and got[3][4] == 0     # ("rusk systms" finds docs through its expansions; "zzzz" none)


SMOKE = [   # tests/smoke.rs:159-325: docs, query, FuzzyOptions (max_edits, prefix_length, max_expansions, min_length), hits
    (["Rust is fast"], "rusk", (1, 1, 20, 3), 1), (["Rust", "Systems"], "rusk systms", (1, 1, 20, 3), 2),
    (["Rust"], "ru", (1, 1, 20, 3), 0),
    (["Rush", "Rust"], "rusk", (1, 1, 1, 3), 1), (["Rush", "Rust"], "rusk", (1, 1, 2, 3), 2),
    (["Dusk"], "rusk", (1, 0, 20, 3), 1), (["Dusk"], "rusk", (1, 1, 20, 3), 0),
    (["Rust"], "rsut", (1, 1, 20, 3), 0), (["Rust"], "rsut", (2, 1, 20, 3), 1),
]


@pytest.mark.parametrize("case", range(len(SMOKE)))
def test_smoke_rs_scenarios_give_the_references_hit_counts(gpu, case):
    docs, query, (me, pl, mx, ml), hits = SMOKE[case]
    b = gpu.SegmentBuilder(["body"])
    for i, text in enumerate(docs):
        b.add_document(f"doc-{i + 1}", {"body": text})
    with gpu.GpuIndex([b.build()]) as ix:
        ix.set_terms_from_segments()
        _, _, _, count = ix.search_fuzzy([query], "body", 11, dict(max_edits=me, prefix_length=pl, max_expansions=mx,
                                                                   min_length=ml))
        assert int(count[0]) == hits
        assert ix.search(query, "body") == []       # without the fuzzy option none of these queries matches


def test_a_query_that_folds_to_more_than_32_terms_is_unsupported(gpu):
    from searchlite_amd import _native as N
    b = gpu.SegmentBuilder(["body"])
    b.add_document("d", {"body": " ".join("aaa" + chr(ord("a") + i) for i in range(26)) + " " +
                                 " ".join("aa" + chr(ord("b") + i) + "a" for i in range(10))})
    with gpu.GpuIndex([b.build()]) as ix:
        ix.set_terms_from_segments()
        ix.search_fuzzy(["aaaa"], "body", 3, dict(max_edits=1, prefix_length=1, max_expansions=31, min_length=3))
        with pytest.raises(N.SlgError) as ei:
            ix.search_fuzzy(["ok", "aaaa"], "body", 3, dict(max_edits=1, prefix_length=1, max_expansions=50, min_length=3))
        assert ei.value.code == N.ERR_UNSUPPORTED and "query 1" in ei.value.msg and "aaaa" in ei.value.msg
