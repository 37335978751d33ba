"""The lifecycle world (tests/lifecycle_world.py) proves, with the references alone, that the device cases of
tests/test_gpu_lifecycle.py cannot pass vacuously:

  * every step of every scenario changes what every kind is expected to return (five kinds are by contract the same
    across a delete: a dictionary holds no tombstone (expand, regex, suggest), a rerank scores the candidates it is
    handed, and host hits are highlighted whatever their tombstones; that sameness is what is asserted for them, here
    and on the device);
  * the kinds added since the suite was written have something to show in every segment a step touches
    (test_the_kinds_added_since_..., test_term_buckets_background_follows_every_step);
  * after a removal, the expectation differs from what the same reference gives when ONE resource list is left
    unshifted (lifecycle_world.unshifted), for every resource a kind reads: a library that forgot to erase that list's
    entry in reshape_per_segment would fail the device check of that kind.

This is the would-it-notice argument, made on the CPU on purpose: no broken library is built or run anywhere."""
import numpy as np
import pytest

from tests import lifecycle_world as W


@pytest.fixture(scope="module")
def states(oracle):
    """per scenario [(label, op, model before, model after)]; the models keep their memoised expectations"""
    out = {}
    for name in W.SCENARIOS:
        m, steps = W.scenario(name)
        rows = []
        for label, op in steps:
            before = m.clone()
            before._memo = m._memo   # (the state is the same: share what was computed for it)
            m = m.clone()
            W.apply(m, op)
            rows.append((label, op, before, m))
        out[name] = rows
    return out


def test_the_world_is_what_the_issue_asks_for():
    m, fifth = W.build()
    assert tuple(m.n_docs()) == (65, 300, 33, 200) and fifth["segs"].n_docs == 64
    assert m.segs[0].deleted is None and m.segs[2].deleted is None          # `deleted` null
    assert m.dead(1).any() and m.dead(3).any() and m.dead(3)[-1]             # tombstones present, the last doc too
    assert all(s.n_terms == W.VOCAB and len(k) == W.VOCAB for s, k in zip(m.segs, m.keys))
    assert all(s.pos_offsets is not None and int(s.pos_offsets[-1]) == len(s.positions) for s in m.segs)
    byte_order = lambda keys: keys == sorted(keys, key=lambda k: k.encode("utf-8"))
    assert [byte_order(k) for k in m.keys] == [True, False, True, True]      # term ids against the byte order in one
    assert all(s.vec_dim == W.DIM for s in m.segs) and [x is None for x in m.xvec] == [False, True, False, False]
    assert all(len(v) <= 1 for seg in m.kw for v in seg)                     # collapse takes one value per doc
    offs = m.q["offs"]
    assert len(offs) - 1 == W.NQ <= 8 and len(W.scan_queries(W.CANON)[0]) <= 8 and int(offs[-1] - offs[-2]) == 12     # the many-term query: 12 lists
    assert {W.K, W.K_PLAIN} == {11, 65}
    # every filter passes some docs and rejects some in every segment: a bitmap of another segment shows
    for name, masks in m.filter_masks().items():
        assert all(0 < int(mk.sum()) < len(mk) for mk in masks), name
    ends = lambda segs: (min(v for s in segs for d in m.num[s] for v in d), max(v for s in segs for d in m.num[s] for v in d))
    assert len({ends([0, 1, 2, 3]), ends([1, 2, 3]), ends([0, 1, 2])}) == 3   # removing the first or the last moves an end
    merged = W.merge_entries(m.entry(0), m.entry(2))
    assert merged["segs"].n_docs == 98 and merged["segs"].deleted is None
    assert merged["tok"] == m.tok[0] + m.tok[2] and merged["keys"] == m.keys[0]
    assert merged["segs"].n_terms == len(merged["keys"]) == W.VOCAB
    assert set(W.KINDS[:len(W.OLD_KINDS)]) == set(W.OLD_KINDS) and len(W.OLD_KINDS) == 16


def test_the_lists_added_since_are_what_the_issue_asks_for():
    m, fifth = W.build()
    entries = [m.entry(s) for s in range(4)] + [fifth, W.merge_entries(m.entry(0), m.entry(2))]
    assert [e["text"] is None for e in entries] == [False, False, False, True, False, False]   # one segment: NULL offsets
    for e in entries:
        n = e["segs"].n_docs
        if e["text"] is not None:
            assert len(e["text"]) == n and all(t.isascii() for t in e["text"]) and 0 < sum(t == b"" for t in e["text"]) < n // 4
            for d, t in enumerate(e["text"]):      # built from the segment's own token sequences
                assert t == b"" or [w.lower() for w in t.replace(b",", b"").replace(b".", b"").replace(b" -", b"").decode().split()] \
                    == [W.tword(x) for x in e["tok"][d]]
        counts, parents = e["npath"]["counts"], e["npath"]["parents"]
        assert set(counts) == {"c", "c.r"} and set(parents) == {"c.r"}
        for p in counts:
            assert len(counts[p]) == n and set(counts[p]) == {0, 1, 2, 5}
        assert all(len(parents["c.r"][d]) == counts["c.r"][d] for d in range(n))
        assert all(x is None or x < counts["c"][d] for d in range(n) for x in parents["c.r"][d])
        assert any(x is None for row in parents["c.r"] for x in row)
        assert n < 64 or W.crosses_a_word(counts["c"])                       # an object range over a 32-bit word
        assert all(len(e["ncol"][name]) == n for name in ("c.author", "c.r.n"))
        assert all(len(e["ncol"]["c.author"][d]) <= counts["c"][d] and len(e["ncol"]["c.r.n"][d]) <= counts["c.r"][d]
                   for d in range(n))
        ts = e["ts"]
        flat = [v for d in ts for v in d]
        assert len(ts) == n and 0 < sum(not d for d in ts) < n // 4 and 0 < sum(len(d) == 2 for d in ts) < n // 3
        assert {-1, 0} <= set(flat) and min(flat) < -31 * W.DAY and max(flat) > 31 * W.DAY   # the epoch, a month on each side
    merged = entries[-1]
    assert merged["text"] == m.text[0] + m.text[2] and merged["ts"] == m.ts[0] + m.ts[2]
    assert merged["npath"]["counts"]["c"] == m.npath[0]["counts"]["c"] + m.npath[2]["counts"]["c"]
    assert merged["ncol"]["c.r.n"] == m.ncol[0]["c.r.n"] + m.ncol[2]["c.r.n"]
    # the registered arrays are what tests/nested_world.py makes of them, for every segment
    arrays = W.nested_arrays(m)
    for s in range(4):
        assert isinstance(arrays["c"][s], np.ndarray) and isinstance(arrays["cr"][s], tuple)
        assert len(arrays["author"][s][0]) == m.n_docs()[s] + 1 and arrays["n"][s][2].dtype == np.int64


def test_tombstone_sets(oracle):
    m, _ = W.build()
    prev = {}
    shifted = m.clone()
    shifted.remove(0)
    for n, (seg, docs) in zip((65, 65, 33, 33), W.tombstone_sets(m, oracle) + [W.shifted_tombstones(shifted, oracle)]):
        edges = {d for d in W.EDGE_DOCS if d < n} | {n - 1}
        assert edges <= set(docs) and max(docs) < n, (seg, sorted(edges - set(docs)))
    for seg, docs in W.tombstone_sets(m, oracle):
        assert set(prev.get(seg, ())) <= set(docs)                            # the reference never resurrects a doc
        prev[seg] = docs
        doc, sg, _, count = W.expect(m, "plain", oracle)
        top_k = {(int(sg[q, i]), int(doc[q, i])) for q in range(len(count)) for i in range(int(count[q]))}
        assert any((seg, d) in top_k for d in docs), f"tombstones of segment {seg} remove no current hit"
        for kind in W.OLD_KINDS:   # and a current hit of every kind that a delete shows in (the kinds added since:
            if kind not in W.SAME_UNDER_DELETE:   # test_the_kinds_added_since_have_something_in_every_touched_segment)
                assert any(s == seg and d in set(docs) for s, d in W.hit_docs(m, kind, oracle)), (seg, kind)
        m.delete(seg, docs)
    assert m.segs[2].docs == 0.0 and m.dead(2).all()                          # live_docs 0.0


@pytest.mark.parametrize("name", W.SCENARIOS)
def test_every_step_changes_every_kind(states, oracle, name):
    for label, op, before, after in states[name]:
        for kind in W.KINDS:
            same_by_contract = op[0] == "delete" and kind in W.SAME_UNDER_DELETE
            assert W.differs(before, after, kind, oracle) != same_by_contract, f"{name} / {label} / {kind}"


@pytest.mark.parametrize("name", [n for n in W.SCENARIOS if n != "delete" and n != "add"])
def test_an_unshifted_resource_shows_in_every_kind_that_reads_it(states, oracle, name):
    seen = 0
    for label, op, before, after in states[name]:
        if op[0] != "remove":
            continue
        for kind in W.KINDS:
            for resource in W.READS[kind]:
                wrong = W.unshifted(before, op[1], resource)
                assert wrong.n_docs() == after.n_docs()
                assert W.differs(after, wrong, kind, oracle), f"{name} / {label}: {kind} is blind to an unshifted {resource}"
                seen += 1
    assert seen >= sum(len(r) for r in W.READS.values())


def live_in(m, s, pairs):
    return [d for sg, d in pairs if sg == s and not m.dead(s)[d]]


def touched(op, after):
    """the segments a step leaves changed or new (a removal touches no segment that is left)"""
    return [] if op[0] == "remove" else [op[1]] if op[0] == "delete" else [after.n_segs - 1]


@pytest.mark.parametrize("name", W.SCENARIOS)
def test_the_kinds_added_since_have_something_in_every_touched_segment(states, oracle, name):
    """at every checkpoint, in every segment the step touched (with a live doc left): an aggregated doc with a
    timestamp, docs that pass and docs that fail the nested tree and a bool hit under it, a row of the plain batch
    with fragments, a host hit with fragments (or, in the segment without text, hits at all); and in EVERY segment
    of every state a key that the regex requests and the suggester's requests return"""
    from searchlite_amd import _native as N
    for label, op, before, after in states[name]:
        m, at = after, f"{name} / {label}"
        for s in range(m.n_segs):
            keys = set(m.keys[s])
            ids = np.concatenate([rows[:, s] for rows, _ in W.expect(m, "regex", oracle)])
            assert (ids != 0xFFFFFFFF).any(), f"{at}: no regex key in segment {s}"
            assert any("body:" + text in keys for opts in W.expect(m, "suggest", oracle) for text, _, _ in opts), (at, s)
        for s in touched(op, after):
            alive = ~m.dead(s)
            if not alive.any():
                continue
            want = W.expect(m, "date_aggs", oracle)
            assert any(m.ts[s][d] for q in want["docs"] for d in live_in(m, s, q)), f"{at}: date_aggs, segment {s}"
            passes = m.filter_masks()["f_nested"][s]
            assert (passes & alive).any() and (~passes & alive).any(), f"{at}: the nested tree in segment {s}"
            want = W.expect(m, "nested", oracle)
            rows = [r for r in (want["bool"], want["scan"]["rows"])]
            assert want["bitmaps"][s].any() and any((r[1][q, :int(r[3][q])] == s).any() for r in rows for q in range(len(r[3]))), \
                f"{at}: nested rows, segment {s}"
            # top_hits: a hit of the root's lists or of a key's list; composite: a doc with a key and a number among the
            # aggregated ones; the compound request: a doc of some matched set, and a row of some page
            want = W.expect(m, "top_hits", oracle)
            assert any((nd["seg"][q, r, :int(nd["count"][q, r])] == s).any() for nd in want["lists"]
                       for q in range(W.NQ) for r in range(nd["count"].shape[1])), f"{at}: top_hits, segment {s}"
            hits = W.TW.hits_of(W.all_hits(m, oracle))
            assert any(sg == s and m.kw[s][d] and m.num[s][d] for h in hits for sg, d, _ in h), f"{at}: composite, segment {s}"
            assert all(n > W.COMPOSITE["size"] for n in W.expect(m, "composite", oracle)["tuples"])   # more tuples than a page
            want = W.expect(m, "request", oracle)
            assert any(sg == s for rows in want["sets"] for sg, _, _ in rows), f"{at}: request, segment {s}"
            assert any((want["page"][1][q, :int(want["page"][3][q])] == s).any() for q in range(W.NQ)), f"{at}: request rows, segment {s}"
            hits, items = W.highlight_hits(m), W.expect(m, "highlight", oracle)
            here = [it[0] for hq, iq in zip(hits, items) for (sg, _), it in zip(hq, iq) if sg == s]
            assert here and (all(st == N.HL_NO_TEXT for st, _ in here) if m.text[s] is None else any(fr for _, fr in here)), \
                f"{at}: highlight, segment {s}"
            want = W.expect(m, "highlight_batch", oracle)
            doc, seg, _, count = want["rows"]
            here = [want["items"][q][i][0] for q in range(W.NQ) for i in range(int(count[q])) if seg[q, i] == s]
            assert here and (m.text[s] is None or any(fr for _, fr in here)), f"{at}: highlight_batch, segment {s}"


@pytest.mark.parametrize("name", W.SCENARIOS)
def test_term_buckets_background_follows_every_step(states, oracle, name):
    """every step moves the background count of a key that some query's foreground holds (tombstones, the segment
    list; test_an_unshifted_resource_... has the reject bitmap), and the per-segment mode the expectation is made in
    (the reference, literally) says what the all-segment mode (the device's counting) says: nothing is truncated"""
    from tests import term_buckets_ref as TB
    for label, op, before, after in states[name]:
        a, b = (W.expect(m, "term_buckets", oracle)["nodes"]["sig"] for m in (before, after))
        moved = [(q, x["key"]) for q in range(W.NQ) for x in a[q]["buckets"] for y in b[q]["buckets"]
                 if x["key"] == y["key"] and x["bg_count"] != y["bg_count"]]
        assert moved, f"{name} / {label}"
        for m in (before, after):
            want = W.expect(m, "term_buckets", oracle)
            dead = [None if s.deleted is None else set(int(d) for d in np.nonzero(m.dead(i))[0]) for i, s in enumerate(m.segs)]
            docs = [[(s, d) for s, d, _ in h] for h in W.TW.hits_of(W.all_hits(m, oracle))]
            for node, body in W.TERM_BUCKETS.items():
                flat = [TB.respond(body, want["cols"], m.n_docs(), dead, want["masks"], d, False) for d in docs]
                assert [TB.strip(r) for r in flat] == [TB.strip(r) for r in want["nodes"][node]], (name, label, node)
                assert all(r["buckets"] for r in flat)


def test_the_highlight_kinds_see_both_a_term_and_a_phrase(oracle):
    m, _ = W.build()
    frags = [f for kind in ("highlight", "highlight_batch")
             for q in (W.expect(m, kind, oracle) if kind == "highlight" else W.expect(m, kind, oracle)["items"])
             for it in q for f in it[0][1]]
    inner = [f[f.find(b"<b>") + 3:f.find(b"</b>")] for f in frags]
    assert any(b" " in x or b"," in x for x in inner) and any(x.isalnum() for x in inner)   # a phrase match, a term match
    assert any(x != x.lower() for x in inner)                                                # ASCII case folding


def test_every_resource_is_read_by_some_kind():
    assert set(r for reads in W.READS.values() for r in reads) == set(W.RESOURCES)
    assert set(W.READS) == set(W.KINDS) and set(W.PREPARED) <= set(W.KINDS)


@pytest.mark.parametrize("name", W.SCENARIOS)
def test_vector_boundaries_are_clear_of_near_ties(states, oracle, name):
    """tests/test_gpu_vector_search.py orders rows only away from near-ties (its queries keep a gap of 1e-4 at every
    cand boundary): every state the device test visits has that gap"""
    models = [states[name][0][2]] + [after for _, _, _, after in states[name]]
    for m in models:
        gap = W.vector_gaps(m, oracle)
        # (0.0: an exact tie, which that test orders by (segment, doc) exactly; the compaction has them while the
        #  merged segment and the two it replaces hold the same vectors)
        assert gap >= 1e-4 or (gap == 0.0 and name == "compaction"), gap
        assert W.hybrid_gaps(m, oracle) >= 4e-5                               # tests/test_gpu_hybrid.py: GAP


def test_vector_boundaries_of_the_states_outside_the_step_lists(oracle):
    """the compaction goes on down to one segment, and test_add checks vector search before the second registration"""
    m, steps = W.scenario("compaction")
    for _, op in steps:
        W.apply(m, op)
    m.remove(0)
    m.remove(0)
    assert m.n_docs() == [98]
    assert W.vector_gaps(m, oracle) >= 1e-4 and W.hybrid_gaps(m, oracle) >= 4e-5
    for kind in W.KINDS:   # every kind has an expectation over one segment
        assert W.expect(m, kind, oracle) is not None
    m, steps = W.scenario("add")
    W.apply(m, steps[0][1])
    assert W.vector_gaps(W.without_registration(m, 4), oracle) >= 1e-4


def test_states_before_registration_after_add(oracle):
    """what the header says of a segment added after a resource: no phrase holds a doc of it (no positions), the
    extra vector field holds no vector there while the embedded store does — and both show in the expectation"""
    m, steps = W.scenario("add")
    W.apply(m, steps[0][1])
    bare = W.without_registration(m, 4)
    _, seg, _, count = W.expect(bare, "phrase", oracle)
    assert not any((seg[q, :int(count[q])] == 4).any() for q in range(len(count)))
    _, seg_full, _, count_full = W.expect(m, "phrase", oracle)
    assert any((seg_full[q, :int(count_full[q])] == 4).any() for q in range(len(count_full)))
    assert W.differs(bare, m, "phrase", oracle) and W.differs(bare, m, "vector", oracle)
    maps = [mp for _, _, per_clause in W.expect(bare, "vector", oracle) for mp in per_clause[1:]]
    assert not any(s == 4 for mp in maps for s, _ in mp)                      # extra field: nothing in segment 4
    emb = [per_clause[0] for _, _, per_clause in W.expect(bare, "vector", oracle)]
    assert any(s == 4 for mp in emb for s, _ in mp)                           # embedded store: it is there
