"""The lifecycle world (tests/lifecycle_world.py) proves, with the references alone, that the device cases of
tests/test_gpu_lifecycle.py cannot pass vacuously:

  * every step of every scenario changes what every kind is expected to return (two kinds are by contract the same
    across a delete: a dictionary holds no tombstone, and a rerank scores the candidates it is handed; that
    sameness is what is asserted for them, here and on the device);
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
        for kind in W.KINDS:   # and a current hit of every kind that a delete shows in
            if kind not in W.SAME_UNDER_DELETE:
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
