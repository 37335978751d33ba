"""slg_highlight_batch and slg_batch_highlight on the device against tests/highlight_ref.py (the reference's loop
over Python's `re`).  The bar is byte equality of every fragment string; every world's items go to the device in one
call, twice, and the two answers are compared.  The worlds are tests/highlight_worlds.py."""
import numpy as np
import pytest

from searchlite_amd import _native as N
from searchlite_amd.highlight import highlight_spec as spec, snippet_spec
from tests import highlight_ref as R
from tests import highlight_worlds as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    return sa


def segment(gpu, bodies):
    """A segment of len(bodies) docs in the given order; bodies are what the searches of the batch form see."""
    b = gpu.SegmentBuilder(["body"])
    for i, body in enumerate(bodies):
        b.add_document(f"{i:07d}", {"body": body})
    return b.build()


def with_field(sp, field):
    return dict(sp, text_field=field)


def twice(fn):
    a, b = fn(), fn()
    assert a == b, "two runs of one call differ"
    return a


@pytest.mark.parametrize("world", sorted(W.WORLDS))
def test_world_equals_the_reference(gpu, world):
    cases = W.WORLDS[world]()
    texts, doc_of = W.layout(cases)
    want = W.expected(cases)
    with gpu.GpuIndex([segment(gpu, ["x"] * len(texts))]) as ix:
        field = ix.add_text_field([texts])
        hits = [[(0, d)] for d in doc_of]
        specs = [[with_field(c["spec"], field)] for c in cases]
        got = twice(lambda: ix.highlight(hits, specs))
    assert len(got) == len(cases)
    n_host = 0
    for c, g, w in zip(cases, got, want):
        assert g == [[w]], c["name"]
        n_host += w[0] == N.HL_HOST
    # the HOST items are exactly the docs with a byte >= 0x80 (W.expected marks those), and they stay few
    assert n_host == sum(any(b >= 0x80 for b in c["text"]) for c in cases) <= len(cases) // 10


def test_the_last_doc_ends_flush_with_the_store(gpu):
    """a match ending at the store's last byte, at every alignment of that byte in its 16-byte line"""
    for pad in range(0, 17):
        texts = [b"#" * pad, b"zz rust"]
        with gpu.GpuIndex([segment(gpu, ["x", "x"])]) as ix:
            f = ix.add_text_field([texts])
            got = ix.highlight([[(0, 1)]], [[spec(f, ["rust"])]])
        assert got == [[[(N.HL_OK, [b"zz <em>rust</em>"])]]], pad


def test_statuses_mixed_in_one_call_and_the_item_order(gpu):
    t0 = [b"rust here", "café rust".encode(), b"", b"rust\x80", b"\xffrust go", b"go rust"]
    t1 = [b"segment one rust", b"nothing"]
    with gpu.GpuIndex([segment(gpu, ["x"] * len(t0)), segment(gpu, ["x"] * len(t1)), segment(gpu, ["x"])]) as ix:
        fa = ix.add_text_field([t0, t1, None])     # segment 2 has no store in fa
        fb = ix.add_text_field([None, t1, [None]])   # segment 0 none in fb; segment 2: a doc without the field
        sa_, sb_ = spec(fa, ["rust"]), spec(fb, ["rust", "one"], [["segment", "one"]], pre_tag="[", post_tag="]")
        hits = [[(0, 0), (0, 1), (1, 0)], [], [(0, 2), (2, 0), (0, 3), (0, 4), (0, 5), (1, 1)]]
        specs = [[sa_, sb_], [sa_], [sb_, sa_]]
        got = twice(lambda: ix.highlight(hits, specs))
    ok, host, none = N.HL_OK, N.HL_HOST, N.HL_NO_TEXT
    assert got[0] == [[(ok, [b"<em>rust</em> here"]), (none, [])],
                      [(host, []), (none, [])],
                      [(ok, [b"segment one <em>rust</em>"]), (ok, [b"[segment one] [rust]"])]]
    assert got[1] == []
    assert got[2] == [[(none, []), (ok, [])],          # an empty text: OK, no fragments
                      [(ok, []), (none, [])],          # a doc without the field is an empty text; fa has no store there
                      [(none, []), (host, [])],        # a byte >= 0x80 at the last byte
                      [(none, []), (host, [])],        # ... at the first
                      [(none, []), (ok, [b"go <em>rust</em>"])],
                      [(ok, []), (ok, [])]]


def bodies_and_texts():
    """docs for the batch form: the body decides which query finds a doc, the text is what is highlighted"""
    rng = __import__("random").Random(9)
    bodies, texts = [], []
    for i in range(40):
        words = ["rust"] * (1 + i % 3) if i % 2 == 0 else ["go"]
        if i in (5, 7, 11):
            words.append("rare")
        bodies.append(" ".join(words))
        texts.append(W.soup(rng, 30 + 37 * i))
    return bodies, texts


def host_form_on_fetched(ix, batch, specs):
    doc, seg, _, count = batch.fetch()
    hits = [[(int(seg[q, i]), int(doc[q, i])) for i in range(int(count[q]))] for q in range(len(count))]
    return hits, ix.highlight(hits, specs)


def test_batch_form_on_a_plain_batch(gpu):
    from searchlite_amd.segment import fold_terms, parse_query_terms, resolve_query
    bodies, texts = bodies_and_texts()
    half = len(bodies) // 2
    segs = [segment(gpu, bodies[:half]), segment(gpu, bodies[half:])]
    with gpu.GpuIndex(segs) as ix:
        f = ix.add_text_field([texts[:half], texts[half:]])
        ids, w, offs = [], [], [0]
        for q in ("rust", "rare", "absentword", "go"):          # count == k, count < k, count == 0, count == k
            t, ww = resolve_query(ix.segments, fold_terms(parse_query_terms(q, "body")))
            ids.append(t)
            w.append(ww)
            offs.append(offs[-1] + len(ww))
        k = 8
        b = ix.prepare(np.array(offs, np.uint32), np.concatenate(ids), np.concatenate(w), k)
        b.run()
        specs = [[spec(f, ["rust", "go"], [["new", "york"]], fragment_size=30, number_of_fragments=3), snippet_spec(f, ["a", "b"])]] * 4
        got = twice(lambda: b.highlight(specs))
        hits, want = host_form_on_fetched(ix, b, specs)
        b.close()
    assert [len(h) for h in hits] == [k, 3, 0, k]
    assert got == want
    for q, hq in enumerate(hits):
        for i, (s, d) in enumerate(hq):
            t = (texts[:half], texts[half:])[s][d]
            assert got[q][i] == [(N.HL_OK, R.highlight_spec_ref(t, sp)) for sp in specs[q]]


def test_batch_form_on_a_scan_batch(gpu):
    bodies, texts = bodies_and_texts()
    with gpu.GpuIndex([segment(gpu, bodies)]) as ix:
        f = ix.add_text_field([texts])
        few = np.zeros(len(bodies), bool)
        few[[3, 17, 38]] = True
        f_few, f_none = ix.add_filter([few]), ix.add_filter([np.zeros(len(bodies), bool)])
        k = 8
        b = ix.prepare_scan([{"match_all": {}}] * 3, k, q_filter=[-1, f_few, f_none])
        b.run()
        specs = [[spec(f, ["rust", "new"], fragment_size=50, number_of_fragments=2)]] * 3
        got = twice(lambda: b.highlight(specs))
        hits, want = host_form_on_fetched(ix, b, specs)
        b.close()
    assert [len(h) for h in hits] == [k, 3, 0]
    assert got == want and sorted(d for _, d in hits[1]) == [3, 17, 38]
    for q, hq in enumerate(hits):
        for i, (_, d) in enumerate(hq):
            assert got[q][i] == [(N.HL_OK, R.highlight_spec_ref(texts[d], specs[q][0]))]


def test_lifecycle(gpu):
    from searchlite_amd.segment import fold_terms, parse_query_terms, resolve_query
    t0, t1, t2 = [b"zero rust", b"zero go rust"], [b"one rust one"], [b"two rust", b"two two rust"]
    s0, s1, s2 = segment(gpu, ["rust", "rust"]), segment(gpu, ["rust"]), segment(gpu, ["rust", "rust"])
    with gpu.GpuIndex([s0, s1], tuning={"updatable": 1}) as ix:
        f = ix.add_text_field([t0, t1])
        sp = spec(f, ["rust"], pre_tag="<", post_tag=">")
        hits = [[(0, 0), (0, 1), (1, 0)]]
        before = ix.highlight(hits, [[sp]])
        assert before == [[[(N.HL_OK, [b"zero <rust>"])], [(N.HL_OK, [b"zero go <rust>"])], [(N.HL_OK, [b"one <rust> one"])]]]
        # a batch prepared now answers from its own state whatever happens to the index afterwards
        t, w = resolve_query(ix.segments, fold_terms(parse_query_terms("rust", "body")))
        b = ix.prepare(np.array([0, 1], np.uint32), t, w, 4)
        b.run()
        held = b.highlight([[sp]])
        assert sorted(x[0][1][0] for x in held[0]) == sorted(x[0][1][0] for x in before[0])
        # a delete changes nothing
        ix.update_deleted(0, np.array([0b01], np.uint8), 1.0)
        assert ix.highlight(hits, [[sp]]) == before
        # add a segment: NO_TEXT until the field is registered over all segments, then its fragments
        assert ix.add_segment(s2) == 2
        new_hits = [[(2, 0), (2, 1), (0, 1)]]
        assert ix.highlight(new_hits, [[sp]]) == [[[(N.HL_NO_TEXT, [])], [(N.HL_NO_TEXT, [])], [(N.HL_OK, [b"zero go <rust>"])]]]
        f2 = ix.add_text_field([t0, t1, t2])
        sp2 = with_field(sp, f2)
        assert ix.highlight(new_hits, [[sp2]]) == [[[(N.HL_OK, [b"two <rust>"])], [(N.HL_OK, [b"two two <rust>"])],
                                                    [(N.HL_OK, [b"zero go <rust>"])]]]
        # remove segment 0: the others keep their fragments under their new ordinals, in both fields
        ix.remove_segment(0)
        assert ix.highlight([[(0, 0), (1, 1)]], [[sp2, sp]]) == [[[(N.HL_OK, [b"one <rust> one"])] * 2,
                                                                  [(N.HL_OK, [b"two two <rust>"]), (N.HL_NO_TEXT, [])]]]
        with pytest.raises(N.SlgError) as e:
            ix.highlight([[(2, 0)]], [[sp2]])        # the segment list is one shorter now
        assert e.value.code == N.ERR_INVALID
        # the batch prepared before all this still answers from its own state
        assert b.highlight([[sp]]) == held
        ix.remove_text_field(f)
        with pytest.raises(N.SlgError) as e:
            ix.highlight([[(0, 0)]], [[sp]])
        assert e.value.code == N.ERR_INVALID and "unknown text field id" in e.value.msg
        assert b.highlight([[sp]]) == held
        b.close()


def test_size_query_and_capacities_one_too_small(gpu):
    import ctypes as C
    from searchlite_amd.highlight import pack_specs
    with gpu.GpuIndex([segment(gpu, ["x", "x"])]) as ix:
        f = ix.add_text_field([[b"rust go rust", b"go"]])
        soffs, arr, keep = pack_specs([[spec(f, ["rust", "go"], fragment_size=4, number_of_fragments=2, pre_tag="<", post_tag=">")]])
        hoffs, seg, doc = np.array([0, 2], np.uint32), np.zeros(2, np.uint32), np.array([0, 1], np.uint32)

        def call(out):
            return ix._lib.slg_highlight_batch(ix._h, 1, hoffs.ctypes.data, seg.ctypes.data, doc.ctypes.data,
                                               soffs.ctypes.data, arr, C.addressof(out))
        size = N.HlOut(struct_size=C.sizeof(N.HlOut))
        assert call(size) == N.OK
        # doc 0: "rust" -> "<rust>", "<go>" at start 3: "t go" -> "t <go>"; doc 1: "<go>"
        assert (size.n_items, size.n_frags, size.text_bytes) == (2, 3, 6 + 6 + 4)
        guard = 0xA5
        for short in (None, "item_capacity", "frag_capacity", "text_capacity"):
            st, io = np.full(2 + 1, guard, np.uint8), np.zeros(2 + 1, np.uint32)
            to, tx = np.zeros(3 + 1, np.uint32), np.full(16 + 1, guard, np.uint8)
            out = N.HlOut(C.sizeof(N.HlOut), 2, 3, 16, st.ctypes.data, io.ctypes.data, to.ctypes.data, tx.ctypes.data, 0, 0, 0)
            if short:
                setattr(out, short, getattr(out, short) - 1)
            rc = call(out)
            assert st[2] == guard and tx[16] == guard
            if short:
                assert rc == N.ERR_INVALID and short in N.last_error()
                assert (tx == guard).all()      # nothing was emitted
            else:
                assert rc == N.OK and io.tolist() == [0, 2, 3] and to.tolist() == [0, 6, 12, 16]
                assert tx[:16].tobytes() == b"<rust>t <go><go>" and st[:2].tolist() == [N.HL_OK, N.HL_OK]
        del keep


def test_refusals_reach_the_caller_with_their_messages(gpu):
    with gpu.GpuIndex([segment(gpu, ["x"])]) as ix:
        f = ix.add_text_field([[b"rust"]])
        with pytest.raises(N.SlgError) as e:
            ix.highlight([[(0, 0)], [(0, 0)]], [[spec(f, ["rust"])], [spec(f, ["rust"]), spec(f, ["café"])]])
        assert e.value.code == N.ERR_UNSUPPORTED and "query 1 field spec 1" in e.value.msg
        with pytest.raises(N.SlgError) as e:
            ix.highlight([[(0, 1)]], [[spec(f, ["rust"])]])
        assert e.value.code == N.ERR_INVALID
        assert ix.highlight([[(0, 0)]], [[spec(f, ["rust", ""], [[]])]]) == [[[(N.HL_OK, [b"<em>rust</em>"])]]]
