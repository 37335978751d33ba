"""Regex term expansion on the device (slg_expand_batch, kind SLG_EXPAND_REGEX): the pattern compiled on the host to
a minimised byte DFA, the device walking every key of the range through it.

Expected: tests/regex_ref.py, the reference's expand_regex restated line for line with Python's `re` as the matcher
(pinned in tests/test_regex_ref.py).  Bar: exact equality of keys, order and term-id rows; every batch runs twice
and must say the same.  The dictionaries are synthetic and tiny; every boundary that depends on the scan's geometry
comes from the constants the library exports.  Every world's requests go to the device in ONE call.
"""
import random

import numpy as np
import pytest

from searchlite_amd import _native as N
from tests import expand_ref as R
from tests import expand_util as U
from tests import expand_worlds as W
from tests import regex_ref as RR
from tests import regex_util as X

pytestmark = pytest.mark.gpu

rx = X.regex


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
    """one expand() call over reqs, twice; every request's rows against the restatements"""
    world = X.World(seg_keys)
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
        assert ids.tolist() == ids2.tolist() and dist.tolist() == dist2.tolist(), what
    return got


def keys_of(seg_keys, got_rows, seg=0):
    return [seg_keys[seg][i] for i in got_rows[0][:, seg].tolist()]


def test_range_wave_and_chunk_edges(gpu):
    """ranges of 1, wave - 1 .. 2 x chunk + 1 keys (tests/expand_worlds.py); passing keys only first, only last, on
    both sides of every wave, workgroup and chunk boundary; caps of 0, of 1, of exactly the passing keys (E: 50 of
    them) and of one past (M: 51); the bare key; a literal prefix that narrows the range to one key"""
    reqs = []
    for n in W.RANGE_SIZES:
        f = f"r{n}"
        reqs += [rx(f, ".*F.*"), rx(f, "[a-z]+.*L"), rx(f, ".*S.*"), rx(f, ".*E.*", 50), rx(f, ".*E.*", 49), rx(f, ".*M", 50),
                 rx(f, ".*M", 51), rx(f, ".*M", 1), rx(f, ".*", 50), rx(f, ".*", 1), rx(f, ".*", 0), rx(f, "[a-z]{4}[A-Z]*", 1024),
                 rx(f, W.word(n - 1) + ".*", 5), rx(f, "^" + W.word(0) + "F.*", 5), rx(f, "zzzzz.*", 5), rx(f, "(" + W.word(0) + "F.*)", 5)]
    for n in (1, W.WAVE, W.WAVE + 1, W.CHUNK + 1):
        reqs += [rx(f"b{n}", ".*", 1024), rx(f"b{n}", "", 5), rx(f"b{n}", "()", 5), rx(f"b{n}", "a*", 5)]
    reqs += [rx("body", ".*"), rx("bod", ".*"), rx("body2", "y|x"), rx("r", ".*"), rx("zz", "l.*"), rx("zz", "last"), rx("zzz", ".*")]
    got = check_world(gpu, W.range_world(), reqs)
    assert sum(len(d) for _, d in got) > 3000                    # (the world does produce keys)


def test_an_empty_literal_prefix_scans_the_whole_field(gpu):
    """the whole dictionary as one range, and a field of four chunks with matches spread over all of them"""
    check_world(gpu, W.whole_world(), [rx("t", ".*", 1024), rx("t", ".b.*", 50), rx("t", "(a|b).c", 1024), rx("t", ".*z", 1024),
                                       rx("t", "[^a]..", 7), rx("t", "(?:" + W.word(W.CHUNK + W.WAVE, 3) + ")", 5)])
    seg_keys = W.dense_world()
    assert len(seg_keys[0]) > 3 * W.CHUNK
    reqs = [rx("d", p, mx) for p in (".*c", "(a|b)*abb", "a.*b.*c", ".", "..", "(.{3})+", "[^a]*", "(ab|c)+", ".*cc.*", "(c{7}|a{7})", "c{7}|a{7}")
            for mx in (1, 50, 1024)]
    got = check_world(gpu, seg_keys, reqs)
    ends = keys_of(seg_keys, got[reqs.index(rx("d", "(c{7}|a{7})", 50))])
    assert ends == ["d:aaaaaaa", "d:ccccccc"]                    # the first chunk and the last key of the last
    # (without the group the literal prefix is "c": the reference scans only that range)
    assert keys_of(seg_keys, got[reqs.index(rx("d", "c{7}|a{7}", 50))]) == ["d:ccccccc"]


def test_key_shapes(gpu):
    """1-byte terms, a 300-byte term (longer than any pattern), 2- / 3- / 4-byte chars, U+000A against '.', [^a]
    and a\\nb (whose literal prefix is the letters "anb": the reference's quirk)"""
    terms = ["a", "b", "z" * 300, "z" * 299, "é", "aé", "éa", "東京", "東亰", "😀", "a😀", "😀a", "a\nb", "anb", "\n", "a\n", "ab", "abc",
             "a.b", "€", "\x7f", "\u0080", "߿", "ࠀ", "￿", "\U00010000", "\U0010ffff"]
    seg_keys = [["kw:" + t for t in terms] + ["kw:", "kx:a"]]
    pats = [".", "..", "...", "[^a]", "[^a]*", r"a\nb", "a\nb", "a[\n]b", "a.b", r"a\.b", ".*\n.*", "(zz)+", "z+", "z(zz)+", "z{200}z*", ".*", "(.|\n)*",
            "東.", "[東-😀]+", "😀.?", ".é|é.", "[^é]+", "[\x7f-\u0080]", "[߿-ࠀ]", "[￿-\U00010000]", "[^\x00-\U0010fffe]", "(a|b|é)"]
    reqs = [rx("kw", p, mx) for p in pats for mx in (50, 1)]
    seg = seg_keys[0]
    got = check_world(gpu, seg_keys, reqs)

    def found(p):
        return sorted(keys_of(seg_keys, got[reqs.index(rx("kw", p, 50))]))
    # spot checks by hand, on top of the restatement
    assert found(".") == sorted("kw:" + t for t in terms if len(t) == 1 and t != "\n")
    assert "kw:\n" in found("[^a]") and "kw:a" not in found("[^a]")
    assert found(r"a\nb") == [] and found("a\nb") == ["kw:a\nb"] and found("a.b") == ["kw:a.b", "kw:anb"]
    assert found("(zz)+") == ["kw:" + "z" * 300] and found("z(zz)+") == ["kw:" + "z" * 299]
    assert found("z+") == found("z{200}z*") == ["kw:" + "z" * 299, "kw:" + "z" * 300]
    assert len(seg) == len(terms) + 2


def literals_63():
    return "_" + "".join(chr(ord("0") + i) for i in range(10)) + "".join(chr(ord("A") + i) for i in range(26)) + \
        "".join(chr(ord("a") + i) for i in range(26))


def test_the_largest_automata(gpu):
    """a DFA of SLG_MAX_REGEX_STATES states (a transition into state 255), one whose table is 16 256 bytes and one
    at SLG_MAX_REGEX_TABLE itself (the LDS staging loop at its largest), each over a range that straddles a chunk"""
    S = N.MAX_REGEX_STATES
    filler = [W.word(i) for i in range(W.CHUNK + 76)]
    big = filler + ["a" * (S - 2), "a" * (S - 3), "a" * (S - 1), "a" * (S - 3) + "b", "z" * (S - 2), "z" * (S - 1), "az" * (S // 2 - 1),
                    "za" * (S // 2 - 1) + "b"]
    P = literals_63()
    wide = [P + w for w in filler] + [P + "z" * k for k in (187, 188, 189, 190, 191, 192)]
    seg_keys = [["big:" + t for t in big] + ["wide:" + t for t in wide]]
    most_states, t16256, t16384 = "[az]{%d}" % (S - 2), P + "{190}", P + "{%d}" % (S - 64)
    shapes = [(X.Dfa(p).n_states, X.Dfa(p).n_classes) for p in (most_states, t16256, t16384)]
    assert shapes == [(S, 2), (254, 64), (S, 64)] and 254 * 64 == 16256 and S * 64 == N.MAX_REGEX_TABLE
    reqs = [rx("big", most_states), rx("big", most_states, 1), rx("wide", t16256), rx("wide", t16384), rx("wide", P + "[a-z]{4}", 1024),
            rx("big", "[a-z]{4}", 1024)]
    got = check_world(gpu, seg_keys, reqs)
    sorted_big = R.sorted_keys(seg_keys[0][:len(big)])
    hits = keys_of(seg_keys, got[0])
    assert hits == ["big:" + "a" * (S - 2), "big:" + "az" * (S // 2 - 1), "big:" + "z" * (S - 2)]
    assert sorted_big.index(hits[0]) < W.CHUNK < sorted_big.index(hits[2])              # both sides of the chunk boundary
    assert keys_of(seg_keys, got[2]) == ["wide:" + P + "z" * 189] and keys_of(seg_keys, got[3]) == ["wide:" + P + "z" * 191]
    assert len(got[4][1]) == len(got[5][1]) == min(len(filler), N.MAX_EXPANSIONS) and len(filler) > W.CHUNK


def test_three_segments(gpu):
    """the per-segment cap behind the duplicates of earlier segments; the key past the cap in segment 0 that enters
    through segment 1; NO_TERM holes"""
    seg_keys = W.segments_world()
    reqs = [rx("body", "r[0-9]+", mx) for mx in (1, 2, 10, 40, 99, 100, 101, 1024)]
    reqs += [rx("body", "r0.*", mx) for mx in (1, 10, 99, 100)] + [rx("body", ".us.", mx) for mx in (1, 2, 3, 50)]
    reqs += [rx("body", "ru(st|sk|sh)", 50), rx("body", "(r|d|b)ust", 1), rx("title", ".*", 50), rx("nope", ".*", 50), rx("body", "r1.[01]", 3)]
    got = check_world(gpu, seg_keys, reqs)
    rows, _ = got[reqs.index(rx("body", "r[0-9]+", 10))]
    assert len(rows) == 30 and rows[10].tolist() == [10, 89, 10]          # r000 .. r029, ten per segment
    rows, _ = got[reqs.index(rx("body", "r1.[01]", 3))]
    # segment 0 takes r100? no: it holds r000 .. r099 only, so r10[01] enter through segment 2, past two segments' caps
    assert [seg_keys[2][i] for i in rows[:, 2].tolist() if i != R.NO_TERM][-2:] == ["body:r100", "body:r101"]
    assert rows[-1].tolist()[:2] == [R.NO_TERM, R.NO_TERM]


def mixed_requests(vocab, n=300, seed=77):
    """tests/expand_worlds.py's seeded fuzzy / prefix / wildcard requests with every third one replaced by a regex:
    regex requests are interleaved with the other kinds, so their chunks are not contiguous in request order"""
    rng = random.Random(seed)
    reqs = W.random_requests(vocab, n)
    for i in range(0, n, 3):
        wd = rng.choice(vocab)
        f = rng.choice(("w", "w", "w", "x"))
        shape = rng.randrange(8)
        p = [wd[:rng.randrange(0, 3)] + ".*", "(a|b)" + wd[1:3] + ".*", "[ab]*é.*", wd[:1] + "[^a]+", ".*" + wd[-2:], wd,
             "(" + wd[:2] + "|" + wd[-2:] + ").{0,3}", "[^é]{%d,}" % rng.randrange(1, 6)][shape]
        reqs[i] = rx(f, p, rng.choice((0, 1, 5, 50, 1024)))
    return reqs


def test_mixed_batch_of_all_four_kinds(gpu):
    seg_keys, vocab = W.random_world()
    assert 2000 <= sum(len(k) for k in seg_keys) <= 3000
    reqs = mixed_requests(vocab)
    kinds = [r["kind"] for r in reqs]
    assert len(reqs) == 300 and {U.FUZZY, U.PREFIX, U.WILDCARD, X.REGEX} == set(kinds)
    assert any(kinds[i] == X.REGEX and kinds[i + 1] != X.REGEX and X.REGEX in kinds[i + 2:] for i in range(len(kinds) - 2))
    got = check_world(gpu, seg_keys, reqs)
    assert sum(len(d) for (_, d), k in zip(got, kinds) if k == X.REGEX) > 500
    # the C++ restatement of the reference's loop (the timing tool's yardstick) agrees too
    ref = U.reference_loop(reqs, [U.HostDict(k) for k in seg_keys], 2)
    for (a, b), (c, d) in zip(got, ref):
        assert a.tolist() == c.tolist() and b.tolist() == d.tolist()


def test_wildcards_written_as_regexes_return_the_same_rows(gpu):
    seg_keys, vocab = W.random_world()
    rng = random.Random(5)
    pats = set()
    while len(pats) < 50:
        wd = rng.choice(vocab)
        pats.add("".join(rng.choice((c, c, "*", "?")) for c in wd[:rng.randrange(1, 6)]))
    pats = sorted(pats)
    reqs = [U.wildcard("w", p, mx) for p in pats for mx in (5, 1024)] + [rx("w", RR.wildcard_as_regex(p), mx) for p in pats for mx in (5, 1024)]
    with open_world(gpu, seg_keys) as ix:
        got = ix.expand(reqs)
    half = len(reqs) // 2
    assert half == 100 and sum(len(d) for _, d in got[:half]) > 1000
    for (a, b), (c, d), r in zip(got[:half], got[half:], reqs):
        assert a.tolist() == c.tolist() and b.tolist() == d.tolist(), r


def test_index_states(gpu):
    """update_deleted keeps the dictionaries, a segment added later has none until it is set, a removed segment's
    goes with it: as for the other kinds"""
    from tests.util import random_segment
    rng = np.random.default_rng(5)
    seg0, seg1 = random_segment(rng, 300, 40, 12), random_segment(rng, 200, 40, 12)
    keys0 = [f"body:{W.word(i)}" for i in range(40)]
    keys1 = [f"body:{W.word(2 * i)}" for i in range(40)]
    req = rx("body", "aaa[a-m].*", 50)
    with gpu.GpuIndex([seg0, seg1]) as ix:
        ix.set_terms(0, keys0)
        with pytest.raises(N.SlgError) as ei:
            ix.expand([req])
        assert ei.value.code == N.ERR_INVALID and "segment 1" in ei.value.msg
        ix.set_terms(1, keys1)
        world = X.World([keys0, keys1])
        ids, dist = ix.expand([req])[0]
        assert ids.tolist() == world.want(req)[0].tolist() and len(dist) == 13
        ix.update_deleted(0, np.packbits(np.arange(300) < 7, bitorder="little"), 293.0)
        assert ix.expand([req])[0][0].tolist() == ids.tolist()
        keys2 = ["body:aaaa", "body:zzzz", "title:aaab"]
        ix.add_segment(W.dict_segment(keys2))
        with pytest.raises(N.SlgError) as ei:
            ix.expand([req])
        assert ei.value.code == N.ERR_INVALID and "segment 2" in ei.value.msg
        ix.set_terms(2, keys2)
        world = X.World([keys0, keys1, keys2])
        assert ix.expand([req])[0][0].tolist() == world.want(req)[0].tolist()
        ix.remove_segment(0)
        world = X.World([keys1, keys2])
        got = ix.expand([req, rx("body", "z+", 5)])
        assert got[0][0].tolist() == world.want(req)[0].tolist()
        assert got[1][0].tolist() == [[R.NO_TERM, 1]]


# ---- end to end ---------------------------------------------------------------------------------------------
CORPUS = [
    [("d1", "Rust is fast and rusty systems trust it"), ("d2", "the dusk of a bust"), ("d3", "rush to the café"),
     ("d4", "systems programming in rust"), ("d5", "naïve cafe owners rest")],
    [("e1", "rusk and ruse"), ("e2", "system of a dusk"), ("e3", "fast fest fist"), ("e4", "cafés and caffe")],
]


def test_search_patterns_is_the_plain_batch_of_the_references_keys(gpu):
    segs = []
    for docs in CORPUS:
        b = gpu.SegmentBuilder(["body"])
        for eid, text in docs:
            b.add_document(eid, {"body": text})
        segs.append(b.build())
    seg_sorted = [R.sorted_keys(s.term_dict) for s in segs]
    nodes = [(N.EXPAND_REGEX, "body", "ru(st|sk|sh).*", 50, 1.0), (N.EXPAND_REGEX, "body", ".*st", 50, 2.5),
             (N.EXPAND_REGEX, "body", "caf.s?", 1, 1.0), (N.EXPAND_REGEX, "body", "f[aei]st", 2, 0.5),
             (N.EXPAND_PREFIX, "body", "sys", 50, 1.0), (N.EXPAND_WILDCARD, "body", "?us?", 50, 3.0),
             (N.EXPAND_REGEX, "body", "zzz+", 50, 1.0), (N.EXPAND_REGEX, "body", "rust?", 50, 1.0)]
    fn = {N.EXPAND_REGEX: RR.expand_regex, N.EXPAND_PREFIX: R.expand_prefix, N.EXPAND_WILDCARD: R.expand_wildcard}
    offs, rows, weights, nleaves = [0], [], [], []
    for kind, field, value, mx, boost in nodes:
        keys = fn[kind](seg_sorted, field, value, mx)
        rows += [[s.term_id(k) for s in segs] for k in keys]
        weights += [np.float32(boost)] * len(keys)
        nleaves.append(1 if keys else 0)
        offs.append(len(rows))
    nq = len(nodes)
    plans = dict(q_leaf=np.zeros(len(rows), np.uint32), q_plan=np.zeros(nq, np.uint32), q_tie=np.zeros(nq, np.float32),
                 q_nleaves=np.array(nleaves, np.uint32))
    with gpu.GpuIndex(segs) as ix:
        ix.set_terms_from_segments()
        got = ix.search_patterns(nodes, 6)
        want = ix.search_plan(np.array(offs, np.uint32), np.array(rows, np.uint32).reshape(-1, len(segs)),
                              np.array(weights, np.float32), 6, **plans)
        with pytest.raises(N.SlgError) as ei:
            ix.search_patterns([(N.EXPAND_REGEX, "body", r"\d+", 50, 1.0)], 6)
        assert ei.value.code == N.ERR_UNSUPPORTED
        with pytest.raises(ValueError):
            ix.search_patterns([(N.EXPAND_FUZZY, "body", "rust", 50, 1.0)], 6)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    counts = got[3].tolist()
    assert counts[0] >= 3 and counts[6] == 0 and counts[7] == 2          # ("rust?" never yields "rus...": rust alone, 2 docs)
    assert got[2][1, 0] > 0                                               # (scores are real)
