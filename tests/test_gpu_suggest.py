"""The completion suggester on the device (slg_suggest_batch): plain prefix and fuzzy, scored by doc frequency.

Expected: tests/suggest_ref.py, the reference's suggester restated line for line and pinned to the reference's own
test in tests/test_suggest_ref.py.  Bar: exact equality of texts, order, doc_freq and the scores' f32 bit patterns;
no tolerance anywhere.  The dictionaries (tests/suggest_worlds.py) are synthetic and small; every world's requests
go to the device in ONE call, twice, and the two answers are compared.
"""
import random

import numpy as np
import pytest

from searchlite_amd import _native as N
from searchlite_amd.searcher import suggest_request as req
from tests import suggest_ref as R
from tests import suggest_worlds as W

pytestmark = pytest.mark.gpu

CAND, MIN_SCAN = W.CAND, W.MIN_SCAN


@pytest.fixture(scope="module")
def gpu():
    import searchlite_amd as sa
    from searchlite_amd import searcher
    assert searcher.device_count() >= 1
    return sa


def open_world(gpu, segs):
    ix = gpu.GpuIndex([W.df_segment(s) for s in segs])
    ix.set_terms_from_segments()
    return ix


def short(r):
    return {k: (v if len(str(v)) < 40 else str(v)[:40] + "...") for k, v in r.items()}


def check_index(ix, world, reqs):
    got = [R.bits(o) for o in ix.suggest(reqs)]
    again = [R.bits(o) for o in ix.suggest(reqs)]
    assert len(got) == len(reqs)
    for r, g, g2 in zip(reqs, got, again):
        assert g == world.want(r), short(r)
        assert g == g2, short(r)                     # the same from run to run
    return got


def check_world(gpu, segs, reqs):
    """one suggest() call over reqs; every request's options against tests/suggest_ref.py"""
    with open_world(gpu, segs) as ix:
        return check_index(ix, W.World(segs), reqs)


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def test_constants_are_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "searchlite_gpu.h")).read()
    for name, val in (("MAX_SUGGEST_CANDIDATES", N.MAX_SUGGEST_CANDIDATES), ("SUGGEST_MIN_SCAN", N.SUGGEST_MIN_SCAN),
                      ("SUGGEST_MERGE_WORKGROUP", N.SUGGEST_MERGE_WORKGROUP)):
        assert int(re.search(r"#define SLG_%s (\d+)u" % name, text).group(1)) == val
    assert N.SUGGEST_MERGE_WORKGROUP >= N.MAX_SUGGEST_CANDIDATES            # a thread per candidate


def test_plain_cap_boundaries(gpu):
    """caps 64 / 65 / 255 / 256 / 256 (size 300) over ranges of 1, 63 .. 65 and 255 .. 257 passing keys: the cap before,
    on and after the end of the range; a bare key and df-0 keys that neither pass nor count; sibling fields"""
    reqs = W.plain_requests()
    got = check_world(gpu, W.plain_world(), reqs)
    by = {(r["field"], r["size"]): len(g) for r, g in zip(reqs, got) if r["term"] == ""}
    assert by[(f"p{CAND + 1}", 300)] == CAND and by[(f"p{CAND}", 300)] == CAND and by[(f"p{CAND - 1}", 300)] == CAND - 1
    assert by[("p1", 300)] == 1 and by[(f"p{MIN_SCAN + 1}", 300)] == MIN_SCAN + 1 and by[("bod", 5)] == 1


def test_fuzzy_scan_boundaries(gpu):
    """ranges of 1, chunk - 1 .. chunk + 1 and 2 chunks + 1 keys with passing keys first, last and on both sides of
    every wave, slab and chunk edge; 300 passing keys over four chunks with the cap reached in the last"""
    reqs = W.fuzzy_requests()
    got = check_world(gpu, W.fuzzy_world(), reqs)
    full = got[reqs.index(req("sp", W.TERM, 256, W.fz(max_expansions=300)))]
    assert len(full) == CAND and sum(len(g) for g in got) > 500
    marks = W.spread_marks()
    assert marks[CAND - 1] >= 3 * W.CHUNK and len(marks) == 300                # (the cap does land in the last chunk)
    n = W.FUZZY_RANGES[-1]
    assert len(got[reqs.index(req(f"f{n}", W.TERM, 50, W.fz()))]) == len(W.fuzzy_marks(n))


WORDS = ["rust", "rusk", "rusts", "trust", "rut", "ust", "rsut", "bust", "best", "ru", "r", "rs", "rus", "rustabc",
         "rustab", "rusta", "dusk", "urst", "ruts", "café", "cafe", "caffe", "cafés", "東京", "東亰", "東京都", "😀a", "😀b",
         "a😀", "ééé", "éééé", "z" * 300]


def test_fuzzy_options(gpu):
    """distance 0, 1 and 2 together (the exact term at weight 1); max_edits 0 (nothing) and 3 (as 2); a term shorter
    than min_length; max_expansions 0, below size (the cap is size) and 300 (256); prefix_length 0 and beyond the term"""
    segs = [[("body:" + w, 1 + i % 7) for i, w in enumerate(WORDS)] + [("body:", 3), ("kw:rust", 1)]]
    reqs = []
    for term in ("rust", "rusk", "rsut", "r", "ru", "cafe", "café", "東京", "😀a", "éééé", "", "z" * 128):
        for me in (0, 1, 2, 3):
            for pl in (0, 1, 4, 200):
                reqs.append(req("body", term, 10, dict(max_edits=me, prefix_length=pl, min_length=0)))
    reqs += [req("body", "ru", 5, {}), req("body", "rus", 5, {}), req("body", "rust", 5, dict(max_expansions=0)),
             req("body", "rust", 4, dict(max_expansions=2, max_edits=2)), req("body", "rust", 9, dict(max_expansions=300, max_edits=2)),
             req("body", "rust", 1, dict(max_expansions=1, max_edits=2))]
    got = check_world(gpu, segs, reqs)
    df = dict(segs[0])
    two = {t: s for t, s, _ in got[reqs.index(req("body", "rust", 10, dict(max_edits=2, prefix_length=1, min_length=0)))]}
    third = np.float32(1.0) / np.float32(3.0)
    assert two["rust"] == f32bits(df["body:rust"]) and two["rusk"] == f32bits(np.float32(0.5) * np.float32(df["body:rusk"]))
    assert two["rsut"] == f32bits(third * np.float32(df["body:rsut"])) and "trust" not in two
    assert got[reqs.index(req("body", "ru", 5, {}))] == [] and got[reqs.index(req("body", "rust", 5, dict(max_expansions=0)))] == []
    assert len(got[reqs.index(req("body", "rust", 4, dict(max_expansions=2, max_edits=2)))]) == 4


def test_three_segments(gpu):
    """a text in one, two and three segments; the cap exhausted inside a segment, so a later copy of a text is not
    added; a segment whose range is empty"""
    ms = [(f"t:m{W.word(i)}", 1 + i % 5) for i in range(70)]
    s0 = [("t:", 4), ("t:aa", 5), ("t:ab", 0), ("t:ac", 7), ("t:b", 1), ("t:both", 3), ("t:all", 2), ("u:only0", 2)] + ms
    s1 = [("t:all", 6), ("t:both", 1), ("t:ac", 0), ("v:x", 1)] + ms[::2]
    s2 = [("t:all", 1), ("t:zz", 8), ("t:aa", 1), ("u:only0", 1), ("u:only2", 1)]
    reqs = [req("t", t, size) for t in ("", "a", "m", "b", "al") for size in (1, 3, 13, 15, 16, 22, 60)]
    reqs += [req("t", t, size, dict(max_edits=2, prefix_length=pl, min_length=0, max_expansions=mx))
             for t in ("all", "aa", "maaaa") for size in (1, 5, 90) for pl in (0, 1) for mx in (1, 3, 50)]
    reqs += [req("u", "", 5), req("v", "", 5), req("u", "only", 5, {})]
    got = check_world(gpu, [s0, s1, s2], reqs)
    all60 = {t: (s, d) for t, s, d in got[reqs.index(req("t", "", 60))]}
    assert all60["all"] == (f32bits(9.0), 9) and all60["both"] == (f32bits(4.0), 4) and all60["zz"] == (f32bits(8.0), 8)
    cut = {t: d for t, _, d in got[reqs.index(req("t", "", 16))]}              # cap 80: 75 of segment 0, 5 of segment 1
    assert cut["all"] == 8 and "zz" not in cut
    assert got[reqs.index(req("v", "", 5))] == [("x", f32bits(1.0), 1)]        # segments 0 and 2: empty ranges


def test_score_arithmetic_is_sequential_and_unfused(gpu):
    """one text over three segments at distance 2, its dfs found by a search: another order of the sum gives other
    f32 bits, and so does a fused multiply-add; the device must give the reference's"""
    third = np.float32(1.0) / np.float32(3.0)

    def seq(dfs):
        s = np.float32(0.0)
        for d in dfs:
            s = np.float32(s + np.float32(third * np.float32(d)))
        return f32bits(s)

    rng = np.random.RandomState(7)
    found = []
    for _ in range(5000):
        dfs = [int(x) for x in rng.randint(1, 5000, 3)]
        fused = np.float32(0.0)
        for d in dfs:
            fused = np.float32(np.float64(third) * np.float64(d) + np.float64(fused))   # one rounding per step: an fma
        others = {seq(p) for p in ([dfs[0], dfs[2], dfs[1]], [dfs[1], dfs[0], dfs[2]], dfs[::-1])}
        if others != {seq(dfs)} and seq(dfs) != f32bits(fused):
            found.append(dfs)
            if len(found) == 4:
                break
    assert len(found) == 4                                                     # the search did find such inputs
    segs = [[(f"t{j}:abcd", dfs[s]) for j, dfs in enumerate(found)] + [("t0:zzzzzzzz", 1)] for s in range(3)]
    reqs = [req(f"t{j}", "abxy", 3, dict(max_edits=2, prefix_length=0, min_length=0)) for j in range(4)]
    got = check_world(gpu, segs, reqs)
    assert got == [[("abcd", seq(dfs), sum(dfs))] for dfs in found]


def test_ordering(gpu):
    """equal scores broken by text; a text that is a prefix of another; 2-, 3- and 4-byte UTF-8 against ASCII in byte
    order; size cutting between two tied options; more groups than size, fewer, none"""
    texts = ["a", "ab", "abc", "a😀", "z", "é", "éa", "東", "東a", "😀", "zz", "b"]
    s0 = [("t:" + t, 2) for t in texts] + [("t:top", 9), ("t:low", 1)]
    s1 = [("t:" + t, 1) for t in reversed(texts)] + [("t:low", 1)]
    reqs = [req("t", "", size) for size in (1, 2, 3, 7, 13, 14, 15, 300)] + [req("t", "a", 2), req("t", "é", 9), req("t", "q", 9)]
    reqs += [req("t", "ab", size, dict(max_edits=2, prefix_length=0, min_length=0)) for size in (1, 2, 3, 50)]
    got = check_world(gpu, [s0, s1], reqs)
    order = [t for t, _, _ in got[reqs.index(req("t", "", 300))]]
    assert order == ["top"] + sorted(texts, key=lambda t: t.encode()) + ["low"]
    assert [t for t, _, _ in got[reqs.index(req("t", "", 3))]] == ["top", "a", "ab"]   # the cut between tied options
    assert got[reqs.index(req("t", "q", 9))] == []


def test_both_constants_are_reached(gpu):
    """exactly 256 candidates in 256 distinct texts; 256 candidates in 86 texts (three segments of 86, the cap
    inside the third)"""
    wide = [[(f"w:{W.word(i)}", W.df_of(i)) for i in range(CAND + 40)]]
    per = (CAND + 2) // 3
    assert per == 86
    three = [[(f"w:{W.word(i)}", 1 + (i + s) % 3) for i in range(per)] for s in range(3)]
    got = check_world(gpu, wide, [req("w", "", CAND), req("w", "", 300), req("w", "", 52)])
    assert [len(g) for g in got] == [CAND, CAND, 52]
    got = check_world(gpu, three, [req("w", "", 300), req("w", "", 86), req("w", "", 52), req("w", "", 51),
                                   req("w", "a", 256, dict(max_edits=2, prefix_length=1, min_length=0, max_expansions=300))])
    assert len(got[0]) == per and sum(d for _, _, d in got[0]) == sum(1 + (i + s) % 3 for s in range(3) for i in range(per)) \
        - sum(1 + (i + 2) % 3 for i in (per - 2, per - 1))                     # the third segment's last two are cut


def test_other_request_shapes(gpu):
    """an empty term scans the whole field; a field that is a prefix of a sibling's name; size 0 inside a batch; no
    requests; the size query"""
    segs = [[("bod:x", 3), ("body:y", 4), ("body:yy", 1), ("body2:z", 5), ("body:", 2)], [("body:y", 1), ("bod:w", 1)]]
    reqs = [req("body", "", 5), req("bod", "", 5), req("body", "y", 0), req("body2", "", 5), req("body", "y", 1), req("", "", 5)]
    with open_world(gpu, segs) as ix:
        got = check_index(ix, W.World(segs), reqs)
        assert got[0] == [("y", f32bits(5.0), 5), ("yy", f32bits(1.0), 1)] and got[2] == [] and ix.suggest([]) == []
        assert [t for t, _, _ in got[1]] == ["x", "w"]
        keep = []
        arr = (N.SuggestReq * len(reqs))(*[W.c_req(r, keep) for r in reqs])
        offs = np.zeros(len(reqs) + 2, np.uint32)
        N.check(ix._lib.slg_suggest_batch(ix._h, arr, len(reqs), offs.ctypes.data, 0, None, None, None, 0, None))
        assert offs.tolist() == [0, 2, 4, 4, 5, 6, 6, sum(len(t.encode()) for g in got for t, _, _ in g)]


def random_world(seed=4321):
    rng = random.Random(seed)
    vocab = sorted({"".join(rng.choice("abcé") for _ in range(rng.randrange(1, 9))) for _ in range(2600)})
    segs = []
    for _ in range(3):
        keys = [("w:" + x, rng.choice((0, 1, 1, 2, 3, 7, 50, 1000))) for x in rng.sample(vocab, 800)]
        keys += [("x:" + x, rng.randrange(0, 4)) for x in rng.sample(vocab, 40)] + [("w:", 5)]
        rng.shuffle(keys)
        segs.append(keys)
    return segs, vocab


def random_requests(vocab, n=300, seed=77):
    rng = random.Random(seed)
    reqs = []
    for _ in range(n):
        f = rng.choice(("w", "w", "w", "x"))
        wd = rng.choice(vocab)
        size = rng.choice((0, 1, 5, 5, 13, 52, 300))
        if rng.random() < 0.5:
            reqs.append(req(f, wd[:rng.randrange(0, 4)], size))
            continue
        if rng.random() < 0.3:                      # a typo of a word
            i = rng.randrange(len(wd))
            wd = wd[:i] + rng.choice("abcé") + wd[i + rng.randrange(2):]
        reqs.append(req(f, wd, min(size, CAND), dict(max_edits=rng.choice((0, 1, 2, 3)), prefix_length=rng.choice((0, 1, 2, 9)),
                                                   max_expansions=rng.choice((0, 1, 5, 50, 300)), min_length=rng.choice((0, 3)))))
    return reqs


def test_randomised_mixed_batch(gpu):
    segs, vocab = random_world()
    assert 2000 <= sum(len(s) for s in segs) <= 3000
    reqs = random_requests(vocab)
    got = check_world(gpu, segs, reqs)
    assert sum(len(g) for g in got) > 1000 and sum(1 for g in got if not g) > 10
    # the C++ restatement of the reference's loop (what tools/suggest_time.py times the device against) agrees too
    hs = [W.HostSegment(s) for s in segs]
    assert W.reference_loop(reqs, hs, 4) == got


def test_index_states(gpu):
    """tombstones change no answer; a new segment refuses until it has its dictionary, then counts; a removed one is gone"""
    s0 = [("t:rust", 4), ("t:rusk", 2), ("t:ruby", 1)]
    s1 = [("t:rust", 1), ("t:rune", 3)]
    s2 = [("t:rust", 2), ("t:rue", 6)]
    reqs = [req("t", "ru", 5), req("t", "rust", 5, dict(min_length=0)), req("t", "", 1)]
    with open_world(gpu, [s0, s1]) as ix:
        before = check_index(ix, W.World([s0, s1]), reqs)
        ix.update_deleted(0, np.array([0xFF], np.uint8), 1.0)                  # every doc of segment 0 deleted
        assert [R.bits(o) for o in ix.suggest(reqs)] == before
        ix.add_segment(W.df_segment(s2))
        with pytest.raises(N.SlgError) as e:
            ix.suggest(reqs)
        assert e.value.code == N.ERR_INVALID and "segment 2 has no term dictionary" in str(e.value)
        ix.set_terms(2, [k for k, _ in s2])
        after = check_index(ix, W.World([s0, s1, s2]), reqs)
        assert after[0][0] == ("rust", f32bits(7.0), 7) and after != before
        ix.remove_segment(0)
        check_index(ix, W.World([s1, s2]), reqs)


def test_the_expansion_is_unchanged(gpu):
    """one of the expansion's own worlds through slg_expand_batch before and after a suggest() on the same index"""
    from tests import expand_util as U
    from tests import expand_worlds as EW
    seg_keys, reqs = EW.segments_world(), EW.segments_requests()
    world = U.World(seg_keys)
    with gpu.GpuIndex([EW.dict_segment(k) for k in seg_keys]) as ix:
        ix.set_terms_from_segments()
        runs = [ix.expand(reqs)]
        got = ix.suggest([req("body", "r", 300), req("body", "rust", 5, {})])
        assert len(got[0]) == 105 and got[1][0][0] == "rust" and got[1][0][2] == 2
        runs.append(ix.expand(reqs))
    for run in runs:
        for r, (ids, dist) in zip(reqs, run):
            want_ids, want_dist = world.want(r)
            assert ids.tolist() == want_ids.tolist() and dist.tolist() == want_dist.tolist(), r
