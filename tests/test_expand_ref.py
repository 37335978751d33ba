"""tests/expand_ref.py pinned to the reference's own tests (tests/smoke.rs:159-325, api/reader.rs:4283 and :4349,
restated at the expansion level), its bounded distance against a plain full-matrix Levenshtein, and the library's
host side (csrc/slg_expand_merge.cpp and the scan's predicates compiled for the host, through the test C ABI of
lib/libslg_plan.so) against it.  No GPU."""
import ctypes as C
import itertools
import random

import numpy as np
import pytest

from tests import expand_ref as R
from tests import expand_util as U

NO = R.NO_TERM


def keys_of(*words, field="body"):
    return R.sorted_keys(f"{field}:{w}" for w in words)


def fz(term, **kw):
    o = dict(max_edits=1, prefix_length=1, max_expansions=20, min_length=3)
    o.update(kw)
    return R.expand_term_fuzzy(o.pop("segs"), "body", term, **o)


# ---- tests/smoke.rs:159-325 ----------------------------------------------------------------------------------
def test_fuzzy_matches_typos():                                  # smoke.rs:159-181 ("Rust is fast")
    segs = [keys_of("rust", "is", "fast")]
    assert fz("rusk", segs=segs) == [("body:rusk", 0), ("body:rust", 1)]


def test_fuzzy_respects_min_length():                            # smoke.rs:213-228
    assert fz("ru", segs=[keys_of("rust")]) == [("body:ru", 0)]


def test_fuzzy_respects_max_expansions():                        # smoke.rs:231-262
    segs = [keys_of("rush", "rust")]
    assert fz("rusk", segs=segs, max_expansions=1) == [("body:rusk", 0), ("body:rush", 1)]
    assert fz("rusk", segs=segs, max_expansions=2) == [("body:rusk", 0), ("body:rush", 1), ("body:rust", 1)]


def test_fuzzy_respects_prefix_length():                         # smoke.rs:265-293
    segs = [keys_of("dusk")]
    assert fz("rusk", segs=segs, prefix_length=0) == [("body:rusk", 0), ("body:dusk", 1)]
    assert fz("rusk", segs=segs, prefix_length=1) == [("body:rusk", 0)]


def test_fuzzy_allows_two_edits():                               # smoke.rs:296-324
    segs = [keys_of("rust")]
    assert fz("rsut", segs=segs, max_edits=1) == [("body:rsut", 0)]
    assert fz("rsut", segs=segs, max_edits=2) == [("body:rsut", 0), ("body:rust", 2)]


def test_prefix_expansion_respects_max_expansions():             # api/reader.rs:4283-4346
    keys = R.expand_prefix([keys_of("ruby", "rumor", "rust")], "body", "ru", 2)
    assert set(keys) == {"body:ruby", "body:rumor"}


def test_wildcard_expansion_handles_star_and_question():         # api/reader.rs:4349-4440
    segs = [keys_of("rust", "rest", "roast", "roost")]
    assert set(R.expand_wildcard(segs, "body", "r*st", 50)) == {"body:rust", "body:rest", "body:roast", "body:roost"}
    assert set(R.expand_wildcard(segs, "body", "ro?st", 50)) == {"body:roast", "body:roost"}


# ---- the bounded distance ------------------------------------------------------------------------------------
ALPHABET_WORDS = ["".join(w) for n in range(6) for w in itertools.product("abé", repeat=n)]


def test_bounded_levenshtein_is_the_full_matrix_distance_within_the_bound():
    """all pairs of strings of length <= 5 over {a, b, é}, max_edits 0 .. 2"""
    for a in ALPHABET_WORDS:
        for b in ALPHABET_WORDS:
            if abs(len(a) - len(b)) > 2:
                assert R.bounded_levenshtein(a, b, 2) is None
                continue
            full = R.full_levenshtein(a, b)
            for me in (0, 1, 2):
                assert R.bounded_levenshtein(a, b, me) == (full if full <= me else None), (a, b, me)


def test_the_scans_banded_distance_is_the_bounded_distance():
    """the kernel's five-cell band (slg_expand.hpp, compiled for the host) on the same pairs"""
    L = U.host_lib()
    for a in ALPHABET_WORDS:
        cps = np.array([ord(c) for c in a] + [0], dtype=np.uint32)
        for b in ALPHABET_WORDS:
            if abs(len(a) - len(b)) > 2:
                continue
            raw = b.encode("utf-8")
            for me in (1, 2):
                if abs(len(a) - len(b)) > me:
                    continue
                got = L.slgx_banded_distance(cps.ctypes.data, len(a), raw, len(raw), me)
                want = R.bounded_levenshtein(a, b, me)
                assert (None if got > me else got) == want, (a, b, me, got)


def test_the_scans_glob_match_is_the_translated_regex():
    """the two-pointer match against re.fullmatch on build_wildcard_regex, '\\n' and multi-byte chars included"""
    L = U.host_lib()
    rng = random.Random(5)
    texts = ["".join(rng.choice("ab\né😀") for _ in range(rng.randrange(0, 7))) for _ in range(300)]
    texts += ["aXbXbc", "abc", "", "a\nb", "ax\n\nb"]
    pats = ["".join(rng.choice("ab*?\né") for _ in range(rng.randrange(0, 6))) for _ in range(300)]
    pats += ["*", "a*b*c", "a*\nb", "?", "**", "*\n*"]
    for p in pats:
        rx = R.build_wildcard_regex(p)
        cps = np.array([ord(c) for c in p] + [0], dtype=np.uint32)
        for t in texts:
            raw = t.encode("utf-8")
            assert bool(L.slgx_glob_match(cps.ctypes.data, len(p), raw, len(raw))) == (rx.fullmatch(t) is not None), (p, t)


# ---- the host side: dictionaries, requests, the merge --------------------------------------------------------
def test_dictionary_is_sorted_by_bytes_with_its_map_and_char_counts():
    keys = ["body:zeta", "body:é", "body:alpha", "title:x", "body:" + "é" * 300, "body:z😀"]
    d = U.HostDict(keys)
    assert d.h
    order = sorted(range(len(keys)), key=lambda i: keys[i].encode("utf-8"))
    assert d.map.tolist() == order
    assert d.nchars.tolist() == [min(len(keys[i]), 255) for i in order]


@pytest.mark.parametrize("keys,word", [(["body:a", "body:a"], b"equal"), (["bodya"], b"':'"),
                                       ([b"body:\xff"], b"UTF-8"), ([b"body:\xed\xa0\x80"], b"UTF-8"),
                                       ([b"body:\xc0\xaf"], b"UTF-8")])
def test_dictionary_errors(keys, word):
    d = U.HostDict(keys)
    assert not d.h and d.code.value == -1 and word in d.err.value


def test_prefix_range_does_not_leak_into_sibling_fields():
    keys = R.sorted_keys(["bod:x", "body:", "body:a", "body:b", "body2:a", "bodz:a"])
    d = U.HostDict(keys)
    lo, hi = C.c_uint32(), C.c_uint32()
    for pre, want in [(b"body:", ["body:", "body:a", "body:b"]), (b"body:b", ["body:b"]), (b"body:c", []),
                      (b"", keys), (b"bodz:", ["bodz:a"]), (b"c", [])]:
        U.host_lib().slgx_prefix_range(d.h, pre, len(pre), C.addressof(lo), C.addressof(hi))
        assert keys[lo.value:hi.value] == want, pre


MERGE_WORLDS = {
    # duplicates across segments, holes, term ids in another order than the bytes in segment 1
    "overlap": [["body:rush", "body:rust", "body:ruse"], ["body:rust", "body:bust", "body:rusk", "body:ruts"],
                ["title:rust", "body:dust"]],
    # a key past segment 0's cap enters through segment 1
    "cap": [["body:ra", "body:rb", "body:rc", "body:rd"], ["body:rb", "body:rd", "body:re"], ["body:ra", "body:rd", "body:rz"]],
}
MERGE_REQS = [
    U.fuzzy("body", "rust", max_edits=1), U.fuzzy("body", "rust", max_edits=2, prefix_length=0),
    U.fuzzy("body", "rust", max_expansions=1), U.fuzzy("body", "rust", max_expansions=2),
    U.fuzzy("body", "rust", max_expansions=3),                     # the global cap, reached inside segment 1
    U.fuzzy("body", "rusx"),                                       # an exact key no segment holds
    U.fuzzy("body", "ru"), U.fuzzy("body", "rust", max_edits=0), U.fuzzy("body", "rust", max_expansions=0),
    U.prefix("body", "r", 1), U.prefix("body", "r", 2), U.prefix("body", "r", 3), U.prefix("body", "", 50),
    U.prefix("body", "r", 0), U.prefix("title", "r", 5), U.prefix("nope", "", 5),
    U.wildcard("body", "r*", 1), U.wildcard("body", "r?", 2), U.wildcard("body", "*st", 2), U.wildcard("body", "ru??", 50),
]


@pytest.mark.parametrize("world", sorted(MERGE_WORLDS))
@pytest.mark.parametrize("ri", range(len(MERGE_REQS)))
def test_host_merge_over_hand_made_device_rows(world, ri):
    """global vs per-segment cap, duplicates, NO_TERM holes, exact keys nobody holds: exact equality"""
    w = U.World(MERGE_WORLDS[world])
    req = MERGE_REQS[ri]
    dicts = [U.HostDict(k) for k in w.seg_keys]
    got_ids, got_dist = U.host_merge(req, dicts, U.device_rows(w.sorted, req))
    want_ids, want_dist = w.want(req)
    assert got_ids.tolist() == want_ids.tolist() and got_dist.tolist() == want_dist.tolist()


def test_a_key_past_segment_0s_cap_enters_through_segment_1():
    w = U.World(MERGE_WORLDS["cap"])
    keyed = R.expand(w.sorted, U.prefix("body", "r", 2))
    assert [k for k, _ in keyed] == ["body:ra", "body:rb", "body:rd", "body:re", "body:rz"]
    req = U.prefix("body", "r", 2)
    ids, _ = U.host_merge(req, [U.HostDict(k) for k in w.seg_keys], U.device_rows(w.sorted, req))
    assert ids.tolist() == [[0, NO, 0], [1, 0, NO], [3, 1, 1], [NO, 2, NO], [NO, NO, 2]]


def test_the_cpp_restatement_of_the_reference_loop():
    """slgx_reference_expand (what tools/expand_time.py times the scan against) answers as tests/expand_ref.py"""
    rng = random.Random(11)
    words = sorted({"".join(rng.choice("abcé") for _ in range(rng.randrange(1, 7))) for _ in range(400)})
    segs = [["body:" + x for x in rng.sample(words, 150)] + ["body:"] for _ in range(3)]
    w = U.World(segs)
    dicts = [U.HostDict(k) for k in w.seg_keys]
    reqs = [U.fuzzy("body", rng.choice(words), max_edits=rng.choice((1, 2, 3)), prefix_length=rng.choice((0, 1, 2)),
                    max_expansions=rng.choice((1, 3, 50)), min_length=rng.choice((0, 3))) for _ in range(40)]
    reqs += [U.prefix("body", rng.choice(words)[:2], rng.choice((1, 4, 50))) for _ in range(20)]
    reqs += [U.wildcard("body", rng.choice(["a*", "*b", "a?c*", "*", "?é*"]), rng.choice((2, 50))) for _ in range(20)]
    for n_threads in (1, 4):
        got = U.reference_loop(reqs, dicts, n_threads)
        for r, (ids, dist) in zip(reqs, got):
            want_ids, want_dist = w.want(r)
            assert ids.tolist() == want_ids.tolist() and dist.tolist() == want_dist.tolist(), r


@pytest.mark.parametrize("change,code,word", [
    (dict(struct_size=8), -1, b"struct_size"), (dict(kind=7), -1, b"kind"),
    (dict(term=b"\xff\xfe"), -1, b"UTF-8"), (dict(field=b"\xc3"), -1, b"UTF-8"),
    (dict(term="a" * 129), -4, b"SLG_MAX_EXPAND_CHARS"), (dict(max_expansions=1025), -4, b"SLG_MAX_EXPANSIONS"),
])
def test_request_errors(change, code, word):
    from searchlite_amd import _native as N
    keep = []
    r = U.c_req(U.fuzzy("body", "rust"), keep)
    for k, v in change.items():
        if k in ("term", "field"):
            v = v.encode("utf-8") if isinstance(v, str) else v
            keep.append(v)
            setattr(r, k + "_len", len(v))
        setattr(r, k, v)
    out = [C.c_uint32() for _ in range(3)]
    buf, err = C.create_string_buffer(64), C.create_string_buffer(256)
    rc = U.host_lib().slgx_check_request(C.addressof(r), C.addressof(out[0]), C.addressof(out[1]), buf, 64,
                                         C.addressof(out[2]), err, 256)
    assert rc == code and word in err.value


def test_a_term_of_exactly_the_char_limit_is_taken_and_multibyte_chars_count_once():
    keep = []
    r = U.c_req(U.fuzzy("body", "é" * 128, prefix_length=2), keep)
    out = [C.c_uint32() for _ in range(3)]
    buf, err = C.create_string_buffer(64), C.create_string_buffer(256)
    rc = U.host_lib().slgx_check_request(C.addressof(r), C.addressof(out[0]), C.addressof(out[1]), buf, 64,
                                         C.addressof(out[2]), err, 256)
    assert rc == 0 and out[0].value == 1 and buf.raw[:out[2].value] == "body:éé".encode("utf-8")
