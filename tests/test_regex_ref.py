"""tests/regex_ref.py pinned to the reference's own regex test (api/reader.rs:4438) and to every quirk of its
literal-prefix rule, and the library's regex compiler (csrc/slg_regex.cpp) with the host build of the device's DFA
walk (csrc/slg_expand_regex.hpp) against it, through the test C ABI of lib/libslg_plan.so: exhaustively over short
strings for a hand-written corpus and 300 seeded random patterns, the minimised sizes, the limits at their edges,
and the host merge over hand-made device rows.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from searchlite_amd import _native as N
from tests import expand_ref as R
from tests import expand_util as U
from tests import regex_ref as RR
from tests import regex_util as X


def keys_of(*words, field="body"):
    return R.sorted_keys(f"{field}:{w}" for w in words)


# ---- the reference's own test and the literal-prefix rule ----------------------------------------------------------
def test_regex_expansion_respects_max_expansions():              # api/reader.rs:4438
    segs = [keys_of("rope", "ruby", "rust")]
    assert RR.expand_regex(segs, "body", "r(ust|uby)", 1) == ["body:ruby"]
    assert RR.expand_regex(segs, "body", "r(ust|uby)", 2) == ["body:ruby", "body:rust"]
    assert RR.expand_regex(segs, "body", "r(ust|uby)", 0) == []


PREFIXES = [   # pattern -> regex_literal_prefix
    ("rust", "rust"), ("r(ust|uby)", "r"), ("^rust", "rust"), ("^^ru", "ru"), ("r^u", "r^u"), ("ab|cd", "ab"), ("rust?", "rust"),
    ("ab*", "ab"), (r"\n.*", "n"), (r"a\.b.*", "a.b"), (r"a\\b+", "a\\b"), (r"ab\d+", "ab"), (r"a\Dx", "a"), (r"a\wb", "a"),
    (r"\Wa", ""), (r"a\s", "a"), (r"a\Sb", "a"), (r"a\b", "a"), (r"a\Bc", "a"), (r"a\pLb", "a"), (r"a\PLb", "a"),
    (r"a\tb", "atb"), (r"\Aab", "Aab"), (r"ab\z", "abz"), ("a.b", "a"), ("a+", "a"), ("(a)", ""), ("a)b", "a"), ("a[bc]", "a"),
    ("a]b", "a"), ("a{2}", "a"), ("a}b", "a"), ("a$", "a"), ("é€😀.*", "é€😀"), (r"\é.", "é"), ("", ""), ("\\", ""), ("ab\\", "ab"),
    (".*ing", ""), ("(?:un)?do.*", ""),
]


@pytest.mark.parametrize("pattern,want", PREFIXES)
def test_literal_prefix_rule(pattern, want):
    assert RR.regex_literal_prefix(pattern) == want
    assert X.literal_prefix(pattern) == want                     # the library's restatement of the same rule


def test_literal_prefix_consequences():
    """the reference's answers, quirks included: the range comes from the pattern's text, the match from its meaning"""
    segs = [keys_of("ab", "abx", "cd", "rus", "rust", "rusty", "a", "abb", "n", "nx", "\n", "\nx")]
    assert RR.expand_regex(segs, "body", "ab|cd", 50) == ["body:ab"]                    # never "cd"
    assert RR.expand_regex(segs, "body", "rust?", 50) == ["body:rust"]                  # never "rus"
    assert RR.expand_regex(segs, "body", "ab*", 50) == ["body:ab", "body:abb"]          # never "a"
    assert RR.expand_regex(segs, "body", r"\n.*", 50) == []                             # the range of the letter n
    assert RR.expand_regex(segs, "body", "\n.*", 50) == ["body:\n", "body:\nx"]         # (a raw U+000A is a literal)
    assert RR.expand_regex(segs, "body", "(ab|cd)", 50) == ["body:ab", "body:cd"]       # (an empty prefix scans the field)
    # the library's range key says the same
    for pattern, want in (("ab|cd", b"body:ab"), ("rust?", b"body:rust"), (r"\n.*", b"body:n"), ("(ab|cd)", b"body:"),
                          (r"a\.b", b"body:a.b"), ("^é+", "body:é".encode())):
        assert check(X.regex("body", pattern))[3] == want


def check(req):
    """slgx_check_request -> (code, message, scan, range key)"""
    keep = []
    cr = U.c_req(req, keep)
    scan, me, rl = C.c_uint32(9), C.c_uint32(9), C.c_uint32(0)
    key, err = C.create_string_buffer(1024), C.create_string_buffer(512)
    rc = U.host_lib().slgx_check_request(C.addressof(cr), C.addressof(scan), C.addressof(me), key, 1024, C.addressof(rl), err, 512)
    return rc, err.value, scan.value, key.raw[:rl.value]


def test_expansion_loop_of_the_restatement():
    """segments in order, the per-segment cap over new keys only, the bare key, whole-term match"""
    s0 = keys_of("r1", "r2", "r3", "r4", "x") + ["body:"]
    s1 = keys_of("r0", "r1", "r2", "r3", "r5")
    assert RR.expand_regex([R.sorted_keys(s0), s1], "body", "r[0-9]", 2) == ["body:r1", "body:r2", "body:r0", "body:r3"]
    assert RR.expand_regex([R.sorted_keys(s0)], "body", ".*", 50) == ["body:r1", "body:r2", "body:r3", "body:r4", "body:x"]
    assert RR.expand_regex([s1], "body", "r", 50) == [] and RR.expand_regex([s1], "body", "5", 50) == []
    with pytest.raises(RR.Refused):
        RR.expand_regex([s1], "body", "(r", 0)                    # an invalid pattern is an error whatever the cap


# ---- the DFA against the restatement ------------------------------------------------------------------------
SHORT = X.strings(X.ALPHABET, 5)


def compare(pattern, terms):
    d = X.Dfa(pattern)
    assert d.code == N.OK, (pattern, d.msg)
    assert RR.classify(pattern) == RR.SUPPORTED, pattern
    rx = RR.compile_pattern(pattern)
    for t in terms:
        assert d.match(t) == (rx.fullmatch(t) is not None), (pattern, t)
    return d


def test_the_corpus_covers_what_it_should():
    assert len(X.CORPUS) >= 60 and len(set(X.CORPUS)) == len(X.CORPUS)
    assert {"a^b", "a$|b", "(^a)*b"} <= set(X.CORPUS)
    assert len(SHORT) == sum(4 ** n for n in range(6))


def test_hand_written_corpus_exhaustively():
    for pattern in X.CORPUS:
        compare(pattern, SHORT)
    # spot checks by hand, on top of the restatement
    assert [t for t in ("", "a", "b", "ab") if X.Dfa("a^b").match(t)] == []
    assert [t for t in ("", "a", "b", "ab") if X.Dfa("a$|b").match(t)] == ["a", "b"]
    assert [t for t in ("", "b", "ab", "aab") if X.Dfa("(^a)*b").match(t)] == ["b", "ab"]
    assert X.Dfa(".").match("😀") and not X.Dfa(".").match("\n") and X.Dfa("[^a]").match("\n") and X.Dfa("$^").match("")


def test_random_patterns_exhaustively():
    patterns = X.random_patterns(300, 2024)
    assert len(patterns) == 300
    refused = [(p, X.Dfa(p).msg) for p in patterns if X.Dfa(p).code != N.OK]
    assert refused == []                                         # none skipped: every one compiles within the limits
    wide = X.strings(X.RANDOM_ALPHABET, 3)                       # (the 3- and 4-byte literals of the patterns)
    for p in patterns:
        compare(p, SHORT)
        compare(p, wide)
    assert any("😀" in p for p in patterns) and any("€" in p for p in patterns) and any("é" in p for p in patterns)


def test_long_terms_and_every_utf8_width():
    d = compare("a{254}", ["a" * 253, "a" * 254, "a" * 255, "a" * 253 + "b"])
    assert d.n_states == 256 and d.match("a" * 254)
    compare(".*z", ["z" * 300, "é" * 150 + "z", "z" * 299 + "\n", "😀" * 70 + "z"])
    compare("[^€]*", ["€", "₭", "₫", "₭", "₫", "aࠀ￿", "\U00010000", "\U0010ffff", "퟿"])
    compare("[ࠀ-\U00010000]+", ["߿", "ࠀ", "￿", "\U00010000", "\U00010001", "퟿"])
    compare("[é-߿]", ["è", "é", "ê", "߿", "ࠀ", "\x7f", "\x80"])


# ---- minimisation ---------------------------------------------------------------------------------------------
def test_minimised_sizes():
    for n in (1, 2, 5, 100):
        d = X.Dfa("a{%d}" % n)
        assert (d.n_states, d.n_classes) == (n + 2, 2)
    assert X.Dfa("(a|b)*abb").n_states == 5
    dot = X.Dfa(".*")
    # dead, start, and what is still owed after each kind of lead byte: one / two / three continuation bytes, and
    # the narrowed second bytes behind E0, ED, F0 and F4
    assert dot.n_states == 9 and dot.accepting() == [1]
    assert (X.Dfa(".*.*").n_states, X.Dfa("(.*)*").n_states, X.Dfa(".*|a").n_states) == (9, 9, 9)
    a, aaa = X.Dfa("a"), X.Dfa("a|a|a")
    assert (a.n_states, a.n_classes) == (aaa.n_states, aaa.n_classes) == (3, 2)
    assert a.table[:6].tolist() == aaa.table[:6].tolist() and a.class_of.tolist() == aaa.class_of.tolist()
    assert a.accept.tolist() == aaa.accept.tolist()
    empty = X.Dfa("a^b")                                         # the empty language: dead and a start that leads to it
    assert (empty.n_states, empty.n_classes, empty.accepting()) == (2, 1, [])
    for d in (a, dot, X.Dfa("(a|b)*abb")):                       # state 0 is dead, state 1 the start
        assert not d.table[:d.n_classes].any() and 0 not in d.accepting()


# ---- the limits at their edges ------------------------------------------------------------------------------------
def distinct_literals(n):
    """a pattern of n distinct one-byte literals (metacharacters escaped)"""
    chars = [chr(c) for c in range(128)][:n]
    return "".join("\\" + c if c in r"\.*+?()[]{}|^$" else c for c in chars)


def test_limits_at_their_edges():
    states, table = N.MAX_REGEX_STATES, N.MAX_REGEX_TABLE
    d = X.Dfa("a{%d}" % (states - 2))
    assert d.code == N.OK and d.n_states == states and d.accepting() == [states - 1]
    d = X.Dfa("a{%d}" % (states - 1))
    assert d.code == N.ERR_UNSUPPORTED and "SLG_MAX_REGEX_STATES" in d.msg
    # n distinct literals: n + 2 states x n + 1 classes; the largest n whose table fits, and one more
    n = max(k for k in range(1, 128) if (k + 2) * (k + 1) <= table)
    assert n == 126 and (n + 2) * (n + 1) == 16256 and (n + 3) * (n + 2) == 16512
    d = X.Dfa(distinct_literals(n))
    assert d.code == N.OK and (d.n_states, d.n_classes) == (n + 2, n + 1)
    assert d.match(bytes(range(n))) and not d.match(bytes(range(n - 1))) and not d.match(bytes(range(n + 1)))
    d = X.Dfa(distinct_literals(n + 1))
    assert d.code == N.ERR_UNSUPPORTED and "SLG_MAX_REGEX_TABLE" in d.msg
    # the table at its very limit inside a request: 63 distinct literals, then the last of them 191 times more
    p = distinct_literals(63) + "{%d}" % (states - 64)
    d = X.Dfa(p)
    assert d.code == N.OK and (d.n_states, d.n_classes) == (states, 64) and d.n_states * d.n_classes == table
    # the pattern's chars: SLG_MAX_EXPAND_CHARS is taken, one more is refused
    assert check(X.regex("body", "a" * N.MAX_EXPAND_CHARS))[0] == N.OK
    rc, msg, _, _ = check(X.regex("body", "a" * (N.MAX_EXPAND_CHARS + 1)))
    assert rc == N.ERR_UNSUPPORTED and b"SLG_MAX_EXPAND_CHARS" in msg
    assert check(X.regex("body", p))[0] == N.OK and len(p) <= N.MAX_EXPAND_CHARS


# ---- the host merge over hand-made device rows ----------------------------------------------------------------------
def merged(world, dicts, req):
    rows = X.device_rows(world.sorted, req)
    return U.host_merge(req, dicts, rows), rows


def test_host_merge_of_regex_rows():
    rs = [f"body:r{i:02d}" for i in range(30)]
    seg_keys = [rs + ["body:x", "body:"], list(reversed(rs[5:])) + ["body:q", "body:r99"], ["title:r00"] + rs[:3]]
    world = X.World(seg_keys)
    dicts = [U.HostDict(k) for k in seg_keys]
    for req in (X.regex("body", "r[0-9]+", 4), X.regex("body", "r[0-9]+", 1), X.regex("body", "r.*", 1024),
                X.regex("body", ".*", 3), X.regex("body", "r0[0-9]|r99", 50), X.regex("body", "r.*", 0),
                X.regex("title", "(r|x)00", 5), X.regex("nope", ".*", 5)):
        (ids, dist), rows = merged(world, dicts, req)
        want_ids, want_dist = world.want(req)
        assert ids.tolist() == want_ids.tolist() and dist.tolist() == want_dist.tolist(), req
    # duplicates, the per-segment cap, and the key that enters through segment 1: cap 4 takes r00 .. r03 of segment
    # 0; segment 1 starts at r05, so r05 .. r08 are new there although segment 0 holds them past its cap
    (ids, _), rows = merged(world, dicts, X.regex("body", "r[0-9]+", 4))
    keys = [world.seg_keys[0][i] if i != R.NO_TERM else None for i in ids[:, 0].tolist()]
    assert keys[:8] == ["body:r00", "body:r01", "body:r02", "body:r03", "body:r05", "body:r06", "body:r07", "body:r08"]
    assert [len(p) for p, _ in rows] == [4, 8, 3]                # R = (seg + 1) x max_expansions, or the range's passing keys
    assert len(keys) == 8                                        # segment 2's r00 .. r02 are all duplicates
    L = U.host_lib()
    keep = []
    cr = U.c_req(X.regex("body", "r.*", 7), keep)
    assert [L.slgx_rows_needed(C.addressof(cr), s) for s in range(3)] == [7, 14, 21]


def test_reference_loop_takes_the_kind():
    """slgx_reference_expand with the host DFA walk as its matcher (the timing tool's yardstick) agrees with the
    restatement; correctness is judged by the restatement, never by it"""
    seg_keys = [[f"w:{a}{b}{c}" for a in "abé" for b in "ab\n" for c in "abc"], ["w:abc", "w:zzz", "w:a"]]
    world = X.World(seg_keys)
    reqs = [X.regex("w", "a.*", 5), X.regex("w", ".b[ac]", 50), X.regex("w", "[^a]+", 2), X.regex("w", "z{3}|a", 9),
            U.wildcard("w", "a?c", 50)]
    for req, (ids, dist) in zip(reqs, U.reference_loop(reqs, [U.HostDict(k) for k in seg_keys], 2)):
        assert ids.tolist() == world.want(req)[0].tolist() and not dist.any(), req


# ---- the compiler and the walk under the sanitizers -----------------------------------------------------------------
def test_compiler_and_walk_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/regex_sanitize.cpp, a stand-alone program: every pattern of the three corpora and the random ones
    through the compiler, and the compiled ones through the host DFA walk, built with -fsanitize=address,undefined"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "searchlite_amd", "csrc")
    exe = str(tmp_path / "regex_sanitize")
    # (the sanitizers' runtimes linked into the program itself: it needs nothing from the environment it runs in)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "regex_sanitize.cpp"),
                           os.path.join(csrc, "slg_regex.cpp")])
    patterns = list(X.CORPUS) + [p for p, _ in X.INVALID] + [p for p, _ in X.UNSUPPORTED] + X.random_patterns(300, 2024)
    patterns += [distinct_literals(126), distinct_literals(127), "a{254}", "a{255}", "a" * 128]
    listing = tmp_path / "patterns.hex"
    listing.write_text("".join(p.encode("utf-8").hex() + "\n" for p in patterns))
    terms = tmp_path / "terms.hex"
    terms.write_text("".join(t.encode("utf-8").hex() + "\n" for t in X.strings(X.ALPHABET, 3) + ["a" * 300, "😀€é" * 20]))
    out = subprocess.run([exe, str(listing), str(terms)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    counts = dict(kv.split("=") for kv in out.stdout.split())
    n_ok = len(X.CORPUS) + 300 + 3
    assert int(counts["patterns"]) == len(patterns) and int(counts["compiled"]) == n_ok
    assert int(counts["invalid"]) == len(X.INVALID) and int(counts["unsupported"]) == len(X.UNSUPPORTED) + 2
