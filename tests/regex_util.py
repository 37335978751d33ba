"""What the regex tests share: the library's regex compiler and the host build of the device's DFA walk through the
test C ABI (lib/libslg_plan.so, csrc/slg_expand_capi.cpp: slgx_regex_*), the pattern corpora (supported, invalid,
unsupported: one list each, so every test and the stand-alone sanitizer program read the same patterns), the
seeded generator of random supported patterns, and hand-made device rows for the host merge."""
from __future__ import annotations

import ctypes as C
import itertools
import random

import numpy as np

from searchlite_amd import _native as N
from tests import expand_util as U
from tests import regex_ref as RR

REGEX = N.EXPAND_REGEX
regex = RR.regex

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = U.host_lib()
        vp, u32 = C.c_void_p, C.c_uint32
        L.slgx_regex_compile.restype = C.c_int
        L.slgx_regex_compile.argtypes = [C.c_char_p, u32, vp, vp, vp, vp, u32, vp, C.c_char_p, u32]
        L.slgx_regex_match.restype = C.c_int
        L.slgx_regex_match.argtypes = [vp, vp, vp, u32, C.c_char_p, u32]
        L.slgx_regex_literal_prefix.restype = C.c_int
        L.slgx_regex_literal_prefix.argtypes = [C.c_char_p, u32, C.c_char_p, u32, vp]
        _lib = L
    return _lib


class Dfa:
    """slgx_regex_compile(pattern): .code / .msg, and on success the tables and .match(term)"""

    def __init__(self, pattern: str):
        raw = pattern.encode("utf-8")
        ns, nc = C.c_uint32(0), C.c_uint32(0)
        self.class_of = np.zeros(256, np.uint8)
        self.table = np.zeros(N.MAX_REGEX_TABLE, np.uint8)
        self.accept = np.zeros(32, np.uint8)
        err = C.create_string_buffer(512)
        self.code = lib().slgx_regex_compile(raw, len(raw), C.addressof(ns), C.addressof(nc), self.class_of.ctypes.data,
                                             self.table.ctypes.data, len(self.table), self.accept.ctypes.data, err, 512)
        self.msg = err.value.decode("utf-8", "replace")
        self.n_states, self.n_classes = ns.value, nc.value
        self._args = (self.class_of.ctypes.data, self.table.ctypes.data, self.accept.ctypes.data, self.n_classes)
        self._match = lib().slgx_regex_match

    def match(self, term) -> bool:
        raw = term.encode("utf-8") if isinstance(term, str) else term
        return bool(self._match(*self._args, raw, len(raw)))

    def accepting(self):
        return [s for s in range(self.n_states) if (self.accept[s >> 3] >> (s & 7)) & 1]


def literal_prefix(pattern: str) -> str:
    raw = pattern.encode("utf-8")
    out = C.create_string_buffer(len(raw) + 1)
    n = C.c_uint32(0)
    assert lib().slgx_regex_literal_prefix(raw, len(raw), out, len(raw) + 1, C.addressof(n)) == 0
    return out.raw[:n.value].decode("utf-8")


def strings(alphabet, up_to):
    return ["".join(t) for n in range(up_to + 1) for t in itertools.product(alphabet, repeat=n)]


ALPHABET = ("a", "b", "é", "\n")

# ---- the hand-written corpus: every supported construct, and anchors in the middle of a pattern -------------------
CORPUS = [
    "", "a", "ab", "é", "aé", "€", "😀", "a😀b", "\n", "a\nb", r"\n", r"a\nb", r"\t", r"\r", r"\.", r"\\", r"a\*b", r"\-", r"\]",
    r"\{a\}", "]", "}", "a]b}", ".", "..", "a.b", ".*", ".+", ".?", "a*", "a+", "a?", "a*b", "a+b+", "(a|b)*abb", "ab|ba", "a|",
    "|a", "a||b", "(|a)b", "(a|)", "()", "()a", "(a)", "(ab)*", "(a*)*", "(a|b|é)+", "(?:ab)+", "(?:a|b){2}", "(?P<x>a)b",
    "(?<x>a)(?P<y_1>b)", "a{0}", "a{1}", "a{2}", "a{2,}", "a{0,}", "a{1,3}", "a{0,2}b", "(ab){2,3}", "(a|b){3}", ".{2}",
    ".{1,2}b", "a*?", "a+?b", "a??", "a{2}?", "a{1,}?b", "(a|b)*?b", "[a]", "[ab]", "[a-b]", "[^a]", "[^ab]", "[^a-b]*",
    "[é]", "[a-é]", "[^é]+", "[\n]", "[^\n]", r"[\n]", r"[^\n]*", "[]]", "[]a]", "[^]]", "[^]a]*", "[-a]", "[a-]", "[-]", "[^-]",
    "[^-a]b", "[a-b-é]", r"[\]]", r"[\-a]", r"[\\]", r"[\^a]", "[a^]", "[^^]", "[.]", "[*+?]", "[(|)]", "[{}]", "[$]",
    "[ -~]*", "[a-b][^a-b]", "[€-😀]", "[^€]", "[😀]a", "^a", "a$", "^a$", "^", "$", "^$", "$^", r"\Aa\z", r"\A", r"\z",
    "a^b", "a$b", "a$|b", "^a|b$", "(^a)*b", "(a$)*", "(^)*a", "($)?", "a(^|b)", "(a|$)b", "(^|a)(b|$)", "a*$", "^.*$", "(^a|b)+",
    "(a$|b)+", r"a\z|b", r"(\Aa)+", "a(?:$|b)a?", ".*a.*", ".*é", ".*\n.*", "[^a]*a[^a]*", "(a|ab)(c|bcd)?", "(ab?)*",
    "((a|b)(a|b))*", "(a{2}|b{3})+", "(é|\n)*a", "a.{0,3}b", "(a.)*", "[ab]{2,4}", "(?:a|(?:b|(?:é)))*",
]

INVALID = [   # (pattern, a word of the message)
    ("(a", "unbalanced '('"), ("a)", "unbalanced ')'"), ("((a)", "unbalanced '('"), ("(a))", "unbalanced ')'"), ("(?:a", "unbalanced '('"),
    ("[a", "unclosed '['"), ("[", "unclosed '['"), ("[]", "unclosed '['"), ("[^]", "unclosed '['"), ("a[b-", "unclosed '['"),
    ("[z-a]", "reversed range"), ("[b-a]", "reversed range"), ("[é-a]", "reversed range"),
    ("*a", "nothing to repeat"), ("+", "nothing to repeat"), ("?a", "nothing to repeat"), ("{2}", "nothing to repeat"),
    ("(*a)", "nothing to repeat"), ("(?:+a)", "nothing to repeat"), ("a|*b", "nothing to repeat"), ("a|{2}", "nothing to repeat"),
    ("a{", "'{'"), ("a{x}", "'{'"), ("a{2", "'{'"), ("a{2,x}", "'{'"), ("a{2,3", "'{'"), ("a{}", "'{'"), ("a{,}", "'{'"), ("a{ 2}", "'{'"),
    ("a{3,2}", "n > m"), ("a{1,0}", "n > m"),
    ("\\", "trailing lone '\\'"), ("ab\\", "trailing lone '\\'"), ("[a\\", "trailing lone '\\'"),
    ("(?P<>a)", "group name"), ("(?<x", "group name"), ("(?<x>a)(?<x>b)", "duplicate group name"),
    ("(?<=a)b", "group name"), ("(?<!a)b", "group name"),   # (look-behind: the reference's engine has none)
]

UNSUPPORTED = [
    (r"\d", r"\d"), (r"\D", r"\D"), (r"\w+", r"\w"), (r"\W", r"\W"), (r"a\s", r"\s"), (r"\S", r"\S"), (r"\pL", r"\p"),
    (r"\P{L}", r"\P"), (r"\bab", r"\b"), (r"a\B", r"\B"), (r"[\d]", r"\d"), (r"[a\w]", r"\w"),
    (r"\x41", r"\x"), ("\\u0041", r"\u"), (r"\101", r"\1"), (r"\0", r"\0"), (r"\a", r"\a"), (r"\f", r"\f"), (r"\v", r"\v"),
    (r"\Z", r"\Z"), (r"\G", r"\G"), (r"\<a", r"\<"), (r"a\>", r"\>"), ("\\é", "\\é"), ("\\ ", "\\ "), (r"[\A]", r"\A"), (r"[\z]", r"\z"),
    ("(?i)a", "flag group"), ("(?s).", "flag group"), ("(?x)a b", "flag group"), ("(?-u)a", "flag group"), ("(?i:a)", "flag group"),
    ("(?=a)", "flag group"), ("(?!a)", "flag group"), ("(?P=x)", "flag group"),
    ("(?<é>a)", "group name"), ("(?<1x>a)", "group name"),
    ("[[a]]", "'[' inside a class"), ("[[:alpha:]]", "'[' inside a class"), ("[a[b]", "'[' inside a class"), ("[a-[]", "'[' inside a class"),
    ("[a&&b]", "'&&'"), ("[a--b]", "'--'"), ("[a~~b]", "'~~'"), ("[--a]", "'--'"), ("[*--]", "'--'"), ("[]-a]", "after a leading ']'"),
    ("a{,2}", "{,m}"), ("a**", "quantifier applied to a quantifier"), ("a+*", "quantifier applied to a quantifier"),
    ("a{2}{3}", "quantifier applied to a quantifier"), ("a?+", "quantifier applied to a quantifier"),
    ("a*??", "quantifier applied to a quantifier"), ("a???", "quantifier applied to a quantifier"), ("(a)*+", "quantifier applied to a quantifier"),
    ("^*a", "applied to an anchor"), ("a$+", "applied to an anchor"), (r"\A?a", "applied to an anchor"), (r"a\z{2}", "applied to an anchor"),
    ("a{1001}", "repetition count"), ("a{2,1001}", "repetition count"),
    ("a{255}", "SLG_MAX_REGEX_STATES"), ("(ab){128}", "SLG_MAX_REGEX_STATES"), (".*a.{8}", "SLG_MAX_REGEX_STATES"),
    ("(" * 33 + "a" + ")" * 33, "nested deeper"),
]


# ---- random supported patterns ------------------------------------------------------------------------------
LITERALS = ("a", "a", "b", "b", "é", "€", "😀", "\n")
RANDOM_ALPHABET = ("a", "b", "é", "€", "😀", "\n")


def random_pattern(rng: random.Random, max_atoms: int = 12) -> str:
    """a pattern of the supported grammar with at most max_atoms atoms.  What bounds its DFA: counts of at most 3,
    and an unbounded repetition only over a single char, class or '.', never around a group"""
    budget = [rng.randint(1, max_atoms)]

    def literal():
        c = rng.choice(LITERALS)
        if c == "\n" and rng.random() < 0.5:
            return r"\n"
        return c

    def klass():
        items = []
        for _ in range(rng.randint(1, 3)):
            if rng.random() < 0.3:
                lo, hi = sorted((rng.choice("abé€😀"), rng.choice("abé€😀")), key=ord)
                items.append(lo + "-" + hi)
            else:
                items.append(rng.choice(("a", "b", "é", "€", "😀", "\n", r"\n", r"\]", r"\-", "^" if items else "a")))
        body = "".join(items)
        lead = rng.choice(("", "", "", "]"))
        if lead and body.startswith("-"):
            lead = ""
        tail = rng.choice(("", "", "-"))
        return "[" + rng.choice(("", "", "^")) + lead + body + tail + "]"

    def atom(depth):
        budget[0] -= 1
        r = rng.random()
        if r < 0.45:
            return literal(), True
        if r < 0.55:
            return ".", True
        if r < 0.70:
            return klass(), True
        if r < 0.76:
            return rng.choice(("^", "$", r"\A", r"\z")), None
        if depth >= 3 or budget[0] <= 0:
            return literal(), True
        opener = rng.choice(("(", "(", "(?:", "(?:", "(?P<g%d>" % budget[0], "(?<h%d>" % budget[0]))
        return opener + alt(depth + 1) + ")", False

    def piece(depth):
        a, simple = atom(depth)
        if simple is None or rng.random() < 0.55:          # (an anchor takes no quantifier)
            return a
        r = rng.random()
        if simple and r < 0.45:
            q = rng.choice(("*", "+", "{1,}", "{2,}"))
        elif r < 0.7:
            q = "?"
        else:
            lo = rng.randint(0, 2)
            q = rng.choice(("{%d}" % (lo + 1), "{%d,%d}" % (lo, rng.randint(lo, 3))))
        return a + q + rng.choice(("", "", "?"))

    def cat(depth):
        out = ""
        for _ in range(rng.randint(0 if depth else 1, 4)):
            if budget[0] <= 0:
                break
            out += piece(depth)
        return out

    def alt(depth):
        out = cat(depth)
        while budget[0] > 0 and rng.random() < 0.3:
            out += "|" + cat(depth)
        return out

    out = alt(0)
    while budget[0] > 0:
        out += piece(0)
    return out


def random_patterns(n=300, seed=2024):
    rng = random.Random(seed)
    return [random_pattern(rng) for _ in range(n)]


# ---- hand-made device rows ----------------------------------------------------------------------------------
def device_rows(seg_sorted_keys, req: dict):
    """per segment (positions, distances) of the first R passing keys of the request's range, R as the library
    states it; the predicate is tests/regex_ref.py's"""
    L = U.host_lib()
    keep = []
    cr = U.c_req(req, keep)
    rx = RR.compile_pattern(req["term"])
    pre = req["field"] + ":" + RR.regex_literal_prefix(req["term"])
    out = []
    for s, keys in enumerate(seg_sorted_keys):
        need = L.slgx_rows_needed(C.addressof(cr), s) if req["max_expansions"] > 0 else 0
        pos = [i for i, k in enumerate(keys)
               if k.startswith(pre) and len(k) > len(req["field"]) + 1 and rx.fullmatch(k[len(req["field"]) + 1:])][:need]
        out.append((pos, [0] * len(pos)))
    return out


class World(U.World):
    def want(self, req: dict):
        if req["kind"] != REGEX:
            return super().want(req)
        from tests import expand_ref as R
        keys = RR.expand_regex(self.sorted, req["field"], req["term"], req["max_expansions"])
        return R.term_rows(self.ids, [(k, 0) for k in keys])
