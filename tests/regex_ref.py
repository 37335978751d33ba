"""Python restatement of the reference's regex term expansion (searchlite-core/src/api/reader.rs): the literal-prefix
rule regex_literal_prefix (:1285-1320) and the loop expand_regex (:1322-1373), line for line on Python str, with the
match of ^(?:pattern)$ (util/regex.rs) done by Python's `re`: a small tokenizer of the SUPPORTED pattern language
(include/searchlite_gpu.h, "REGEX"), written independently of the library's C++ parser as one flat scan with a
stack, classifies a pattern as supported, unsupported or invalid and translates a supported one ($ and \\z -> \\Z,
^ -> \\A, (?<n> -> (?P<n>, every literal escaped), and re.fullmatch decides.  A backtracking engine is a properly
independent check on the library's DFA.  Within the supported language the two engines agree: '.' is any char but
U+000A in both (no DOTALL), a negated class contains U+000A in both, an empty alternative matches the empty string.
"""
from __future__ import annotations

import re
from typing import List, Sequence

from tests.expand_ref import terms_with_prefix

SUPPORTED, UNSUPPORTED, INVALID = "supported", "unsupported", "invalid"
REGEX = 4
MAX_REPEAT = 1000


class Refused(Exception):
    def __init__(self, status: str, what: str):
        super().__init__(f"{status}: {what}")
        self.status, self.what = status, what


_PUNCT = set(chr(c) for c in range(0x21, 0x7F) if not chr(c).isalnum())
_COUNT = re.compile(r"\{(\d+)(?:(,)(\d*))?\}")
_NAME = re.compile(r"[A-Za-z_][A-Za-z0-9_]*\Z")


def _escape(p: str, i: int, in_class: bool):
    """the escape whose '\\' is p[i] -> (python text, next index, is an anchor)"""
    if i + 1 >= len(p):
        raise Refused(INVALID, "trailing backslash")
    e = p[i + 1]
    if e in "ntr":
        return "\\" + e, i + 2, False
    if not in_class and e == "A":
        return r"\A", i + 2, True
    if not in_class and e == "z":
        return r"\Z", i + 2, True
    if e in _PUNCT and e not in "<>":
        return re.escape(e), i + 2, False
    raise Refused(UNSUPPORTED, "escape \\" + e)


def _class(p: str, i: int):
    """the class whose '[' is p[i] -> (python text, next index)"""
    start = i
    out = "["
    i += 1
    if i < len(p) and p[i] == "^":
        out += "^"
        i += 1
    if i < len(p) and p[i] == "]":
        out += r"\]"
        i += 1
        if i + 1 < len(p) and p[i] == "-" and p[i + 1] != "]":
            raise Refused(UNSUPPORTED, "'-' after a leading ']'")
    while True:
        if i >= len(p):
            raise Refused(INVALID, f"unclosed '[' at {start}")
        c = p[i]
        if c == "]":
            return out + "]", i + 1
        if c == "[":
            raise Refused(UNSUPPORTED, "'[' inside a class")
        if c in "&-~" and p[i + 1:i + 2] == c:
            raise Refused(UNSUPPORTED, c + c + " inside a class")

        def prim(j):
            if p[j] == "\\":
                text, j2, _ = _escape(p, j, True)
                return text, j2, {"\\n": "\n", "\\t": "\t", "\\r": "\r"}.get(text, p[j + 1])
            return re.escape(p[j]), j + 1, p[j]
        lo_text, i, lo = prim(i)
        if i + 1 < len(p) and p[i] == "-" and p[i + 1] != "]":
            if p[i + 1] == "-":
                raise Refused(UNSUPPORTED, "-- inside a class")
            if p[i + 1] == "[":
                raise Refused(UNSUPPORTED, "'[' inside a class")
            hi_text, i, hi = prim(i + 1)
            if ord(lo) > ord(hi):
                raise Refused(INVALID, "reversed range")
            out += lo_text + "-" + hi_text
        else:
            out += lo_text


def translate(p: str) -> str:
    """a supported pattern as a Python `re` pattern for re.fullmatch; raises Refused(UNSUPPORTED | INVALID)"""
    out: List[str] = []
    open_groups = 0
    names = set()
    # what a quantifier would meet: "none" (start, after '(' or '|'), "atom", "anchor", "quant" (a quantifier, which
    # may still take its lazy '?'), "lazy"
    last = "none"
    i = 0
    while i < len(p):
        c = p[i]
        if c in "*+?{":
            if last == "quant" and c == "?":
                out.append("?")
                last = "lazy"
                i += 1
                continue
            if last in ("quant", "lazy"):
                raise Refused(UNSUPPORTED, "a quantifier applied to a quantifier")
            if last == "none":
                raise Refused(INVALID, "nothing to repeat")
            if last == "anchor":
                raise Refused(UNSUPPORTED, "a quantifier applied to an anchor")
            if c == "{":
                m = _COUNT.match(p, i)
                if m is None:
                    if re.compile(r"\{,\d+\}").match(p, i):
                        raise Refused(UNSUPPORTED, "{,m}")
                    raise Refused(INVALID, "'{' that is no counted repetition")
                lo = int(m.group(1))
                hi = lo if m.group(2) is None else (None if m.group(3) == "" else int(m.group(3)))
                if hi is not None and lo > hi:
                    raise Refused(INVALID, "{n,m} with n > m")
                if lo > MAX_REPEAT or (hi is not None and hi > MAX_REPEAT):
                    raise Refused(UNSUPPORTED, "repetition count")
                out.append(m.group(0))
                i = m.end()
            else:
                out.append(c)
                i += 1
            last = "quant"
        elif c == "\\":
            text, i, anchor = _escape(p, i, False)
            out.append(text)
            last = "anchor" if anchor else "atom"
        elif c == "(":
            i += 1
            if p[i:i + 1] == "?":
                if p[i + 1:i + 2] == ":":
                    out.append("(?:")
                    i += 2
                elif p[i + 1:i + 2] == "<" or p[i + 1:i + 3] == "P<":
                    j = i + (2 if p[i + 1] == "<" else 3)
                    end = p.find(">", j)
                    if end < 0 or end == j:
                        raise Refused(INVALID, "group name")
                    name = p[j:end]
                    if not _NAME.match(name):
                        raise Refused(UNSUPPORTED, "group name")
                    if name in names:
                        raise Refused(INVALID, "duplicate group name")
                    names.add(name)
                    out.append(f"(?P<{name}>")
                    i = end + 1
                elif i + 1 >= len(p):
                    raise Refused(INVALID, "unbalanced '('")
                else:
                    raise Refused(UNSUPPORTED, "flag group")
            else:
                out.append("(")
            open_groups += 1
            last = "none"
        elif c == ")":
            if open_groups == 0:
                raise Refused(INVALID, "unbalanced ')'")
            open_groups -= 1
            out.append(")")
            i += 1
            last = "atom"
        elif c == "|":
            out.append("|")
            i += 1
            last = "none"
        elif c == "[":
            text, i = _class(p, i)
            out.append(text)
            last = "atom"
        elif c in "^$":
            out.append(r"\A" if c == "^" else r"\Z")
            i += 1
            last = "anchor"
        elif c == ".":
            out.append(".")
            i += 1
            last = "atom"
        else:
            out.append(re.escape(c))
            i += 1
            last = "atom"
    if open_groups:
        raise Refused(INVALID, "unbalanced '('")
    return "".join(out)


def classify(p: str) -> str:
    try:
        translate(p)
    except Refused as e:
        return e.status
    return SUPPORTED


def compile_pattern(p: str):
    return re.compile(translate(p))


def regex_literal_prefix(pattern: str) -> str:      # :1285-1320
    prefix = ""                                     # :1286
    escaped = False                                 # :1287
    for ch in pattern:                              # :1288
        if escaped:                                 # :1289
            if ch == "\\":                          # :1291
                prefix += ch
                escaped = False
                continue
            if ch in "dDwWsSbB":                    # :1299
                break
            if ch in "pP":                          # :1300
                break
            prefix += ch                            # :1301-1306
            escaped = False
            continue
        if ch == "\\":                              # :1310
            escaped = True
        elif ch == "^" and prefix == "":            # :1311
            continue
        elif ch in ".*+?()[]{}|$":                  # :1312
            break
        else:
            prefix += ch                            # :1313-1316
    return prefix


def expand_regex(segments: Sequence[Sequence[str]], field: str, pattern: str, max_expansions: int) -> List[str]:
    """:1322-1373 -> keys.  (The planner compiles the pattern before this runs, query/planner.rs:599: an invalid
    pattern is an error whatever max_expansions is; here compile_pattern raises Refused.)"""
    regex = compile_pattern(pattern)                # planner.rs:599 / :1334
    if max_expansions == 0:                         # :1331
        return []
    literal_prefix = regex_literal_prefix(pattern)  # :1335
    prefix_key = field + ":" + literal_prefix       # :1336
    field_prefix_len = len((field + ":").encode("utf-8"))   # :1337
    keys: List[str] = []
    seen = set()                                    # :1340
    for seg in segments:                            # :1341
        expanded = 0
        for key in terms_with_prefix(seg, prefix_key):
            if expanded >= max_expansions:          # :1344
                break
            if len(key.encode("utf-8")) <= field_prefix_len:   # :1347
                continue
            term = key[len(field) + 1:]             # :1350
            if regex.fullmatch(term) is None:       # :1351
                continue
            if key in seen:                         # :1354
                continue
            seen.add(key)
            keys.append(key)                        # :1368
            expanded += 1
    return keys


def regex(field, term, max_expansions=50):
    """a request of GpuIndex.expand()"""
    return dict(kind=REGEX, field=field, term=term, max_expansions=max_expansions, max_edits=0, prefix_length=0,
                min_length=0)


def wildcard_as_regex(pattern: str) -> str:
    """a wildcard pattern whose literals hold no regex metacharacter, as the regex with the same literal prefix and
    the same language: '*' -> '.*', '?' -> '.'"""
    assert not set(pattern) & set("\\.+()[]{}|^$")
    return pattern.replace("*", ".*").replace("?", ".")
