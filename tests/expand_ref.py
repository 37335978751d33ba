"""Python restatement of the reference's term expansion (searchlite-core/src/api/reader.rs), line for line, on
Python str (code points = Rust chars): bounded_levenshtein (:981-1018), expand_prefix (:1164-1210),
expand_wildcard (:1212-1283, with re.fullmatch on the same translated pattern, no DOTALL) and expand_term_fuzzy
(:1394-1465).  A segment is the byte-sorted list of its "field:term" keys (util/fst.rs:25-33: a BTreeMap), and
terms_with_prefix its keys that start with the prefix, in that order.  tests/test_expand_ref.py pins this file to
the reference's own tests; the device and the host merge are compared against it for exact equality.
"""
from __future__ import annotations

import re
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

NO_TERM = 0xFFFFFFFF


def sorted_keys(keys) -> List[str]:
    """the dictionary order: by UTF-8 bytes (Rust String order)"""
    return sorted(keys, key=lambda k: k.encode("utf-8"))


def terms_with_prefix(seg_keys: Sequence[str], prefix: str):
    """seg_keys is sorted by bytes; the keys that start with prefix, in order"""
    return [k for k in seg_keys if k.startswith(prefix)]


def char_prefix(s: str, n: int) -> str:           # :966-975
    return s[:n]


def distance_weight(distance: int) -> np.float32:  # :977-979
    return np.float32(1.0) / (np.float32(distance) + np.float32(1.0))


def bounded_levenshtein(a: str, b: str, max_edits: int) -> Optional[int]:   # :981-1018
    a_len = len(a)                                  # :982
    b_chars = list(b)                               # :983
    b_len = len(b_chars)                            # :984
    if abs(a_len - b_len) > max_edits:              # :985
        return None
    if a_len == 0:                                  # :988
        return b_len if b_len <= max_edits else None
    if b_len == 0:                                  # :991
        return a_len if a_len <= max_edits else None
    prev = list(range(b_len + 1))                   # :994
    curr = [0] * (b_len + 1)                        # :995
    for i, ca in enumerate(a):                      # :996
        curr[0] = i + 1
        row_min = curr[0]
        for j, cb in enumerate(b_chars):            # :999
            cost = 0 if ca == cb else 1
            dele = prev[j + 1] + 1
            ins = curr[j] + 1
            sub = prev[j] + cost
            val = min(dele, ins, sub)
            curr[j + 1] = val
            row_min = min(row_min, val)
        if row_min > max_edits:                     # :1008
            return None
        prev, curr = curr, prev                     # :1011
    return prev[b_len] if prev[b_len] <= max_edits else None   # :1013


def full_levenshtein(a: str, b: str) -> int:
    """the plain full-matrix distance (the yardstick of bounded_levenshtein in tests/test_expand_ref.py)"""
    d = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        d[i][0] = i
    for j in range(len(b) + 1):
        d[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            d[i][j] = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return d[len(a)][len(b)]


def expand_prefix(segments: Sequence[Sequence[str]], field: str, prefix: str, max_expansions: int) -> List[str]:
    """:1164-1210 -> keys"""
    if max_expansions == 0:                         # :1173
        return []
    prefix_key = field + ":" + prefix               # :1176
    field_prefix_len = len((field + ":").encode("utf-8"))   # :1177 (bytes)
    keys: List[str] = []
    seen = set()
    for seg in segments:                            # :1181
        expanded = 0
        for key in terms_with_prefix(seg, prefix_key):
            if expanded >= max_expansions:          # :1184
                break
            if len(key.encode("utf-8")) <= field_prefix_len:   # :1187
                continue
            if key in seen:                         # :1190
                continue
            seen.add(key)
            keys.append(key)                        # :1205
            expanded += 1
    return keys


def wildcard_literal_prefix(pattern: str) -> str:   # :1212-1214
    return re.split(r"[*?]", pattern)[0]


def build_wildcard_regex(pattern: str):             # :1216-1230 (fullmatch stands for ^ ... $)
    buf = ""
    for ch in pattern:
        if ch == "*":
            buf += ".*"
        elif ch == "?":
            buf += "."
        else:
            buf += re.escape(ch)
    return re.compile(buf)


def expand_wildcard(segments: Sequence[Sequence[str]], field: str, pattern: str, max_expansions: int) -> List[str]:
    """:1232-1283 -> keys"""
    if max_expansions == 0:                         # :1241
        return []
    regex = build_wildcard_regex(pattern)
    prefix_key = field + ":" + wildcard_literal_prefix(pattern)   # :1245-1246
    field_prefix_len = len((field + ":").encode("utf-8"))
    keys: List[str] = []
    seen = set()
    for seg in segments:                            # :1251
        expanded = 0
        for key in terms_with_prefix(seg, prefix_key):
            if expanded >= max_expansions:          # :1254
                break
            if len(key.encode("utf-8")) <= field_prefix_len:   # :1257
                continue
            term = key[len(field) + 1:]             # :1260
            if regex.fullmatch(term) is None:       # :1261
                continue
            if key in seen:                         # :1264
                continue
            seen.add(key)
            keys.append(key)                        # :1278
            expanded += 1
    return keys


def expand_term_fuzzy(segments: Sequence[Sequence[str]], field: str, term: str, max_edits: int, prefix_length: int,
                      max_expansions: int, min_length: int) -> List[Tuple[str, int]]:
    """expand_term_for_group's Exact arm with fuzzy options (:1137-1144), then :1394-1465 -> [(key, distance)]"""
    exact_key = field + ":" + term                  # :1403
    out = [(exact_key, 0)]                          # :1404-1411
    if min(max_edits, 2) == 0:                      # :1140-1143 expand_term_exact
        return out
    term_len = len(term)                            # :1402
    if term_len < min_length or max_expansions == 0:   # :1412
        return out
    max_edits = min(max_edits, 2)                   # :1415
    prefix_len = min(prefix_length, term_len)       # :1416
    prefix_key = field + ":" + char_prefix(term, prefix_len)   # :1417-1421
    field_prefix_len = len((field + ":").encode("utf-8"))      # :1422
    seen = {exact_key}                              # :1423-1424
    expansions = 0
    for seg in segments:                            # :1426
        for key in terms_with_prefix(seg, prefix_key):
            if expansions >= max_expansions:        # :1428
                return out
            if len(key.encode("utf-8")) <= field_prefix_len:   # :1431
                continue
            candidate = key[len(field) + 1:]        # :1434
            if candidate == term:                   # :1435
                continue
            if abs(len(candidate) - term_len) > max_edits:     # :1438-1441
                continue
            distance = bounded_levenshtein(term, candidate, max_edits)   # :1442
            if distance is None:
                continue
            if distance == 0:                       # :1445
                continue
            if key not in seen:                     # :1448
                seen.add(key)
                out.append((key, distance))
                expansions += 1
                if expansions >= max_expansions:    # :1458
                    return out
    return out


# ---- the shapes the library answers in -------------------------------------------------------------------------
FUZZY, PREFIX, WILDCARD = 0, 1, 2


def expand(segments: Sequence[Sequence[str]], req: dict) -> List[Tuple[str, int]]:
    """one request of GpuIndex.expand() -> [(key, distance)]"""
    if req["kind"] == FUZZY:
        return expand_term_fuzzy(segments, req["field"], req["term"], req["max_edits"], req["prefix_length"],
                                 req["max_expansions"], req["min_length"])
    fn = expand_prefix if req["kind"] == PREFIX else expand_wildcard
    return [(k, 0) for k in fn(segments, req["field"], req["term"], req["max_expansions"])]


def term_rows(seg_ids: Sequence[Dict[str, int]], keyed: Sequence[Tuple[str, int]]):
    """[(key, distance)] -> (term ids u32[n, n_segs] with NO_TERM holes, distances u8[n]); seg_ids[s]: key -> id"""
    ids = np.full((len(keyed), len(seg_ids)), NO_TERM, dtype=np.uint32)
    for r, (key, _) in enumerate(keyed):
        for s, d in enumerate(seg_ids):
            ids[r, s] = d.get(key, NO_TERM)
    return ids, np.array([d for _, d in keyed], dtype=np.uint8)
