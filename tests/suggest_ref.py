"""Python restatement of the reference's completion suggester (searchlite-core/src/api/reader.rs), line for line:
collect_completion_candidates (:1785-1877) and completion_suggest (:1941-1977), on Python str (code points = Rust
chars) and np.float32 (one rounding per operation, as Rust's f32).  A segment is the byte-sorted list of its
("field:term" key, df) pairs: terms_with_prefix yields the keys that start with the prefix in that order, and df is
PostingsReader::len() of the key, whatever has been deleted.  tests/test_suggest_ref.py pins this file to the
reference's own test; the device and the host-compiled merge are compared against it for exact equality.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from tests.expand_ref import bounded_levenshtein, char_prefix, distance_weight

DEFAULT_SUGGEST_SCAN = 64        # :618
MAX_SUGGEST_CANDIDATES = 256     # :619

FUZZY_DEFAULTS = dict(max_edits=1, prefix_length=1, max_expansions=50, min_length=3)   # FuzzyOptions::default

Segment = Sequence[Tuple[str, int]]


def sorted_segment(key_df) -> List[Tuple[str, int]]:
    """(key, df) pairs (or a dict) in the dictionary's order: by UTF-8 bytes"""
    items = key_df.items() if isinstance(key_df, dict) else key_df
    return sorted(items, key=lambda kv: kv[0].encode("utf-8"))


def collect_completion_candidates(segments: Sequence[Segment], field: str, term: str, size: int,
                                  fuzzy: Optional[dict]) -> Dict[str, list]:
    """:1785-1877 -> text -> [doc_freq, score (np.float32)]"""
    out: Dict[str, list] = {}                                        # :1792
    max_candidates = min(max(size * 5, DEFAULT_SUGGEST_SCAN), MAX_SUGGEST_CANDIDATES)   # :1793-1795
    expanded_total = 0                                               # :1796
    field_prefix_len = len(field.encode("utf-8")) + 1                # :1800, :1839 (bytes)

    def add(text, df, weight):
        entry = out.setdefault(text, [0, np.float32(0.0)])           # :1814, :1862 or_default
        entry[0] += df                                               # :1815, :1863
        part = np.float32(df) if weight is None else np.float32(weight * np.float32(df))
        entry[1] = np.float32(entry[1] + part)                       # :1816, :1864

    if fuzzy is None:                                                # :1798
        prefix_key = field + ":" + term                              # :1799
        for seg in segments:                                         # :1801
            for key, df in seg:
                if not key.startswith(prefix_key):                   # :1802 terms_with_prefix
                    continue
                if expanded_total >= max_candidates:                 # :1803
                    break
                if len(key.encode("utf-8")) <= field_prefix_len:     # :1806
                    continue
                if df == 0:                                          # :1811
                    continue
                add(key[len(field) + 1:], df, None)
                expanded_total += 1                                  # :1817
                if expanded_total >= max_candidates:                 # :1818
                    break
            if expanded_total >= max_candidates:                     # :1822
                break
        return out
    term_len = len(term)                                             # :1828
    if term_len < fuzzy["min_length"] or fuzzy["max_expansions"] == 0:   # :1829
        return out
    max_edits = min(fuzzy["max_edits"], 2)                           # :1832
    if max_edits == 0:                                               # :1833
        return out
    prefix_len = min(fuzzy["prefix_length"], term_len)               # :1836
    prefix_key = field + ":" + char_prefix(term, prefix_len)         # :1837-1838
    global_cap = max(min(fuzzy["max_expansions"], MAX_SUGGEST_CANDIDATES), size)   # :1840-1841
    for seg in segments:                                             # :1842
        for key, df in seg:
            if not key.startswith(prefix_key):                       # :1843
                continue
            if expanded_total >= global_cap:                         # :1844
                break
            if len(key.encode("utf-8")) <= field_prefix_len:         # :1847
                continue
            candidate = key[len(field) + 1:]                         # :1850
            if abs(len(candidate) - term_len) > max_edits:           # :1851-1853
                continue
            distance = bounded_levenshtein(term, candidate, max_edits)   # :1855
            if distance is None:
                continue
            if df == 0:                                              # :1859
                continue
            add(candidate, df, distance_weight(distance))
            expanded_total += 1                                      # :1865
            if expanded_total >= global_cap:                         # :1866
                break
        if expanded_total >= global_cap:                             # :1870
            break
    return out


def completion_suggest(segments: Sequence[Segment], field: str, term: str, size: int,
                       fuzzy: Optional[dict]) -> List[Tuple[str, np.float32, int]]:
    """:1941-1977 with completion_inputs' one input already in hand -> [(text, score, doc_freq)]"""
    if size == 0:                                                    # :1948
        return []
    merged: Dict[str, list] = {}                                     # :1952
    for text, (df, score) in collect_completion_candidates(segments, field, term, size, fuzzy).items():   # :1954
        entry = merged.setdefault(text, [0, np.float32(0.0)])
        entry[0] += df                                               # :1957
        entry[1] = np.float32(entry[1] + score)                      # :1958
    options = [(text, score, df) for text, (df, score) in merged.items()]
    options.sort(key=lambda o: (-float(o[1]), o[0].encode("utf-8")))   # :1969-1974 (f32 -> f64 is exact and monotonic)
    return options[:size]                                            # :1975


def suggest(segments: Sequence[Segment], req: dict):
    """one request of GpuIndex.suggest() (searcher.suggest_request)"""
    fz = req.get("fuzzy")
    return completion_suggest(segments, req["field"], req["term"], req.get("size", 5),
                              None if fz is None else dict(FUZZY_DEFAULTS, **fz))


def bits(options):
    """options in a form that compares exactly: text, the score's f32 bit pattern, doc_freq"""
    return [(t, int(np.float32(s).view(np.uint32)), int(d)) for t, s, d in options]
