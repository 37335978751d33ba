"""The synthetic dictionaries of tests/test_gpu_expand.py and the requests that go with them.  Every boundary
that depends on the scan's geometry is built from the constants the library exports (wave, workgroup, chunk)."""
from __future__ import annotations

import itertools
import random

import numpy as np

from searchlite_amd import _native as N
from searchlite_amd.segment import Segment
from tests import expand_util as U

WAVE, GROUP, CHUNK = N.EXPAND_WAVE, N.EXPAND_WORKGROUP, N.EXPAND_CHUNK


def dict_segment(keys) -> Segment:
    """a one-doc segment whose terms are `keys` in term-id order (one posting each): a dictionary to expand against"""
    v = len(keys)
    return Segment(n_docs=1, term_offsets=np.arange(v + 1, dtype=np.uint64), doc_ids=np.zeros(v, np.uint32),
                   tfs=np.ones(v, np.uint32), field_doc_len=[np.ones(1, np.float32)], field_avgdl=np.ones(1, np.float32),
                   docs=1.0, term_dict={k: i for i, k in enumerate(keys)})


def word(i: int, width: int = 4) -> str:
    """the i-th lowercase word of `width` letters in byte order"""
    out = []
    for _ in range(width):
        out.append(chr(ord("a") + i % 26))
        i //= 26
    return "".join(reversed(out))


# ---- ranges of exact sizes with passing keys at chosen positions ------------------------------------------------
RANGE_SIZES = [1, WAVE - 1, WAVE, WAVE + 1, GROUP - 1, GROUP, GROUP + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]


def flags_of(i: int, n: int) -> str:
    """the marks of key i of a range of n keys: a wildcard '*X*' passes exactly the keys marked X"""
    f = ""
    if i == 0:
        f += "F"
    if i == n - 1:
        f += "L"
    if any(i in (b - 1, b) for b in (WAVE, GROUP, CHUNK, 2 * CHUNK) if b < n):
        f += "S"                                     # the keys on both sides of every boundary inside the range
    if i in set(np.linspace(0, n - 1, min(50, n)).astype(int).tolist()):
        f += "E"                                     # up to 50 keys spread over the whole range
    if i in set(np.linspace(0, n - 1, min(51, n)).astype(int).tolist()):
        f += "M"                                     # one more
    return f


def range_world():
    """one segment: field r<n> holds exactly n keys; field b<n> holds n keys of which the first is the bare key;
    sibling fields around them.  Term ids are a shuffle of the byte order."""
    keys = ["bod:x", "body2:y", "r:", "zz:last"]
    for n in RANGE_SIZES:
        keys += [f"r{n}:{word(i)}{flags_of(i, n)}" for i in range(n)]
    for n in (1, WAVE, WAVE + 1, CHUNK + 1):
        keys += [f"b{n}:"] + [f"b{n}:{word(i)}" for i in range(n - 1)]
    random.Random(3).shuffle(keys)
    return [keys]


def range_requests():
    reqs = []
    for n in RANGE_SIZES:
        f = f"r{n}"
        reqs += [U.wildcard(f, "*F*"), U.wildcard(f, "*L*"), U.wildcard(f, "*S*"), U.wildcard(f, "*E*", 50),
                 U.wildcard(f, "*M*", 50), U.wildcard(f, "*M*", 1), U.wildcard(f, "*", 50), U.wildcard(f, "*", 1),
                 U.wildcard(f, "*", 0), U.wildcard(f, "*", 1024), U.prefix(f, "", 50), U.prefix(f, "", 1024),
                 U.prefix(f, "", 1), U.prefix(f, "", 0), U.prefix(f, word(n - 1), 5), U.prefix(f, "zzzzz", 5),
                 U.fuzzy(f, word(0) + "F", max_edits=2, prefix_length=0, min_length=0),
                 U.fuzzy(f, word(n - 1), max_edits=2, prefix_length=9, min_length=0)]
    for n in (1, WAVE, WAVE + 1, CHUNK + 1):
        reqs += [U.prefix(f"b{n}", "", 50), U.wildcard(f"b{n}", "*", 1024), U.fuzzy(f"b{n}", "aaab", 2, 0, 50, 0)]
    # sibling fields do not leak; the whole dictionary is no field's range; the range at the dictionary's end
    reqs += [U.prefix("body", "", 50), U.prefix("bod", "", 50), U.prefix("body2", "", 50), U.prefix("r", "", 50),
             U.prefix("zz", "", 50), U.prefix("zz", "last", 50), U.wildcard("zz", "l*", 50), U.prefix("zzz", "", 50),
             U.fuzzy("zz", "lest", 1, 1, 50, 3), U.fuzzy("r", "abc", 2, 0, 50, 0)]
    return reqs


def whole_world():
    """one field is the whole dictionary: the range of prefix_length 0 is every key"""
    return [[f"t:{word(i, 3)}" for i in range(CHUNK + WAVE + 1)]]


def whole_requests():
    return [U.prefix("t", "", 1024), U.wildcard("t", "*", 1024), U.wildcard("t", "?b*", 50),
            U.fuzzy("t", "abc", 2, 0, 50, 0), U.fuzzy("t", "abc", 1, 0, 3, 0), U.fuzzy("t", word(CHUNK + WAVE, 3), 1, 5, 50, 0)]


# ---- passing keys spread over many chunks -----------------------------------------------------------------------
def dense_world():
    """every word over {a, b, c} of 1 .. 7 letters: 3279 keys, fuzzy matches of a term all over the field"""
    return [["d:" + "".join(w) for n in range(1, 8) for w in itertools.product("abc", repeat=n)]]


def dense_requests():
    reqs = []
    for term in ("abcab", "cc", "b", "abcabca", "bbbbbbb"):
        for me in (0, 1, 2, 3):
            for pl in (0, 1, 2, 9):
                for mx in (1, 7, 50, 1024):
                    reqs.append(U.fuzzy("d", term, me, pl, mx, 0))
    reqs += [U.wildcard("d", p, mx) for p in ("*", "a*b*c", "?", "??", "*c", "c*", "ab?ab*") for mx in (1, 50, 1024)]
    return reqs


# ---- distances, UTF-8, wildcards: small hand-made vocabularies --------------------------------------------------
def words_world():
    body = ["rust", "rusk", "rusts", "trust", "rut", "ust", "rsut", "bust", "best", "trusts", "ru", "r", "rs", "rus",
            "rustabc", "rustab", "rusta", "dusk", "urst", "ruts", "tsur", "a" * 128, "a" * 127 + "b", "a" * 129,
            "a" * 130, "a" * 131, "a" * 127, "a" * 126,
            "café", "cafe", "caffe", "cafés", "naïve", "naive", "naïf", "東京", "東亰", "京都", "東京都", "😀a", "😀b", "a😀",
            "😀", "éééé", "ééé", "ééééa", "éééaaa", "aaaaaa", "éé",
            "z" * 300, "é" * 252]   # (255 chars and more with the field: the saturated char count)
    glob = ["abc", "aXbXbc", "ac", "abbc", "a\nc", "ab", "b", "é", "aé", "aéc", "xyzc", "a\n", "\n", "abcabc", "a*c"]
    return [["body:" + w for w in body] + ["kw:" + w for w in glob] + ["body:", "kw:"]]


def words_requests():
    reqs = []
    for term in ("rust", "rusk", "rsut", "r", "ru", "rus", "tsur", "a" * 128, "a" * 127, "café", "cafe", "naïve", "東京",
                 "😀a", "éééé", "aaaaaa", "ééé", ""):
        for me in (0, 1, 2, 3):
            for pl in (0, 1, 4, 200):
                reqs.append(U.fuzzy("body", term, me, pl, 50, 0))
    reqs += [U.fuzzy("body", "ru", 1, 1, 20, 3), U.fuzzy("body", "rus", 1, 1, 20, 3), U.fuzzy("body", "rust", 1, 1, 0, 3)]
    for p in ("*", "*c", "a*", "a*b*c", "?", "a?", "a?c", "abc", "a*c", "??", "*\n*", "a\n*", "a\\*c", "é", "?é*", "**", "*?"):
        reqs += [U.wildcard("kw", p, 50), U.wildcard("kw", p, 1)]
    reqs += [U.prefix("kw", p, 50) for p in ("", "a", "ab", "a\n", "é", "q")]
    return reqs


# ---- segments ------------------------------------------------------------------------------------------------
def segments_world():
    """three segments with overlapping and disjoint vocabularies, term ids in another order than the bytes in one of
    them; r000 .. r099 in every segment: a per-segment prefix cap meets the duplicates of two earlier segments"""
    rs = [f"body:r{i:03d}" for i in range(100)]
    s0 = rs + ["body:rush", "body:rust", "body:ruse", "title:only0"]
    s1 = list(reversed(rs)) + ["body:rust", "body:bust", "body:rusk", "body:ruts", "body:only1"]
    s2 = rs + ["body:r100", "body:r101", "title:rust", "body:dust", "body:rusk"]
    return [s0, s1, s2]


def segments_requests():
    reqs = [U.prefix("body", "r", mx) for mx in (1, 2, 10, 40, 99, 100, 101, 1024)]
    reqs += [U.wildcard("body", "r0*", mx) for mx in (1, 10, 99, 100)] + [U.wildcard("body", "?us?", mx) for mx in (1, 2, 3, 50)]
    reqs += [U.fuzzy("body", "rust", me, pl, mx, 3) for me in (1, 2) for pl in (0, 1) for mx in (1, 2, 3, 4, 5, 50)]
    reqs += [U.fuzzy("body", "r05", 1, 1, mx, 0) for mx in (5, 15, 30, 200)] + [U.fuzzy("title", "rusx", 1, 1, 50, 3)]
    reqs += [U.prefix("title", "", 50), U.prefix("nope", "", 50)]
    return reqs


def random_world(seed=1234):
    rng = random.Random(seed)
    vocab = sorted({"".join(rng.choice("abcé") for _ in range(rng.randrange(1, 9))) for _ in range(2600)})
    segs = []
    for _ in range(3):
        keys = ["w:" + x for x in rng.sample(vocab, 800)] + ["x:" + x for x in rng.sample(vocab, 40)]
        rng.shuffle(keys)
        segs.append(keys)
    return segs, vocab


def random_requests(vocab, n=300, seed=99):
    rng = random.Random(seed)
    reqs = []
    for _ in range(n):
        kind = rng.choice((U.FUZZY, U.FUZZY, U.PREFIX, U.WILDCARD))
        f = rng.choice(("w", "w", "w", "x"))
        wd = rng.choice(vocab)
        if kind == U.FUZZY:
            if rng.random() < 0.3:                  # a typo of a word
                i = rng.randrange(len(wd))
                wd = wd[:i] + rng.choice("abcé") + wd[i + rng.randrange(2):]
            reqs.append(U.fuzzy(f, wd, rng.choice((0, 1, 2, 3)), rng.choice((0, 1, 2, 9)), rng.choice((0, 1, 5, 50, 1024)),
                                rng.choice((0, 3))))
        elif kind == U.PREFIX:
            reqs.append(U.prefix(f, wd[:rng.randrange(0, 3)], rng.choice((0, 1, 5, 50, 1024))))
        else:
            p = "".join(rng.choice((c, c, "*", "?")) for c in wd[:rng.randrange(1, 5)])
            reqs.append(U.wildcard(f, p, rng.choice((0, 1, 5, 50, 1024))))
    return reqs
