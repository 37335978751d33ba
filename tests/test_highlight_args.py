"""The argument checks of slg_highlight_batch / slg_batch_highlight (csrc/slg_highlight_host.cpp: the one validation
of both entry points) through its test C ABI (slgx_hl_validate in lib/libslg_plan.so), against hand-made index
facts: every SLG_ERR_INVALID and SLG_ERR_UNSUPPORTED of searchlite_gpu.h, each limit at its value and one above.  The
limits are read from the header.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from searchlite_amd import _native as N
from searchlite_amd.highlight import highlight_spec as spec, pack_specs
from tests import highlight_worlds as W

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "searchlite_gpu.h")


def header_limit(name):
    m = re.search(r"#define\s+%s\s+(\d+)u" % name, open(HEADER).read())
    assert m, name
    return int(m.group(1))


MAX_TERMS, MAX_PHRASES = header_limit("SLG_MAX_HL_TERMS"), header_limit("SLG_MAX_HL_PHRASES")
MAX_PHRASE_WORDS, MAX_WORD = header_limit("SLG_MAX_PHRASE_TERMS"), header_limit("SLG_MAX_EXPAND_CHARS")
MAX_TAG, MAX_FRAGMENT, MAX_FRAGMENTS = header_limit("SLG_MAX_HL_TAG"), header_limit("SLG_MAX_HL_FRAGMENT"), header_limit("SLG_MAX_HL_FRAGMENTS")


def test_the_limits_are_the_ones_the_issue_names_and_python_mirrors_them():
    assert (MAX_TERMS, MAX_PHRASES, MAX_PHRASE_WORDS, MAX_WORD, MAX_TAG, MAX_FRAGMENT, MAX_FRAGMENTS) == (32, 8, 8, 128, 64, 1024, 8)
    assert (N.MAX_HL_TERMS, N.MAX_HL_PHRASES, N.MAX_PHRASE_TERMS, N.MAX_EXPAND_CHARS, N.MAX_HL_TAG, N.MAX_HL_FRAGMENT,
            N.MAX_HL_FRAGMENTS) == (MAX_TERMS, MAX_PHRASES, MAX_PHRASE_WORDS, MAX_WORD, MAX_TAG, MAX_FRAGMENT, MAX_FRAGMENTS)
    assert C.sizeof(N.HlSpec) == 72 and C.sizeof(N.HlOut) == 72   # as a C compiler lays slg_hl_spec / slg_hl_out out


# the index facts every call here is checked against: two segments of 3 and 2 docs, text fields 0 and 4
SEG_DOCS = np.array([3, 2], np.uint32)
FIELDS = np.array([0, 4], np.int32)


def validate(specs_per_query, hits_per_query=None, batch_form=False, out=None, mutate=None, raw=None):
    """-> (rc, message).  mutate(arr, soffs, hoffs, seg, doc): change the packed arrays before the call; raw: a dict
    of arguments that replace the packed ones (None = NULL)."""
    L = W.plan_lib()
    nq = len(specs_per_query)
    soffs, arr, keep = pack_specs(specs_per_query)
    hits_per_query = hits_per_query if hits_per_query is not None else [[(0, 0)]] * nq
    hoffs = np.zeros(nq + 1, np.uint32)
    np.cumsum([len(h) for h in hits_per_query], out=hoffs[1:])
    flat = [x for h in hits_per_query for x in h]
    seg = np.array([s for s, _ in flat] + [0], np.uint32)
    doc = np.array([d for _, d in flat] + [0], np.uint32)
    o = out if out is not None else N.HlOut(struct_size=C.sizeof(N.HlOut))
    if mutate:
        mutate(arr, soffs, hoffs, seg, doc)
    args = dict(hoffs=hoffs.ctypes.data, seg=seg.ctypes.data, doc=doc.ctypes.data, soffs=soffs.ctypes.data,
                specs=C.addressof(arr), out=C.addressof(o))
    args.update(raw or {})
    err = C.create_string_buffer(512)
    vp = C.c_void_p
    rc = L.slgx_hl_validate(C.c_uint32(nq), C.c_int(int(batch_form)), vp(args["hoffs"]), vp(args["seg"]), vp(args["doc"]),
                            vp(args["soffs"]), vp(args["specs"]), C.c_uint32(len(SEG_DOCS)), vp(SEG_DOCS.ctypes.data),
                            vp(FIELDS.ctypes.data), C.c_uint32(len(FIELDS)), vp(args["out"]), None, None, err, C.c_uint32(512))
    del keep
    return rc, err.value.decode()


GOOD = spec(0, ["rust", "go"], [["new", "york"], ["a"]])


def test_a_valid_call_in_both_forms():
    assert validate([[GOOD], [], [GOOD, spec(4, [], [])]], [[(0, 2), (1, 1)], [], [(1, 0)]]) == (N.OK, "")
    assert validate([[GOOD]], batch_form=True, raw=dict(hoffs=None, seg=None, doc=None)) == (N.OK, "")


@pytest.mark.parametrize("raw, what", [
    (dict(out=None), "out is NULL"),
    (dict(soffs=None), "spec_offsets is NULL"),
    (dict(specs=None), "specs is NULL"),
    (dict(hoffs=None), "hit_offsets is NULL"),
    (dict(seg=None), "hit_seg or hit_doc is NULL"),
    (dict(doc=None), "hit_seg or hit_doc is NULL"),
])
def test_null_arrays(raw, what):
    rc, msg = validate([[GOOD]], raw=raw)
    assert rc == N.ERR_INVALID and what in msg


def set_field(name, value, which=0):
    def m(arr, *_):
        setattr(arr[which], name, value)
    return m


@pytest.mark.parametrize("mutate, what", [
    (set_field("struct_size", 71), "struct_size"),
    (set_field("text_field", 1), "unknown text field id 1"),
    (set_field("text_field", -1), "unknown text field id -1"),
    (set_field("phrase_offsets", None), "phrase_offsets is NULL"),
    (set_field("word_offsets", None), "word_offsets is NULL"),
    (set_field("word_bytes", None), "word_bytes is NULL"),
    (set_field("pre_tag", None), "pre_tag is NULL"),
    (set_field("post_tag", None), "post_tag is NULL"),
    (lambda arr, soffs, *_: soffs.__setitem__(1, 5) or soffs.__setitem__(2, 1), "spec_offsets decrease"),
    (lambda arr, soffs, *_: soffs.__setitem__(0, 1), "spec_offsets does not start at 0"),
    (lambda arr, soffs, hoffs, *_: hoffs.__setitem__(1, 9) or hoffs.__setitem__(2, 1), "hit_offsets decrease"),
    (lambda arr, soffs, hoffs, seg, doc: seg.__setitem__(0, 2), "segment 2 is out of range"),
    (lambda arr, soffs, hoffs, seg, doc: doc.__setitem__(0, 3), "doc 3 is out of range"),
    (lambda arr, soffs, hoffs, seg, doc: (seg.__setitem__(1, 1), doc.__setitem__(1, 2)), "doc 2 is out of range"),
])
def test_invalid_arguments(mutate, what):
    rc, msg = validate([[GOOD], [GOOD]], [[(0, 2)], [(0, 0)]], mutate=mutate)
    assert rc == N.ERR_INVALID and what in msg, msg


def poke_u32(address, index, value):
    C.cast(address, C.POINTER(C.c_uint32))[index] = value


def test_offsets_inside_a_spec():
    # GOOD's words: rust go | new york | a -> word_offsets 0 4 6 9 13 14, phrase_offsets 0 2 3
    for mutate, what in [
        (lambda arr, *_: poke_u32(arr[0].word_offsets, 2, 3), "word_offsets decrease"),
        (lambda arr, *_: poke_u32(arr[0].word_offsets, 0, 1), "word_offsets does not start at 0"),
        (lambda arr, *_: poke_u32(arr[0].word_offsets, 1, 0), "term 0 is empty"),
        (lambda arr, *_: poke_u32(arr[0].word_offsets, 3, 6), "a phrase holds an empty word"),
        (lambda arr, *_: poke_u32(arr[0].phrase_offsets, 1, 3), "phrase 1 has no words"),
        (lambda arr, *_: poke_u32(arr[0].phrase_offsets, 1, 0), "phrase 0 has no words"),
        (lambda arr, *_: poke_u32(arr[0].phrase_offsets, 0, 1), "phrase_offsets does not start at 0"),
        (lambda arr, *_: (poke_u32(arr[0].phrase_offsets, 1, 3), poke_u32(arr[0].phrase_offsets, 2, 2)), "phrase_offsets decrease"),
    ]:
        rc, msg = validate([[GOOD]], mutate=mutate)
        assert rc == N.ERR_INVALID and what in msg, (what, msg)


def test_the_python_layer_drops_empties_but_the_c_abi_refuses_them():
    s = spec(0, ["", "rust"], [[], ["new", "york"]])
    assert validate([[s]])[0] == N.OK
    s["terms"].append(b"")
    assert validate([[s]]) == (N.ERR_INVALID, "highlight: query 0 field spec 0: term 1 is empty")
    s = spec(0, ["rust"], [["new", "", "york"]])
    assert validate([[s]]) == (N.ERR_INVALID, "highlight: query 0 field spec 0: a phrase holds an empty word")
    s = spec(0, ["rust"], [["new"]])
    s["phrases"].append([])
    assert validate([[s]]) == (N.ERR_INVALID, "highlight: query 0 field spec 0: phrase 1 has no words")


def out_with(**arrays):
    o = N.HlOut(struct_size=C.sizeof(N.HlOut))
    keep = np.zeros(8, np.uint32)
    for name in arrays:
        setattr(o, name, keep.ctypes.data)
    return o, keep


def test_output_struct():
    o = N.HlOut(struct_size=C.sizeof(N.HlOut) - 8)
    assert validate([[GOOD]], out=o)[0] == N.ERR_INVALID
    o, keep = out_with(status=1, offsets=1, text_offsets=1, text=1)
    assert validate([[GOOD]], out=o)[0] == N.OK
    for some in (("status",), ("status", "offsets", "text_offsets"), ("text",)):
        o, keep = out_with(**{n: 1 for n in some})
        rc, msg = validate([[GOOD]], out=o)
        assert rc == N.ERR_INVALID and "all NULL (a size query) or all given" in msg


def w(n, ch="a"):
    return ch * n


@pytest.mark.parametrize("at_limit, above, what", [
    (spec(0, [f"t{i}" for i in range(MAX_TERMS)]), spec(0, [f"t{i}" for i in range(MAX_TERMS + 1)]), "SLG_MAX_HL_TERMS"),
    (spec(0, [], [["p"]] * MAX_PHRASES), spec(0, [], [["p"]] * (MAX_PHRASES + 1)), "SLG_MAX_HL_PHRASES"),
    (spec(0, [], [["p"] * MAX_PHRASE_WORDS]), spec(0, [], [["p"], ["p"] * (MAX_PHRASE_WORDS + 1)]), "phrase 1 has more than SLG_MAX_PHRASE_TERMS"),
    (spec(0, [w(MAX_WORD)]), spec(0, [w(MAX_WORD + 1)]), "SLG_MAX_EXPAND_CHARS"),
    (spec(0, [], [["a", w(MAX_WORD)]]), spec(0, [], [["a", w(MAX_WORD + 1)]]), "SLG_MAX_EXPAND_CHARS"),
    (spec(0, ["a"], pre_tag=w(MAX_TAG)), spec(0, ["a"], pre_tag=w(MAX_TAG + 1)), "SLG_MAX_HL_TAG"),
    (spec(0, ["a"], post_tag=w(MAX_TAG)), spec(0, ["a"], post_tag=w(MAX_TAG + 1)), "SLG_MAX_HL_TAG"),
    (spec(0, ["a"], fragment_size=MAX_FRAGMENT), spec(0, ["a"], fragment_size=MAX_FRAGMENT + 1), "SLG_MAX_HL_FRAGMENT"),
    (spec(0, ["a"], number_of_fragments=MAX_FRAGMENTS), spec(0, ["a"], number_of_fragments=MAX_FRAGMENTS + 1), "SLG_MAX_HL_FRAGMENTS"),
])
def test_every_limit_at_its_value_and_one_above(at_limit, above, what):
    assert validate([[GOOD], [at_limit]])[0] == N.OK
    rc, msg = validate([[GOOD], [GOOD, above]], batch_form=True)
    assert rc == N.ERR_UNSUPPORTED and what in msg and msg.startswith("highlight: query 1 field spec 1: "), msg


def test_the_whole_table_at_every_limit_at_once():
    full = spec(4, [w(MAX_WORD, chr(65 + i % 26)) for i in range(MAX_TERMS)],
                [[w(MAX_WORD, chr(97 + (p + i) % 26)) for i in range(MAX_PHRASE_WORDS)] for p in range(MAX_PHRASES)],
                pre_tag=bytes(range(256 - MAX_TAG, 256)), post_tag=b"\0" * MAX_TAG, fragment_size=MAX_FRAGMENT,
                number_of_fragments=MAX_FRAGMENTS)
    assert validate([[full, full]])[0] == N.OK


@pytest.mark.parametrize("word", ["caf\u00e9", "new york", "a-b", "a.b", "x\0", "\u017f", "\u212a", "\u00e9", "a'"])
def test_words_outside_the_word_bytes_are_refused_not_approximated(word):
    for s in (spec(0, ["ok", word]), spec(0, ["ok"], [["ok", word]])):
        rc, msg = validate([[s]])
        assert rc == N.ERR_UNSUPPORTED and "outside [0-9A-Za-z_]" in msg and "query 0 field spec 0" in msg
    assert validate([[spec(0, ["AZaz09_"], [["_", "0"]])]])[0] == N.OK
