"""The worlds of the highlight tests (tests/test_highlight_ref.py on the host, tests/test_gpu_highlight.py on the
device): small sets of (text, field spec) cases, each chosen for one thing that can go wrong — a text length or a
doc alignment against the 16-byte lane and the 1024-byte tile, where a match lies, which alternative wins, the
fragment arithmetic, the table limits.  A world is a list of cases; `layout` puts every case's text into one
segment store as a doc of its own (pad docs in front where a case asks for an alignment), and every case becomes one
query with one hit and one spec.  Expected strings always come from tests/highlight_ref.py."""
import random

from searchlite_amd import _native as N
from searchlite_amd.highlight import highlight_spec as spec, snippet_spec

VOCAB = [b"rust", b"Rust", b"RUST", b"go", b"new", b"york", b"yorker", b"New", b"a", b"b", b"x_1", b"_", b"42", b"ust",
         b"ru", b"systems", b"language", b"z9_Z", b"ab", b"the"]
SEPS = [b" ", b" ", b" ", b", ", b"-", b"\n", b"  ", b".", b"+", b"/", b"'"]


def soup(rng, n_bytes, vocab=VOCAB, seps=SEPS):
    """Exactly n_bytes of words and separators."""
    out = b""
    while len(out) < n_bytes:
        out += rng.choice(vocab) + rng.choice(seps)
    return out[:n_bytes]


def case(text, sp, align=None, name=""):
    return dict(text=bytes(text), spec=sp, align=align, name=name)


LENGTHS = (0, 1, 15, 16, 17, 1023, 1024, 1025, 2049)
ALIGNS = (0, 1, 15, 16)


def lengths_world():
    """Every length at every alignment; a match at byte 0 and one ending at the last byte where the text has room."""
    rng = random.Random(11)
    sp = spec(0, [b"rust", b"a", b"go"], [[b"new", b"york"]], number_of_fragments=3, fragment_size=40)
    out = []
    for n in LENGTHS:
        for a in ALIGNS:
            t = bytearray(soup(rng, n))
            if n >= 6:
                t[:5] = b"rust "
                t[-3:] = b" go"
            elif n == 1:
                t[:] = b"a"
            out.append(case(t, sp, align=a, name=f"len{n}@{a}"))
    return out


def places_world():
    """A run over a lane edge (16 B) and a tile edge (1024 B), a phrase with its words in different tiles, and no match
    at all in 2049 bytes; each at doc alignments 0 and 5 (the lane and tile edges are those of the STORE's 16-byte
    lines, so both the text offset and the alignment move the match across them)."""
    out = []
    fill = lambda n: (b"qq " * (n // 3 + 1))[:n]
    for a in (0, 5):
        for at in (13, 14, 15, 16, 1021, 1022, 1023, 1024, 2040):
            t = fill(at - 1) + b" " + b"rust" + b" " + fill(30)
            out.append(case(t, spec(0, [b"rust"], fragment_size=20, number_of_fragments=2), align=a, name=f"run@{at}+{a}"))
        # the phrase: first word in tile 0, the second one or two tiles on, non-word bytes between
        for gap in (1, 1020, 2100):
            t = fill(9) + b" new" + b"." * gap + b"york " + fill(20)
            out.append(case(t, spec(0, [], [[b"new", b"york"]], fragment_size=1024, number_of_fragments=1), align=a,
                            name=f"phrase gap{gap}+{a}"))
        out.append(case(fill(2049), spec(0, [b"rust", b"q"], [[b"qq", b"q"]]), align=a, name=f"nomatch+{a}"))
    return out


def order_world():
    """Which alternative wins at a run start."""
    t = b"New York, new yorker; NEW   york new-york new york"
    out = [case(t, spec(0, terms, phrases, fragment_size=fs, number_of_fragments=nf), name=f"order{i}")
           for i, (terms, phrases) in enumerate([
               ([b"new"], [[b"new", b"york"]]),                    # a phrase and a term at the same run
               ([], [[b"new", b"york"]]),                          # `new york` against "new yorker" without the term
               ([b"york"], [[b"new"], [b"new", b"york"]]),         # two phrases sharing a first word ...
               ([b"york"], [[b"new", b"york"], [b"new"]]),         # ... in both orders
               ([b"new", b"NEW", b"new", b"york", b"york"], []),   # duplicate terms, case in the words
               ([b"YORKER"], [[b"NEW", b"YORK"]]),
               ([b"yorker", b"york"], [[b"york", b"new"], [b"new", b"yorker", b"new"]]),
           ]) for fs, nf in ((160, 1), (12, 8))]
    w = b"x_1 _ 42 x 1 _x_ 4 2 X_1 __ z9_z Z9_Z"
    out.append(case(w, spec(0, [b"x_1", b"_", b"42", b"z9_Z"], [[b"4", b"2"]], fragment_size=200, number_of_fragments=8), name="wordbytes"))
    out.append(case(w, spec(0, [b"1", b"x", b"__"], [[b"x", b"1", b"_x_"]], fragment_size=7, number_of_fragments=8), name="wordbytes2"))
    return out


def fragments_world():
    """The fragment arithmetic: every fs and nf of the list, fewer / as many / more matches than nf, the edges that
    cut words, the cut-off match, overlap, and the fullest fragment."""
    rng = random.Random(5)
    M = N.MAX_HL_FRAGMENT
    out = []
    few = b"zz rust zz zz go zz"                                      # 2 matches
    eight = b" ".join([b"rust"] * N.MAX_HL_FRAGMENTS)                # exactly SLG_MAX_HL_FRAGMENTS
    many = soup(rng, 3000)
    for fs in (0, 1, 2, 3, M - 1, M):
        for nf in (0, 1, N.MAX_HL_FRAGMENTS):
            for t in (few, eight, many):
                out.append(case(t, spec(0, [b"rust", b"go"], [], fragment_size=fs, number_of_fragments=nf), name=f"fs{fs} nf{nf}"))
    # m.start < fs / 2 and start + fs > len
    out.append(case(b"a rust b", spec(0, [b"rust"], fragment_size=100), name="both clamps"))
    out.append(case(b"q" * 300 + b" rust", spec(0, [b"rust"], fragment_size=40), name="end clamp"))
    # an edge that cuts a word into another term: "ust" from "rust" at the left edge, "ru" from "rust" at the right
    out.append(case(b"xxxxrust go", spec(0, [b"go", b"ust"], fragment_size=8), name="left cut"))      # start = 9 - 4
    out.append(case(b"go xrust rust", spec(0, [b"go", b"ru"], fragment_size=11), name="right cut"))   # "go xrust ru"
    out.append(case(b"aaaa rust", spec(0, [b"rust", b"ru"], fragment_size=4, pre_tag="[", post_tag="]"), name="own match cut"))
    out.append(case(b"aaaa language", spec(0, [b"language"], fragment_size=6), name="own match cut off entirely"))
    out.append(case(b"rust go rust go rust go", spec(0, [b"rust", b"go"], fragment_size=14, number_of_fragments=6), name="overlap"))
    dense = b"a " * (M // 2)                                          # one-byte words one byte apart
    out.append(case(dense, spec(0, [b"a"], fragment_size=M, number_of_fragments=2, pre_tag="<", post_tag=">"), name="dense"))
    out.append(case(dense, snippet_spec(0, [b"a"]), name="dense snippet"))
    return out


def limits_world():
    """The table at its limits: 32 terms, 8 phrases of SLG_MAX_PHRASE_TERMS words, a 128-byte word, 64-byte tags, an
    empty tag."""
    rng = random.Random(3)
    terms = [b"t%d" % i for i in range(N.MAX_HL_TERMS)]
    phrases = [[b"p%d" % p] + [b"w%d" % i for i in range(N.MAX_PHRASE_TERMS - 1)] for p in range(N.MAX_HL_PHRASES)]
    long_word = b"L" * N.MAX_EXPAND_CHARS
    vocab = terms + [w for p in phrases for w in p] + [long_word, long_word + b"L", b"w", b"t"]
    text = soup(rng, 4000, vocab, [b" ", b" ", b"; "])
    text += b" " + b" ".join(phrases[-1]) + b" " + long_word + b" " + terms[-1]
    tag = bytes(range(128, 128 + N.MAX_HL_TAG))  # any bytes, copied verbatim
    big = spec(0, terms + [long_word], phrases, pre_tag=tag, post_tag=b"", fragment_size=N.MAX_HL_FRAGMENT,
               number_of_fragments=N.MAX_HL_FRAGMENTS)
    big["terms"] = big["terms"][1:]  # 32 terms with the long word among them
    return [case(text, big, name="limits"),
            case(text, spec(0, [long_word], phrases[:1], pre_tag=b"", post_tag=tag[::-1], fragment_size=300, number_of_fragments=4),
                 name="limits2")]


def random_world(n_cases=300, seed=2025):
    """Random word and separator soup, random specs within the limits; at most 10 % of the docs non-ASCII."""
    rng = random.Random(seed)
    out = []
    for i in range(n_cases):
        t = bytearray(soup(rng, rng.choice((0, 3, 40, 200, 700, 1500, 2600))))
        if t and rng.random() < 0.08:
            t[rng.randrange(len(t))] = rng.choice((0x80, 0xC3, 0xFF))
        terms = [rng.choice(VOCAB) for _ in range(rng.randint(0, 5))]
        phrases = [[rng.choice(VOCAB) for _ in range(rng.randint(1, 4))] for _ in range(rng.randint(0, 3))]
        out.append(case(t, spec(0, terms, phrases, pre_tag=rng.choice(("<em>", "", "**", "<<<")), post_tag=rng.choice(("</em>", "", "**")),
                                fragment_size=rng.choice((0, 1, 5, 20, 120, 160, 1024)), number_of_fragments=rng.randint(0, 8)),
                        name=f"random{i}"))
    return out


WORLDS = dict(lengths=lengths_world, places=places_world, order=order_world, fragments=fragments_world, limits=limits_world,
              random=random_world)


def layout(cases):
    """-> (texts of the one segment, doc of each case): every case a doc of its own; a case with `align` gets a pad doc
    in front so that its first byte lies at that offset modulo 32 in the store.  The last doc ends flush with the store."""
    texts, doc_of, at = [], [], 0
    for c in cases:
        if c["align"] is not None:
            pad = (c["align"] - at) % 32
            if pad:
                texts.append(b"#" * pad)
                at += pad
        doc_of.append(len(texts))
        texts.append(c["text"])
        at += len(c["text"])
    return texts, doc_of


_PLAN = None


def plan_lib():
    """lib/libslg_plan.so: the highlighter's host side behind its test C ABI (csrc/slg_highlight_capi.cpp)."""
    global _PLAN
    if _PLAN is None:
        import ctypes as C
        from searchlite_amd import build
        _PLAN = C.CDLL(build.build_plan_lib())
    return _PLAN


def host_highlight(cases, n_threads=1):
    """The cases through the host TU's sequential highlighter (slgx_hl_reference) -> per case (status, fragments)."""
    import ctypes as C
    import numpy as np
    from searchlite_amd.highlight import pack_specs, unpack, call
    L = plan_lib()
    offs = np.zeros(len(cases) + 1, dtype=np.uint64)
    np.cumsum([len(c["text"]) for c in cases], out=offs[1:])
    blob = np.frombuffer(b"".join(c["text"] for c in cases) + b"\0", dtype=np.uint8)
    item_spec = np.arange(len(cases) + 1, dtype=np.uint32)
    _, arr, keep = pack_specs([[c["spec"] for c in cases]])
    err = C.create_string_buffer(512)

    def fn(out):
        rc = L.slgx_hl_reference(C.c_uint32(len(cases)), C.c_void_p(offs.ctypes.data), C.c_void_p(blob.ctypes.data),
                                 C.c_void_p(item_spec.ctypes.data), C.c_uint32(len(cases)), arr, C.c_uint32(n_threads),
                                 C.c_void_p(out), err, C.c_uint32(512))
        assert rc == 0, err.value
        return rc
    res = unpack([1] * len(cases), [[c["spec"]] for c in cases], *call(fn))
    return [r[0][0] for r in res]


def expected(cases):
    """Per case (status, fragments) by tests/highlight_ref.py."""
    from tests import highlight_ref as R
    return [(N.HL_HOST, []) if any(b >= 0x80 for b in c["text"]) else (N.HL_OK, R.highlight_spec_ref(c["text"], c["spec"]))
            for c in cases]
