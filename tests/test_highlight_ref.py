"""tests/highlight_ref.py pinned to the reference's own test and to the consequences of its loop, and the host side of
the device highlighter (csrc/slg_highlight_host.cpp through csrc/slg_highlight_capi.cpp: the packed tables and
hl_match_at of csrc/slg_highlight.hpp, the code the kernels run, one byte at a time) against it on every world of
tests/highlight_worlds.py.  Every comparison is byte equality.  No GPU."""
import os
import subprocess

import pytest

from searchlite_amd import _native as N
from searchlite_amd.highlight import highlight_spec as spec, snippet_spec
from tests import highlight_ref as R
from tests import highlight_worlds as W


# ---- the restatement --------------------------------------------------------------------------------------------
def test_the_references_own_test():
    """highlights_first_term (index/highlight.rs:86-93)"""
    snippet = R.make_snippet(b"Rust is a systems programming language", [b"systems"], [])
    assert snippet is not None and b"**systems**" in snippet
    assert snippet == b"Rust is a **systems** programming language"
    assert R.make_snippet(b"", [b"systems"], []) is None


def hl(text, terms=(), phrases=(), fs=160, nf=1, pre=b"<", post=b">"):
    return R.highlight_fragments(text, list(terms), [list(p) for p in phrases], pre, post, fs, nf)


def test_no_alternative_and_empty_ones():
    assert hl(b"rust", [], []) == [] and hl(b"rust", [b""], [[]]) == []
    assert hl(b"rust", [b"", b"rust"], [[]]) == [b"<rust>"]


def test_fragments_overlap_and_repeat_matches():
    got = hl(b"rust go rust", [b"rust", b"go"], fs=12, nf=3)
    # the matches at 0 and 5 give start 0; the one at 8 gives start 2, whose fragment begins inside the first "rust"
    assert got == [b"<rust> <go> <rust>", b"<rust> <go> <rust>", b"st <go> <rust>"]


def test_fragment_size_zero_pushes_an_empty_string_per_match():
    assert hl(b"rust go rust", [b"rust"], fs=0, nf=8) == [b"", b""]
    assert hl(b"rust go rust", [b"rust"], fs=0, nf=1) == [b""]


def test_an_edge_cuts_a_word_into_another_term():
    # "go" at 9: start = 9 - 4 = 5, the fragment "ust go" starts inside "rust": its "ust" is a word of its own there
    assert hl(b"xxxxrust go", [b"go", b"ust"], fs=8) == [b"<ust> <go>"]
    assert hl(b"xxxxrust go", [b"go", b"ust"], fs=160) == [b"xxxxrust <go>"]


def test_a_fragment_may_cut_off_its_own_match():
    assert hl(b"aaaa language", [b"language"], fs=6) == [b"aa lan"]
    assert hl(b"aaaa rust", [b"rust", b"ru"], fs=4) == [b"a <ru>"]


def test_phrase_falls_through_to_the_term():
    assert hl(b"new yorker", [b"new"], [[b"new", b"york"]]) == [b"<new> yorker"]
    assert hl(b"new yorker", [], [[b"new", b"york"]]) == []
    assert hl(b"New   York", [b"new"], [[b"new", b"york"]]) == [b"<New   York>"]


# ---- the host side of the device highlighter against it -----------------------------------------------------------
@pytest.mark.parametrize("world", sorted(W.WORLDS))
def test_host_highlighter_equals_the_restatement(world):
    cases = W.WORLDS[world]()
    want = W.expected(cases)
    got = W.host_highlight(cases, n_threads=3)
    assert len(got) == len(want)
    some = 0
    for c, g, w in zip(cases, got, want):
        assert g == w, c["name"]
        some += bool(w[1])
    assert some > 0


def test_specs_drop_empties_and_carry_the_defaults():
    s = spec(3, ["rust", ""], [[], ["new", "york"]])
    assert s["terms"] == [b"rust"] and s["phrases"] == [[b"new", b"york"]]
    assert (s["pre_tag"], s["post_tag"], s["fragment_size"], s["number_of_fragments"]) == (b"<em>", b"</em>", 160, 1)
    n = snippet_spec(3, ["rust"])
    assert (n["pre_tag"], n["post_tag"], n["fragment_size"], n["number_of_fragments"]) == (b"**", b"**", 120, 1)
    text = b"Rust is a systems programming language"
    assert W.host_highlight([W.case(text, snippet_spec(0, ["systems"]))]) == [(N.HL_OK, [R.make_snippet(text, [b"systems"], [])])]


def test_host_highlighter_marks_non_ascii_texts():
    cases = [W.case("café rust".encode(), spec(0, ["rust"])), W.case(b"cafe rust", spec(0, ["rust"]))]
    assert W.host_highlight(cases) == [(N.HL_HOST, []), (N.HL_OK, [b"cafe <em>rust</em>"])]


# ---- the host TU under the sanitizers -------------------------------------------------------------------------------
def test_host_side_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/highlight_sanitize.cpp, a stand-alone program: valid and malformed spec arrays through the validation,
    the packing and the sequential highlighter, built with -fsanitize=address,undefined"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "searchlite_amd", "csrc")
    exe = str(tmp_path / "highlight_sanitize")
    # (the sanitizers' runtimes linked into the program itself: it needs nothing from the environment it runs in)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-Wall", "-pthread", "-o", exe,
                           os.path.join(root, "tests", "cpp", "highlight_sanitize.cpp"),
                           os.path.join(csrc, "slg_highlight_host.cpp"), os.path.join(csrc, "slg_highlight_capi.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "highlight_sanitize ok" in out.stdout
