"""Highlighting on the device (slg_highlight_batch / slg_batch_highlight; index/highlight.rs).

A field spec is a dict from highlight_spec() / snippet_spec(): the text field id of GpuIndex.add_text_field, the
FINAL term and phrase word lists (the caller has run the analysis of highlight_terms per field and
normalize_phrase_terms), the two tags, fragment_size and number_of_fragments.  Empty terms and empty phrases are
dropped here, as the reference skips them; what the device does not build is refused with SlgError(ERR_UNSUPPORTED)
— the CPU path — by the library, never approximated.

Results come back per query, per hit, per field spec as (status, [fragment bytes]): N.HL_OK, N.HL_HOST (the text
holds a byte >= 0x80: highlight this one on the CPU) or N.HL_NO_TEXT (the hit's segment has no store for the field).
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as N


def _bytes(x) -> bytes:
    return x.encode("utf-8") if isinstance(x, str) else bytes(x)


def highlight_spec(text_field: int, terms: Sequence = (), phrases: Sequence[Sequence] = (), pre_tag="<em>",
                   post_tag="</em>", fragment_size: int = 160, number_of_fragments: int = 1) -> dict:
    """One field of SearchRequest.highlight (HighlightOptions' defaults: <em>, </em>, 160, 1).  Empty terms and
    phrases without words are dropped (highlight.rs:22-38); an empty word inside a phrase stays and is refused by the
    library (the reference would build `\\W+\\W+` from it)."""
    return dict(text_field=int(text_field), terms=[_bytes(t) for t in terms if len(t)],
                phrases=[[_bytes(w) for w in p] for p in phrases if len(p)], pre_tag=_bytes(pre_tag),
                post_tag=_bytes(post_tag), fragment_size=int(fragment_size), number_of_fragments=int(number_of_fragments))


def snippet_spec(text_field: int, terms: Sequence = (), phrases: Sequence[Sequence] = ()) -> dict:
    """SearchRequest.highlight_field: make_snippet's "**", "**", 120, 1 (highlight.rs:67-80); the snippet is the
    item's last (only) fragment, None when it has none."""
    return highlight_spec(text_field, terms, phrases, "**", "**", 120, 1)


def pack_specs(specs_per_query: Sequence[Sequence[dict]]):
    """-> (spec_offsets u32[nq + 1], N.HlSpec array, keep): the arrays of a highlight call."""
    nq = len(specs_per_query)
    offs = np.zeros(nq + 1, dtype=np.uint32)
    np.cumsum([len(s) for s in specs_per_query], out=offs[1:])
    arr = (N.HlSpec * max(int(offs[nq]), 1))()
    keep = []
    i = 0
    for specs in specs_per_query:
        for sp in specs:
            words = list(sp["terms"]) + [w for p in sp["phrases"] for w in p]
            woffs = np.zeros(len(words) + 1, dtype=np.uint32)
            np.cumsum([len(w) for w in words], out=woffs[1:])
            poffs = np.zeros(len(sp["phrases"]) + 1, dtype=np.uint32)
            np.cumsum([len(p) for p in sp["phrases"]], out=poffs[1:])
            blob = np.frombuffer(b"".join(words) + b"\0", dtype=np.uint8)  # (one spare byte: never an empty array)
            pre = np.frombuffer(sp["pre_tag"] + b"\0", dtype=np.uint8)
            post = np.frombuffer(sp["post_tag"] + b"\0", dtype=np.uint8)
            keep += [woffs, poffs, blob, pre, post]
            arr[i] = N.HlSpec(C.sizeof(N.HlSpec), sp["text_field"], len(sp["terms"]), len(sp["phrases"]),
                              poffs.ctypes.data, woffs.ctypes.data, blob.ctypes.data, pre.ctypes.data, post.ctypes.data,
                              len(sp["pre_tag"]), len(sp["post_tag"]), sp["fragment_size"], sp["number_of_fragments"])
            i += 1
    return offs, arr, keep


def call(fn) -> Tuple[np.ndarray, np.ndarray, np.ndarray, bytes]:
    """fn(address of an N.HlOut) -> rc, twice: the size query, then the call with arrays of exactly that size.
    -> (status u8[n_items], offsets u32[n_items + 1], text_offsets u32[n_frags + 1], text)."""
    out = N.HlOut(struct_size=C.sizeof(N.HlOut))
    N.check(fn(C.addressof(out)))
    n_items, n_frags, n_bytes = int(out.n_items), int(out.n_frags), int(out.text_bytes)
    status = np.zeros(max(n_items, 1), dtype=np.uint8)
    offsets = np.zeros(n_items + 1, dtype=np.uint32)
    toffs = np.zeros(n_frags + 1, dtype=np.uint32)
    text = np.zeros(max(n_bytes, 1), dtype=np.uint8)
    out = N.HlOut(C.sizeof(N.HlOut), n_items, n_frags, n_bytes, status.ctypes.data, offsets.ctypes.data,
                  toffs.ctypes.data, text.ctypes.data, 0, 0, 0)
    N.check(fn(C.addressof(out)))
    n_items, n_frags = int(out.n_items), int(out.n_frags)
    return status[:n_items], offsets[:n_items + 1], toffs[:n_frags + 1], text[:int(out.text_bytes)].tobytes()


def unpack(rows_per_query: Sequence[int], specs_per_query, status, offsets, toffs, text) -> List[List[List[Tuple[int, List[bytes]]]]]:
    """The flat arrays of a call as result[q][hit][spec] = (status, [fragment bytes])."""
    res, item = [], 0
    for q, rows in enumerate(rows_per_query):
        hits = []
        for _ in range(int(rows)):
            per_spec = []
            for _ in specs_per_query[q]:
                frags = [text[int(toffs[f]):int(toffs[f + 1])] for f in range(int(offsets[item]), int(offsets[item + 1]))]
                per_spec.append((int(status[item]), frags))
                item += 1
            hits.append(per_spec)
        res.append(hits)
    assert item == len(status)
    return res


def highlight_hits(lib, index_handle, hits_per_query, specs_per_query):
    """slg_highlight_batch over host hits: hits_per_query[q] = [(seg, doc), ...]."""
    nq = len(hits_per_query)
    assert len(specs_per_query) == nq
    hoffs = np.zeros(nq + 1, dtype=np.uint32)
    np.cumsum([len(h) for h in hits_per_query], out=hoffs[1:])
    flat = [hd for h in hits_per_query for hd in h]
    seg = np.array([s for s, _ in flat] + [0], dtype=np.uint32)
    doc = np.array([d for _, d in flat] + [0], dtype=np.uint32)
    soffs, arr, keep = pack_specs(specs_per_query)
    flat_out = call(lambda out: lib.slg_highlight_batch(index_handle, nq, hoffs.ctypes.data, seg.ctypes.data,
                                                        doc.ctypes.data, soffs.ctypes.data, arr, out))
    del keep
    return unpack([len(h) for h in hits_per_query], specs_per_query, *flat_out)


def highlight_batch(lib, batch_handle, count: Optional[np.ndarray], specs_per_query):
    """slg_batch_highlight over a finished batch's own rows; count: its fetched counts (the result's shape)."""
    soffs, arr, keep = pack_specs(specs_per_query)
    flat_out = call(lambda out: lib.slg_batch_highlight(batch_handle, soffs.ctypes.data, arr, out))
    del keep
    return unpack([int(c) for c in count], specs_per_query, *flat_out)
