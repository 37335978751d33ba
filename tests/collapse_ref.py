"""Field collapsing restated in plain Python (api/reader.rs:3499-3562 collapse_hits, :3578-3595 collapse_value):
the reference for tests/test_gpu_collapse.py, itself checked against hand-derived tables in
tests/test_collapse_ref.py.

Rows are a query's hits in SortKey order, (seg, doc, score).  A column is, per segment, None (the segment has no
column) or one list of ordinals per doc.  A sort is [(part, order)], part = "_score" or a field name in `fields`
(name -> (values[seg][doc] = list of numbers, is_float)), as in tests/test_gpu_sort.py.
"""
import struct

import numpy as np

from tests.test_sort_keys import pick, total_key

SCORE_DESC = [("_score", "desc")]


class MultiValued(Exception):
    """a row has more than one value in the collapse column: the reference fails the request (reader.rs:3587)"""


def score_key(x):
    b = struct.unpack("<i", struct.pack("<f", float(x)))[0]
    return b ^ ((b >> 31) & 0x7FFFFFFF)  # f32::total_cmp as a signed integer order


def part_key(part, order, seg, doc, score, fields):
    """one SortKeyPart as a tuple that orders like SortKeyPart::cmp (Missing after every value in both orders)"""
    if part == "_score":
        k = score_key(score)
        return (0, -k if order == "desc" else k)
    values, is_float = fields[part]
    v = pick(values[seg][doc], order)
    if v is None:
        return (1, 0)
    k = total_key(v, is_float)
    return (0, -k if order == "desc" else k)


def sort_key(sort, fields):
    """the full SortKey of a row under `sort`: its parts, then segment asc, doc asc (query/sort.rs:80-123)"""
    return lambda row: tuple(part_key(p, o, row[0], row[1], row[2], fields) for p, o in sort) + (row[0], row[1])


def resolve_sort(sort):
    """an empty sort is `_score` desc (query/sort.rs:159-167)"""
    return list(sort) if sort else list(SCORE_DESC)


def collapse_hits(rows, column, inner=None, main_sort=None, fields=None):
    """rows -> [(representative index, ordinal, [member indices in inner order])] in group order.
    inner: None (no inner_hits: members are discarded, as reader.rs:3554-3556) or a dict with `from` (0), `size`
    (None: all) and `sort` (a list, [] resolving to `_score` desc; or None = the request's own order, what the
    library's NULL inner_sort means).  main_sort: the request's sort (None / []: `_score` desc).
    Raises MultiValued."""
    groups, order = {}, []
    for i, (seg, doc, _score) in enumerate(rows):
        vals = [] if column[seg] is None else column[seg][doc]
        if len(vals) == 0:
            continue  # no value: in no group, nobody's inner hit
        if len(vals) > 1:
            raise MultiValued((seg, doc))
        o = int(vals[0])
        if o not in groups:
            order.append(o)
            groups[o] = []
        groups[o].append(i)
    main = resolve_sort(main_sort)
    out = []
    for o in order:
        lst = groups[o]  # (already in key order: the stable sort at :3532 changes nothing)
        top, members = lst[0], lst[1:]
        if inner is None:
            members = []
        else:
            isort = main if inner.get("sort") is None else resolve_sort(inner["sort"])
            if members and isort != main:
                key = sort_key(isort, fields)
                members = sorted(members, key=lambda i: key(rows[i]))
            frm = int(inner.get("from") or 0)
            members = members[frm:] if frm < len(members) else []
            size = inner.get("size")
            if size is not None:
                members = members[:size]
        out.append((top, o, members, len(lst)))
    return out


def expected_arrays(doc, seg, score, count, column, group_limit, inner_from=0, inner_size=0, inner_sort=None,
                    main_sort=None, fields=None):
    """The arrays of slg_batch_fetch_collapse for a batch's rows (doc, seg, score [nq, k], count [nq]), as
    PreparedBatch.collapse_groups returns them: zeros past the counts, zeros only for a query with status 1."""
    nq, G, S = len(count), int(group_limit), int(inner_size)
    u = lambda *shape: np.zeros((nq,) + shape, np.uint32)
    f = lambda *shape: np.zeros((nq,) + shape, np.float32)
    out = dict(n_groups=u(), total_groups=u(), status=u(), group_row=u(G), group_ord=u(G), group_size=u(G),
               group_doc=u(G), group_seg=u(G), group_score=f(G), inner_count=u(G), inner_row=u(G, S),
               inner_doc=u(G, S), inner_seg=u(G, S), inner_score=f(G, S))
    inner = None if S == 0 else {"from": inner_from, "size": S, "sort": inner_sort}
    for q in range(nq):
        rows = [(int(seg[q, i]), int(doc[q, i]), score[q, i]) for i in range(int(count[q]))]
        try:
            groups = collapse_hits(rows, column, inner, main_sort, fields)
        except MultiValued:
            out["status"][q] = 1
            continue
        out["total_groups"][q] = len(groups)
        out["n_groups"][q] = min(len(groups), G)
        for g, (top, o, members, size) in enumerate(groups[:G]):
            out["group_row"][q, g], out["group_ord"][q, g], out["group_size"][q, g] = top, o, size
            out["group_seg"][q, g], out["group_doc"][q, g], out["group_score"][q, g] = rows[top]
            out["inner_count"][q, g] = len(members)
            for j, i in enumerate(members):
                out["inner_row"][q, g, j] = i
                out["inner_seg"][q, g, j], out["inner_doc"][q, g, j], out["inner_score"][q, g, j] = rows[i]
    return out


def assert_same_arrays(got, want, what=""):
    """tolerance 0: integers as they are, scores as f32 bit patterns"""
    assert sorted(got) == sorted(want), what
    for name in want:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what} {name}: {a.shape} {a.dtype} != {b.shape} {b.dtype}"
        if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
            where = tuple(int(x) for x in np.argwhere(a.view(np.uint32) != b.view(np.uint32))[0])
            raise AssertionError(f"{what} {name}{list(where)}: {a[where]!r} != {b[where]!r}")
