"""The centroid update of slg_index_train_vector_field in numpy, operation by operation as include/searchlite_gpu.h
states it, and the training loop around an assignment the caller supplies.  Only the update is new arithmetic: the
assignment is slg_index_cluster_vector_field's, so the GPU tests take it from that call on a second index and this
module never scores a row against a centroid."""
import numpy as np

CHUNK = 256  # SLG_VECTOR_TRAIN_CHUNK
NOVEC = 0xFFFFFFFF


def update(rows, offsets, list_begin, docs, prev, metric):
    """C_t from the lists (list_begin, docs: docs ascending inside a list) of A_t and C_{t-1} = prev.
    rows f32 [R, dim], offsets u32 [n_docs] (row or NOVEC), metric 0 cosine / 1 L2 -> f32 [n_lists, dim]"""
    rows = np.ascontiguousarray(rows, np.float32)
    prev = np.ascontiguousarray(prev, np.float32)
    n_lists, dim = prev.shape
    out = prev.copy()
    with np.errstate(all="ignore"):
        for l in range(n_lists):
            ld = docs[int(list_begin[l]):int(list_begin[l + 1])]
            n = len(ld)
            if n == 0:
                continue
            total = np.zeros(dim, np.float64)
            for c0 in range(0, n, CHUNK):
                part = np.zeros(dim, np.float64)
                for d in ld[c0:c0 + CHUNK]:          # doc order
                    part += rows[int(offsets[int(d)])].astype(np.float64)
                total += part                        # chunk order
            m = (total / np.float64(n)).astype(np.float32)
            s = np.float64(0.0)
            for d in range(dim):                     # ascending d
                s = s + np.float64(m[d]) * np.float64(m[d])
            if not np.isfinite(s) or (metric == 0 and not s > 0.0):
                continue
            out[l] = m if metric != 0 else (m.astype(np.float64) / np.sqrt(s)).astype(np.float32)
    return out


def lists_of(row_list, offsets, n_lists):
    """(list_begin, docs) of an assignment of the rows: every doc with a vector goes to its row's list, docs ascending"""
    have = np.nonzero(np.asarray(offsets) != NOVEC)[0]
    l_of_doc = np.asarray(row_list)[np.asarray(offsets)[have]]
    order = np.argsort(l_of_doc, kind="stable")
    begin = np.concatenate([[0], np.cumsum(np.bincount(l_of_doc, minlength=n_lists))]).astype(np.uint32)
    return begin, have[order].astype(np.uint32)


def row_lists(list_begin, docs, offsets, n_rows):
    """the list of every row that some doc refers to (0xFFFFFFFF: no doc does)"""
    out = np.full(n_rows, NOVEC, np.uint32)
    for l in range(len(list_begin) - 1):
        out[np.asarray(offsets)[docs[int(list_begin[l]):int(list_begin[l + 1])]]] = l
    return out


def train(assign, rows, offsets, init, metric, iters, stop=True):
    """The loop of the header.  assign(C) -> (list_begin, docs, row_list u32 [R]): the lists of centroids C and the
    list of every row.  -> (centroids, list_begin, docs, stats) with stats = dict(iters_run, moved, empty_lists,
    max_len); stop=False runs all `iters` steps (the early stop must not change the result)."""
    cents = np.ascontiguousarray(init, np.float32).copy()
    prev_rl, iters_run, moved = None, 0, 0
    for t in range(1, iters + 1):
        begin, docs, rl = assign(cents)
        moved = len(rl) if t == 1 else int((rl != prev_rl).sum())
        if stop and t > 1 and moved == 0:
            break                                    # (lists: those of the previous step, the same)
        cents = update(rows, offsets, begin, docs, cents, metric)
        iters_run += 1
        prev_rl = rl
    else:
        begin, docs, _ = assign(cents)               # the finishing assignment is no step: `moved` stays
    lens = np.diff(begin.astype(np.int64))
    stats = dict(iters_run=iters_run, moved=moved if iters else 0, empty_lists=int((lens == 0).sum()),
                 max_len=int(lens.max()) if len(lens) else 0)
    return cents, begin, docs, stats
