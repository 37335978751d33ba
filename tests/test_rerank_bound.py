"""The float64 rerank reference and its error bound (tests.util.rerank_exact / check_rerank_result), on
the CPU: the oracle's left-to-right f32 rerank stays inside the bound on the cases the GPU rerank tests
use, the multi-segment oracle (combined ids) agrees with a direct per-segment f32 restatement, and
references broken on purpose — a ragged 1030-d row missing its last element, two clauses' boosts
swapped, cosine's missing score on an L2 field — are rejected, so the bound is tight enough to catch a
subtly wrong kernel."""
import numpy as np
import pytest

from tests.test_gpu_rerank_widths import PATHS, _fields, _field, _kind, _l2_identity, _queries, _truncated
from tests.util import F32_MIN, check_rerank_result, oracle_rerank_segments, rerank_row


def _f32_reference(fields, q, kind, k_out, drop_last=False, swap_boost=False, cosine_missing=False):
    """compute_hybrid_score (api/reader.rs:225-254) restated per (seg, doc) in f32, sums left to right,
    with optional mistakes.  -> (doc, seg, score, vec, count) of the top k_out."""
    f32 = np.float32
    nc = len(q["cf"])
    boost = np.ones(nc, f32) if q.get("boost") is None else np.asarray(q["boost"], f32).copy()
    if swap_boost:
        boost[[0, 1]] = boost[[1, 0]]
    rows = []
    with np.errstate(all="ignore"):
        for sg, doc, bm in zip(q["seg"], q["doc"], np.asarray(q["bm"], f32)):
            bsum, vsum, has = f32(0), f32(0), False
            for c in range(nc):
                f = fields[q["cf"][c]]
                row = rerank_row(f, int(sg), int(doc))
                if row is None:
                    vs = f32(-1.0) if f["metric"] == 0 or cosine_missing else f32(F32_MIN)
                else:
                    x, y = np.asarray(row, f32), np.asarray(q["qv"][c], f32)
                    if drop_last:
                        x, y = x[:-1], y[:-1]
                    if f["metric"] == 0:
                        sm = np.add.accumulate((y * x).astype(f32), dtype=f32)[-1]
                        sim = f32(0) if np.isnan(sm) else sm
                    else:
                        d = (y - x).astype(f32)
                        sim = -np.sqrt(np.add.accumulate((d * d).astype(f32), dtype=f32)[-1], dtype=f32)
                    vs = sim if kind == "one" else f32(sim * boost[c])
                    vsum = f32(vsum + vs)
                    has = True
                a = f32(q["alpha"][c])
                bl = bm if a >= 1 else vs if a <= 0 else f32(f32(a * bm) + f32(f32(f32(1) - a) * vs))
                bsum = f32(bsum + bl)
            score = bsum if kind == "one" else f32(bsum / f32(nc))
            m0 = f32(-1.0) if fields[q["cf"][0]]["metric"] == 0 else f32(F32_MIN)
            b = int(np.array(score, f32).view(np.int32))
            key = b ^ 0x7FFFFFFF if b < 0 else b
            rows.append((-key, int(sg), int(doc), score, vsum if has else m0))
    rows.sort(key=lambda r: r[:3])
    rows = rows[:k_out]
    return (np.array([r[2] for r in rows], np.uint32), np.array([r[1] for r in rows], np.uint32),
            np.array([r[3] for r in rows], f32), np.array([r[4] for r in rows], f32), len(rows))


def _oracle_got(oracle, fields, q, kind, k_out):
    d, s, sc, v = oracle_rerank_segments(oracle, fields, q, kind, k_out)
    return d, s, np.asarray(sc, np.float32), np.asarray(v, np.float32), len(d)


@pytest.mark.parametrize("path", list(PATHS))
def test_oracle_inside_the_bound(oracle, path):
    """oracle.rerank / rerank_multi / rerank_fields (left-to-right f32) on the real-data queries of the GPU
    width matrix (mixed alphas, counts around k_out and max_cand) and at alpha 0 lie inside the float64
    bound."""
    kind = _kind(path)
    fields = _fields(path, "real")
    for k_out in (1, 65, 1024):
        rng = np.random.default_rng(k_out)
        max_cand = k_out + 40
        for mode in ("mixed", "zero"):
            for i, q in enumerate(_queries(rng, path, fields, [k_out - 1, k_out + 1, max_cand], max_cand, mode,
                                           "real")):
                q = _truncated(q)
                check_rerank_result(fields, q, kind, k_out, _oracle_got(oracle, fields, q, kind, k_out),
                                    _l2_identity(path), f"{path} k_out {k_out} {mode} query {i}")


@pytest.mark.parametrize("path", ["one-rows1-cos", "one-generic-dim102-l2", "multi-mfma-cos", "fields-fast-slow"])
@pytest.mark.parametrize("metric", [0, 1], ids=["cos", "l2"])
def test_oracle_across_segments(oracle, path, metric):
    """oracle_rerank_segments (one store, combined ids seg * N + doc) equals the per-segment f32 restatement
    bit for bit on integer vectors: docs past n_docs, segments >= n_segs and a segment without the field
    are candidates without a vector, scored with the field's metric; ties order by (seg, doc)."""
    kind, cl = PATHS[path]
    rng = np.random.default_rng(metric)
    dims = {}
    for f, dim, m in cl:
        dims[f] = (dim, metric if f == 0 else m)
    vl = (1,) if kind != "multi" else ()
    fields = [_field(rng, *dims[f], "int", vectorless=vl if f == 0 else ()) for f in sorted(dims)]
    for mode in ("zero", "mixed", "one"):
        for q in _queries(rng, path, fields, [300, 17], 300, mode, "int"):
            q = _truncated(q)
            want = _f32_reference(fields, q, kind, 100)
            got = _oracle_got(oracle, fields, q, kind, 100)
            assert got[4] == want[4]
            for a, b in zip(got[:4], want[:4]):
                assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)), mode
            check_rerank_result(fields, q, kind, 100, got, False, f"{path} {mode}")


MUTANTS = {
    "drop-last-element": ("one-generic-dim1030-cos", dict(drop_last=True)),
    "swap-boosts": ("multi-streaming-cos", dict(swap_boost=True)),
    "cosine-missing-on-l2": ("one-rows2-l2", dict(cosine_missing=True)),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_bound_rejects_mutants(mutant):
    """The checker accepts the correct f32 restatement and rejects each broken one."""
    path, bug = MUTANTS[mutant]
    kind = _kind(path)
    fields = _fields(path, "real")
    rng = np.random.default_rng(8)
    qs = [_truncated(q) for q in _queries(rng, path, fields, [300, 300], 300, "zero", "real")]
    for q in qs:
        if q.get("boost") is not None:
            q["boost"] = np.array([0.5, 2.0], np.float32)
    for q in qs:
        check_rerank_result(fields, q, kind, 250, _f32_reference(fields, q, kind, 250), _l2_identity(path), mutant)
    rejected = 0
    for q in qs:
        try:
            check_rerank_result(fields, q, kind, 250, _f32_reference(fields, q, kind, 250, **bug),
                                _l2_identity(path), mutant)
        except AssertionError:
            rejected += 1
    assert rejected == len(qs), f"{mutant}: {len(qs) - rejected} queries accepted"
