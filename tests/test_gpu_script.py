"""script_score on the device (slg_batch_prepare_script, slg_search_batch_script) through the C ABI against
tests/script_ref.py applied to the oracle's exhaustive result.  Tolerance 0, no exceptions: docs, segments, scores (bit
patterns), counts, scored_docs and matched counts are identical to the reference; rows past the count are zero.  Every
operation of the script language is a correctly rounded IEEE operation, so no world has to keep away from rounding
boundaries.  Every expected drop count is asserted on the CPU before the device is touched."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

from searchlite_amd import _native as N
from tests import fscore_ref, script_ref as R
from tests.script_worlds import KEEPS, World, one_term_queries, world_a, world_b
from tests.test_gpu_bool import csr, dead_bitmap, same
from tests.test_gpu_sort import check as check_sorted, part_key
from tests.util import random_queries, random_segment

pytestmark = pytest.mark.gpu
F32 = np.float32
KS = (1, 11, 257, 1025)

W = lambda w, **kw: dict(kind="weight", weight=w, **kw)
FVF = lambda field, **kw: dict(kind="field_value_factor", field=field, **kw)


@pytest.fixture(scope="module")
def A(oracle):
    import searchlite_amd as sa
    Wd = world_a(sa, oracle)
    yield Wd
    Wd.ix.close()


@pytest.fixture(scope="module")
def Bw(oracle):
    import searchlite_amd as sa
    Wd = world_b(sa, oracle)
    yield Wd
    Wd.ix.close()


def first_n(qs, n):
    """the first n queries of a three-term query set"""
    return qs[0][:n + 1], qs[1][:3 * n], qs[2][:3 * n]


def test_chunk_edges_of_the_compaction(Bw):
    """regions of 1, 63, 64, 65, 129 candidates (one slice each) left whole, and the 129 left with 0, 1, 63, 64, 65
    survivors by a division"""
    scored = ["c1", "c63", "c64", "c65", "c129"] + ["c129"] * 5
    left = [1, 63, 64, 65, 129, 0, 1, 63, 64, 65]
    qs = one_term_queries(Bw, scored)
    scripts = [Bw.script("_score * 2 + rank")] * 5 + [Bw.script(f"(_score + rank) / keep{m}") for m in KEEPS]
    want, sd, matched, _ = Bw.want(qs, scripts, 257)  # on the CPU first: the regions and the survivors are the case
    assert [len(Bw.lists[nm]) for nm in scored] == [1, 63, 64, 65, 129, 129, 129, 129, 129, 129]
    assert sd.tolist() == left and matched.tolist() == left
    b = Bw.ix.prepare(*qs, 11, script=scripts)
    info = b.info()
    b.close()
    assert info["n_slices"] == len(scored) and info["script_queries"] == 10 and info["script_max_depth"] == 2
    for k in (11, 257):
        got, _, _ = Bw.check(qs, scripts, k, f"chunk edges k={k}")
        assert got[3].tolist() == [min(x, k) for x in left]


@pytest.mark.parametrize("k", KS)
def test_many_slices_division_drops_all_none_every_other(Bw, k):
    """6000 candidates over several slices: a division drops all, none, every other one; a negative boost reverses
    the order (the ordered key of negative scores)"""
    T = Bw.T
    qs = csr([[(T["all"], 1.0), (int(t), 0.5)] for t in (3, 5, 7, 9)], 1)
    scripts = [Bw.script("_score / (parity - parity)"), Bw.script("_score / (parity + 1)"), Bw.script("_score / parity"),
               Bw.script("_score + parity", boost=-1.5)]
    want, sd, _, _ = Bw.want(qs, scripts, k)
    assert sd.tolist() == [0, 6000, 3000, 6000]
    b = Bw.ix.prepare(*qs, 11, script=scripts)
    assert b.info()["n_slices"] > 4
    b.close()
    got, _, _ = Bw.check(qs, scripts, k, f"many slices k={k}")
    assert got[3].tolist() == [0, k, k, k]
    assert np.all(got[0][2, :k] % 2 == 1) and np.all(got[2][3, :k] < 0) and np.all(np.diff(got[2][3, :k]) <= 0)


def test_each_op_alone(A):
    scripts = [A.script("2.5"), A.script("pop"), A.script("_score"), A.script("_score + age"), A.script("_score - age"),
               A.script("_score * pop"), A.script("_score / age"), A.script("-_score"), A.script("w", w=-0.75),
               A.script("half"), A.script("-pop", boost=2.0)]
    qs = first_n(A.qs16, len(scripts))
    want, sd, _, _ = A.want(qs, scripts, 1025)
    total = A.cands(qs, {})[3]
    assert (sd[:6] == total[:6]).all() and 0 < sd[6] < total[6]  # age is 0 for some docs: `/ age` drops them
    assert (want[2][7, :want[3][7]] < 0).all() and (want[2][0, :want[3][0]] == 2.5).all()
    A.check(qs, scripts, 1025, "each op")


def test_every_depth_and_the_longest_program(A):
    """right-nested programs of depth 1 .. 8 (the deepest touches every slot, with 7 distinct fields), a left-nested
    one of 64 instructions, and a 64-instruction one of depth 8 with every operator"""
    names = ["pop", "age", "c0", "c1", "c2", "c3", "c4"]
    right = lambda d: "_score" + "".join(f" + ({n}" for n in names[:d - 1]) + ")" * (d - 1)
    scripts = [A.script(right(d)) for d in range(1, 9)]
    long_left = dict(program=[(N.SCRIPT_PUSH_SCORE, 0)] + [x for i in range(31) for x in
                                                             ((N.SCRIPT_PUSH_CONST, 0.5 + i), (N.SCRIPT_ADD if i % 2 else N.SCRIPT_MUL, 0))]
                     + [(N.SCRIPT_NEG, 0)])
    # 8 pushes, then operators over all of them, then left-nested to 64: (((score - (pop * (age + ...))) ...
    deep = [(N.SCRIPT_PUSH_SCORE, 0)] + [(N.SCRIPT_PUSH_FIELD, A.F[n]) for n in names] + \
           [(op, 0) for op in (N.SCRIPT_ADD, N.SCRIPT_MUL, N.SCRIPT_SUB, N.SCRIPT_ADD, N.SCRIPT_MUL, N.SCRIPT_SUB, N.SCRIPT_ADD)]
    deep += [x for i in range(24) for x in ((N.SCRIPT_PUSH_FIELD, A.F[names[i % 7]]), (N.SCRIPT_SUB if i % 3 else N.SCRIPT_ADD, 0))]
    deep += [(N.SCRIPT_NEG, 0)]
    scripts += [long_left, dict(program=deep, boost=0.001)]
    assert [R.well_formed(s["program"]) for s in scripts] == [1, 2, 3, 4, 5, 6, 7, 8, 2, 8]
    assert len(long_left["program"]) == 64 and len(deep) == 64
    qs = first_n(A.qs16, len(scripts))
    want, sd, _, _ = A.want(qs, scripts, 257)
    assert (sd == A.cands(qs, {})[3]).all()  # nothing overflows here
    b = A.ix.prepare(*qs, 11, script=scripts)
    assert b.info()["script_queries"] == 10 and b.info()["script_max_depth"] == 8
    b.close()
    A.check(qs, scripts, 257, "depths")


def test_fields_pushed_again_eight_fields_and_missing_values(A):
    eight = "pop + age * c0 - c1 * c2 + c3 - c4 * half"
    scripts = [A.script("pop * pop + pop"), A.script(eight), A.script(eight + " + pop * age - half", boost=-1.0),
               A.script("half * 2 + 1"), A.script("_score / half")]
    qs = first_n(A.qs16, len(scripts))
    want, sd, _, _ = A.want(qs, scripts, 1025)
    total = A.cands(qs, {})[3]
    assert (sd[:4] == total[:4]).all() and 0 < sd[4] < total[4]  # a doc without `half` divides by 0.0
    assert (want[2][3, :want[3][3]] == 1.0).any()                # ... and has half * 2 + 1 == 1
    A.check(qs, scripts, 1025, "fields")


def test_zero_divisors_and_overflow_drops(A):
    """+0.0 and -0.0 divisors from a column, from a constant and from arithmetic; a product that overflows f64, a value
    that overflows in the f32 cast, a boost that overflows the f32 product"""
    scripts = [A.script("_score / zed"), A.script("_score / (zed * -1)"), A.script("_score / -0"), A.script("0 / zed"),
               A.script("pop * big", big=1e308), A.script("pop * big", big=1e36), A.script("pop * big", boost=1e3, big=1e35),
               A.script("pop * big", boost=-1e3, big=1e35), A.script("0 - pop * big - pop * big", big=1e308 / 1000.0)]
    qs = first_n(A.qs16, len(scripts))
    want, sd, _, _ = A.want(qs, scripts, 1025)
    total = A.cands(qs, {})[3]
    assert all(0 < sd[i] < total[i] for i in (0, 1, 3)) and sd[2] == 0
    assert all(0 < sd[i] < total[i] for i in (4, 5, 6, 7, 8)), (sd, total)
    zero = want[2][3, :want[3][3]]
    assert (zero == 0.0).all() and np.signbit(zero).any() and not np.signbit(zero).all()  # 0 / -2 is -0.0
    A.check(qs, scripts, 1025, "divisors and overflows")


@pytest.mark.parametrize("k", KS)
def test_score_alone_is_the_plain_batch_and_mixed_queries(A, k):
    """`_score` with boost 1 gives the plain batch's rows bit for bit; so does a query without a program beside
    scripted ones"""
    plain = A.ix.search_plan(*A.qs16, k)
    same(A.ix.search_batch_script(*A.qs16, k, [A.script("_score")] * 16), plain, f"_score alone k={k}")
    scripts = [A.script("_score * pop / (c0 + c1)", boost=0.5) if q % 3 == 0 else None for q in range(16)]
    got, sd, _ = A.check(A.qs16, scripts, k, f"mixed k={k}")
    for q in range(16):
        if q % 3:
            for g, p in zip(got[:3], plain[:3]):
                assert np.array_equal(g[q].view(np.uint32), p[q].view(np.uint32)), f"query {q} was touched"
            assert got[3][q] == plain[3][q]
    b = A.ix.prepare(*A.qs16, k, script=scripts)
    assert b.info()["script_queries"] == 6 and b.info()["script_max_depth"] == 3
    b.close()


def test_no_program_launches_nothing(A, oracle):
    b = A.ix.prepare(*A.qs16, 11, script=[None] * 16)
    assert b.info()["script_queries"] == 0 and b.info()["script_max_depth"] == 0
    b.run()
    same(b.fetch(), oracle.search_batch(A.segs, *A.qs16, 11, strategy=oracle.BM25), "no work")
    b.close()


def test_query_filter_on_top(A):
    qf = np.where(np.arange(16) % 2 == 0, A.flt["f0"], -1).astype(np.int32)
    scripts = [A.script("_score / zed + pop") if q % 3 else A.script("_score * age") for q in range(16)]
    got, sd, matched = A.check(A.qs16, scripts, 257, "query filter", q_filter=qf)
    plain, sd2, matched2 = A.check(A.qs16, scripts, 257, "no query filter")
    assert sd.tolist() == sd2.tolist() and (matched[0::2] < matched2[0::2]).all() and (matched[1::2] == matched2[1::2]).all()


def test_field_sort_with_matched_counts(A):
    rng = np.random.default_rng(41)
    vals = [[[int(rng.integers(0, 8))] for _ in range(s.n_docs)] for s in A.segs]
    fields = {"low": (vals, False)}
    fid = A.ix.add_sort_field(vals, np.int64)
    try:
        scripts = [A.script("_score * pop / zed" if q % 2 else "_score + c0 * age", boost=(-1.0 if q % 5 == 0 else 1.0))
                   for q in range(16)]
        _, sd, matched, rows = A.want(A.qs16, scripts, 1)
        assert (sd[1::2] < A.cands(A.qs16, {})[3][1::2]).all()  # `/ zed` drops docs
        for order in ("asc", "desc"):
            sort = [("low", order), ("_score", "desc")]
            want = [sorted(hits, key=lambda h: tuple(part_key(p, o, h[0], h[1], h[2], fields) for p, o in sort) + (h[0], h[1]))
                    for hits in rows]
            for k in (11, 257):
                got = A.ix.search_batch_script(*A.qs16, k, scripts, sort=[(fid, order), ("_score", "desc")])
                check_sorted(got, want, k, sort, f"sorted {order} k={k}")
                assert got[4].tolist() == matched.tolist()
    finally:
        A.ix.remove_sort_field(fid)


def test_plans_and_the_many_term_kernel(A):
    """a flat DisMax plan, and 12 scored lists (the many-term kernel)"""
    nq = 16
    scripts = [A.script("_score * (1 + pop / 10) + age * w", w=0.001) if q % 2 else A.script("(_score - c0) / zed")
               for q in range(nq)]
    flat = dict(q_leaf=np.tile([0, 0, 1], nq), q_plan=np.full(nq, 1, np.int32), q_tie=np.full(nq, 0.3, F32))
    A.check(A.qs16, scripts, 257, "flat DisMax", **flat)
    if not hasattr(A, "qs12"):
        A.qs12 = random_queries(np.random.default_rng(51), 6, 12, 40, n_segs=2, weights=True)
    for k in (11, 1025):
        A.check(A.qs12, scripts[:6], k, f"12 lists k={k}")


@pytest.mark.parametrize("order", ["outer", "inner"])
def test_both_chain_orders(A, order):
    """script_score{query: function_score} (outer) and function_score{query: script_score} (inner): the second stage
    reads the first one's score, a doc dropped by the first stays dropped, and the second drops docs of its own.  The
    expected result is fscore_ref and script_ref composed on the CPU"""
    pop, f0 = A.F["pop"], A.flt["f0"]
    fs = dict(functions=[FVF(pop, modifier="sqrt", missing=1.0), W(2.0, filter=f0)], score_mode="sum", boost_mode="sum",
              min_score=12.0, boost=0.5)
    fscore = [fs if q % 4 != 3 else None for q in range(16)]
    scripts = [A.script("_score * 2 / zed", boost=1.5) if q % 4 != 2 else None for q in range(16)]
    want, sd, _, _ = A.want(A.qs16, scripts, 257, fscore=fscore, order=order)
    # on the CPU first: what each stage drops alone, and that the chain is not just one of them
    untouched = [None] * 16
    sd_script = A.want(A.qs16, scripts, 257)[1]
    sd_fscore = A.want(A.qs16, untouched, 257, fscore=fscore)[1]
    total = A.cands(A.qs16, {})[3]
    first, second = (sd_fscore, sd_script) if order == "outer" else (sd_script, sd_fscore)
    for q in (0, 1, 4):
        assert first[q] < total[q], "the inner stage drops nothing"
        assert sd[q] < first[q], "no doc is dropped only by the outer stage"
        assert sd[q] > 0
    other = A.want(A.qs16, scripts, 257, fscore=fscore, order="inner" if order == "outer" else "outer")
    assert not np.array_equal(other[0][2], want[2]), "the two orders give the same scores: the case shows nothing"
    assert sd[2] == sd_fscore[2] and sd[3] == sd_script[3]  # queries with one stage only
    A.check(A.qs16, scripts, 257, f"chain {order}", fscore=fscore, order=order)
    b = A.ix.prepare(*A.qs16, 11, script=scripts, fscore=fscore, script_order=order)
    info = b.info()
    b.close()
    assert info["script_queries"] == 12 and info["fscore_queries"] == 12 and info["fscore_kernel"] == "lean"


def test_chain_at_the_chunk_edges(Bw):
    """both stages compact the same regions one after the other: 129 candidates left with 65 by the first stage and
    with 63, 1 and 0 by the second"""
    qs = one_term_queries(Bw, ["c129"] * 6)
    rank = Bw.F["rank"]
    fs65 = dict(functions=[FVF(rank)], boost_mode="replace", min_score=64.0)   # ranks 64 .. 128
    for order in ("outer", "inner"):
        if order == "outer":  # function_score first (65 left), then the script
            scripts = [Bw.script(f"(_score + 1) / keep{m}") for m in (63, 1, 0)] + [Bw.script("_score")] * 3
            fscore = [fs65] * 3 + [fs65, None, dict(min_score=1e9)]
            left = [63, 1, 0, 65, 129, 0]
        else:                 # the script first (65 left), then function_score on its value, the rank
            scripts = [Bw.script("rank / keep65")] * 4 + [None, Bw.script("rank / keep0")]
            fscore = [dict(min_score=float(129 - m)) for m in (63, 1, 0)] + [None, None, dict(min_score=-1.0)]
            left = [63, 1, 0, 65, 129, 0]
        want, sd, matched, _ = Bw.want(qs, scripts, 257, fscore=fscore, order=order)
        assert sd.tolist() == left and matched.tolist() == left, (order, sd)
        Bw.check(qs, scripts, 257, f"chain edges {order}", fscore=fscore, order=order)


def test_run_twice_and_batches_in_flight(A, Bw):
    """slg_batch_run twice on one batch gives the same rows (the scoring kernel rewrites the regions the stages
    consumed); two batches in flight on their own streams"""
    import torch
    k = 257
    scripts = [A.script("_score * pop / zed", boost=0.5)] * 16
    fscore = [dict(functions=[W(3.0, filter=A.flt["f1"])], boost_mode="sum", min_score=3.5)] * 16
    want, sd, _, _ = A.want(A.qs16, scripts, k, fscore=fscore, order="inner")
    b = A.ix.prepare(*A.qs16, k, script=scripts, fscore=fscore, script_order="inner")
    for _ in range(2):
        b.run()
        got = b.fetch(want_stats=True)
        same(got[:4], want, "run again")
        assert [int(got[4][q].scored_docs) for q in range(16)] == sd.tolist()
    b.close()
    T = Bw.T
    qs = csr([[(T["all"], 1.0), (int(t), 0.5)] for t in (3, 5)], 1)
    specs = [[Bw.script("_score / parity"), Bw.script("_score + rank")],
             [Bw.script("rank - _score", boost=-1.0), Bw.script("_score / (1 - parity)")]]
    wants = [Bw.want(qs, s, k)[0] for s in specs]
    streams = [torch.cuda.Stream() for _ in specs]
    batches = [Bw.ix.prepare(*qs, k, script=s) for s in specs]
    for bb, s in zip(batches, streams):
        bb.set_stream(s.cuda_stream)
    for _ in range(3):
        for bb in batches:
            bb.run()
    for bb, w in zip(batches, wants):
        same(bb.fetch(), w, "in flight")
        bb.close()


def test_batch_keeps_its_index_state(oracle):
    """a batch prepared before slg_index_update_deleted answers against the state it was prepared on"""
    import searchlite_amd as sa
    rng = np.random.default_rng(13)
    segs = [random_segment(rng, 300, 30, 6), random_segment(rng, 200, 30, 6)]
    qs = random_queries(rng, 8, 3, 30, n_segs=2)
    old = [copy.copy(s) for s in segs]
    Wd = World(sa, oracle, segs, tuning={"updatable": 1})
    try:
        Wd.add_field("v", [[[float(rng.integers(0, 4))] for _ in range(s.n_docs)] for s in segs], np.float64)
        scripts = [Wd.script("_score / v + v")] * 8
        chains = Wd.chains(scripts)
        want_old = R.apply(fscore_ref.all_candidates(oracle, old, *qs), old, chains, fscore_ref.Columns(old, Wd.cols.fields), 33)[0]
        b = Wd.ix.prepare(*qs, 33, script=scripts)
        bm = dead_bitmap(rng, 300, 0.3)
        Wd.ix.update_deleted(0, bm, 300.0 - float(np.unpackbits(bm, bitorder="little")[:300].sum()))
        b.run()
        same(b.fetch(), want_old, "prepared before the update")
        b.close()
        new = Wd.ix.segments
        want_new = R.apply(fscore_ref.all_candidates(oracle, new, *qs), new, chains, fscore_ref.Columns(new, Wd.cols.fields), 33)[0]
        same(Wd.ix.search_batch_script(*qs, 33, scripts), want_new, "prepared after the update")
    finally:
        Wd.ix.close()


def test_one_call_form_and_refusals(A):
    """slg_search_batch_script = prepare + run + fetch; a script batch does not run sharded; ids are checked against
    the batch's index state; programs the device does not run are unsupported; the other batch kinds take no spec"""
    from searchlite_amd import searcher
    from searchlite_amd.script import script_spec
    k = 11
    scripts = [A.script("_score * pop / zed", boost=2.0)] * 16
    fscore = [dict(functions=[W(2.0, filter=A.flt["f0"])], boost_mode="sum", min_score=2.5)] * 16
    sspec, keep = script_spec(scripts, 16)
    fspec, keep2 = searcher.fscore_spec(fscore, 16)
    o, t, w = (np.ascontiguousarray(a) for a in A.qs16)
    for fs, order in ((None, "outer"), (fspec, "outer"), (fspec, "inner")):
        outs = [np.zeros((16, k), dt) for dt in (np.uint32, np.uint32, F32)] + [np.zeros(16, np.uint32)]
        stats = (N.Stats * 16)()
        N.check(A.ix._lib.slg_search_batch_script(A.ix._h, 16, o.ctypes.data, t.ctypes.data, w.ctypes.data, None, None, None,
                                                  C.addressof(sspec), None if fs is None else C.addressof(fs),
                                                  N.SCRIPT_INNER if order == "inner" else N.SCRIPT_OUTER, k, 1,
                                                  *[a.ctypes.data for a in outs], C.addressof(stats), None))
        want, sd, _, _ = A.want(A.qs16, scripts, k, fscore=None if fs is None else fscore, order=order)
        same(tuple(outs), want, f"one call {order}")
        assert [int(s.scored_docs) for s in stats] == sd.tolist()
    b = A.ix.prepare(*A.qs16, k, script=scripts)
    try:
        group = searcher.ShardGroup(A.ix, 0, 1, searcher.shard_unique_id(), 2)
        try:
            for call in (lambda: b.run_sharded(group), b.fetch_sharded):
                with pytest.raises(N.SlgError) as ei:
                    call()
                assert ei.value.code == N.ERR_UNSUPPORTED
        finally:
            group.close()
        with pytest.raises(N.SlgError):  # score order: no matched counts
            b.run()
            b.matched_counts()
    finally:
        b.close()
    plain = A.ix.prepare(*A.qs16, k)
    try:
        with pytest.raises(N.SlgError) as ei:
            plain.is_script = True
            plain.info()
        assert ei.value.code == N.ERR_INVALID  # slg_batch_script_info: not a script batch
    finally:
        plain.is_script = False
        plain.close()
    kw = A.ix.add_agg_keyword_field([[[0]] * s.n_docs for s in A.segs], 1)
    nonfin = A.ix.add_agg_field([[[math.inf]] * s.n_docs for s in A.segs], np.float64)
    push = lambda f: [(N.SCRIPT_PUSH_SCORE, 0), (N.SCRIPT_PUSH_FIELD, f), (N.SCRIPT_ADD, 0)]
    const = lambda v: [(N.SCRIPT_PUSH_SCORE, 0), (N.SCRIPT_PUSH_CONST, v), (N.SCRIPT_MUL, 0)]
    try:
        for program, code, word in ((push(12345), N.ERR_INVALID, "unknown agg field"), (push(kw), N.ERR_INVALID, "keyword"),
                                    (push(nonfin), N.ERR_UNSUPPORTED, "non-finite"),
                                    (const(math.inf), N.ERR_UNSUPPORTED, "non-finite constant"),
                                    (const(1.0)[:2], N.ERR_UNSUPPORTED, "ill-formed"),
                                    ([(N.SCRIPT_PUSH_CONST, 1.0)] * 9 + [(N.SCRIPT_ADD, 0)] * 8, N.ERR_UNSUPPORTED, "SLG_MAX_SCRIPT_DEPTH"),
                                    (const(1.0) * 22, N.ERR_UNSUPPORTED, "SLG_MAX_SCRIPT_INSTRS"),
                                    ([(9, 0)], N.ERR_INVALID, "unknown script op")):
            with pytest.raises(N.SlgError) as ei:
                A.ix.prepare(*A.qs16, k, script=[program] * 16)
            assert ei.value.code == code and word in ei.value.msg, (program, ei.value.msg)
        for boost in (math.inf, math.nan):
            with pytest.raises(N.SlgError) as ei:
                A.ix.prepare(*A.qs16, k, script=[dict(program=const(1.0), boost=boost)] * 16)
            assert ei.value.code == N.ERR_INVALID and "q_boost" in ei.value.msg
        with pytest.raises(N.SlgError) as ei:
            A.ix.prepare(*A.qs16, k, script=scripts, script_order=2)
        assert ei.value.code == N.ERR_INVALID and "order" in ei.value.msg
        with pytest.raises(N.SlgError) as ei:  # the fscore stage's ids are checked as in its own batch
            A.ix.prepare(*A.qs16, k, script=scripts, fscore=[dict(functions=[FVF(12345)])] * 16)
        assert ei.value.code == N.ERR_INVALID and "unknown agg field" in ei.value.msg
    finally:
        A.ix.remove_agg_field(kw)
        A.ix.remove_agg_field(nonfin)
    from tests import bool_ref
    for other in (dict(hybrid=True), dict(cursors=[None] * 16), dict(clauses=bool_ref.clauses_of([([], 0)] * 16, 2)),
                  dict(rescore=dict(q_offsets=np.zeros(17, np.uint32), q_terms=np.zeros((0, 2), np.uint32),
                                    q_weights=np.zeros(0, F32), window=4)),
                  dict(collapse=dict(field=kw, group_limit=1))):
        with pytest.raises(N.SlgError) as ei:
            A.ix.prepare(*A.qs16, k, script=scripts, **other)
        assert ei.value.code == N.ERR_UNSUPPORTED
