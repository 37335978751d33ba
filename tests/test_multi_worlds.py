"""CPU proof that the worlds of tests/multi_worlds.py reach the edges of score_multi_kernel they are named for.

Every world is planned with the plan library (lib/libslg_plan.so, the planner the device uses) under its tuning and a
champion table built as the device builds it (stage_ref.lane_table over stage_ref.impacts_np); tests/multi_model.py
then restates the kernel's chunk loop over that plan, and a predicate per edge name looks for the edge in the trace.
tests/test_gpu_multi_edges.py repeats the same on the plan the device reports, then runs the batch."""
import ctypes as C

import numpy as np
import pytest

from tests import multi_model as M
from tests import multi_worlds as MW
from tests import stage_ref
from tests.test_plan import RQ, TR, Planned, _family_plans, default_tuning

MAX_PLAN_DEPTH = 4     # SLG_MAX_PLAN_DEPTH


def plan_lib():
    from searchlite_amd import build
    L = C.CDLL(build.build_plan_lib())
    L.slgp_plan.restype = C.c_void_p
    L.slgp_plan.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32, C.c_char_p,
                            C.c_uint32, C.c_void_p]
    L.slgp_facts_of.argtypes = [C.c_void_p, C.c_void_p]
    L.slgp_bytes.restype = C.c_uint64
    L.slgp_bytes.argtypes = [C.c_void_p, C.c_int]
    L.slgp_copy.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.slgp_free.argtypes = [C.c_void_p]
    return L


@pytest.fixture(scope="module")
def lib():
    return plan_lib()


def lane_champions(seg):
    """the champion table the device stages for a segment without deleted docs"""
    imps = stage_ref.impacts_np(seg)
    offs = np.asarray(seg.term_offsets, dtype=np.int64)
    return np.stack([stage_ref.lane_table(imps[offs[t]:offs[t + 1]]) for t in range(seg.n_terms)])


class WorldPlan:
    """A world planned at (k, strategy): the planner's arrays, the model's trace over them, the counters it predicts.
    q_filter / filter_live: a doc filter per query, as Planned takes it; multi_trace False: the arrays alone (the worlds
    of the few-term kernel, which tests/fewterm_model.py traces)."""

    def __init__(self, lib, W, k, strategy, tuning=None, champs=None, q_filter=None, filter_live=b"", multi_trace=True):
        tune = tuning if tuning is not None else default_tuning(**W.tuning)
        champs = champs if champs is not None else [lane_champions(s) for s in W.segs]
        p = Planned(lib, W.segs, W.offs, W.terms, W.w, k, strategy=strategy, tuning=tune,
                    plans=_family_plans(W.plans), champs=champs, q_filter=q_filter, filter_live=filter_live)
        assert p.h, (W.name, p.err)
        self.W, self.k, self.strategy = W, k, strategy
        self.facts = p.facts
        self.sqs, self.terms = p.array(0, RQ).copy(), p.array(1, TR).copy()
        self.q_postings = p.array(7, "<u8").copy()
        p.close()
        self.nq = len(W.offs) - 1
        self.block_skip = bool(self.facts.pruned and self.facts.multi and tune.block_max)
        if not multi_trace:
            return
        self.traced = M.trace(W.segs, self.sqs, self.terms, self.block_skip)
        self.scored, self.skipped = M.counters(self.sqs, self.traced, self.nq)

    def chunks(self):
        """(sub-query, round, chunk number, record) of every chunk"""
        for i, _, _, per_round in self.traced:
            for r, recs in enumerate(per_round):
                for n, c in enumerate(recs):
                    yield i, r, n, c

    def real(self):
        return [x for x in self.chunks() if not x[3]["no_essential"]]

    def n_terms(self, i):
        return int(self.sqs[i]["n_terms"])

    def leaf_lists(self, i):
        tt = self.terms[int(self.sqs[i]["term_begin"]):int(self.sqs[i]["term_begin"]) + self.n_terms(i)]
        return [int(x) for x in tt["leaf"]], [float(x) for x in tt["weight"]]


def _slots(P, pred):
    return any(pred(c, s) for _, _, _, c in P.real() for s in c["slots"])


def _idle_leaves(P, leaves):
    """a chunk after a round's first, in which every list of `leaves` has no live posting while another list has"""
    for i, _, n, c in P.real():
        leaf, _ = P.leaf_lists(i)
        mine = [t for t in range(len(leaf)) if leaf[t] in leaves]
        if n >= 1 and mine and all(c["live"][t] == 0 for t in mine) and sum(c["live"]) > 0:
            return True
    return False


def _empty_list_at(P, where):
    for i, _, _, c in P.real():
        T = P.n_terms(i)
        t = {"first": 0, "middle": T // 2 - 1, "last": T - 1}[where]
        if c["rem"][t] == 0 and (where != "middle" or (c["rem"][:t].sum() and c["rem"][t + 1:].sum())):
            return True
    return False


def _ess_before(P):
    """a probed list ahead of every essential list in term order, with a doc the essential bitmap has and one it lacks"""
    for i, bounds, _, per_round in P.traced:
        ess = int(P.sqs[i]["ess_mask"])
        if ess & 1:
            continue
        tt = P.terms[int(P.sqs[i]["term_begin"]):int(P.sqs[i]["term_begin"]) + P.n_terms(i)]
        docs0 = M.lists_of(P.W.segs[int(P.sqs[i]["seg"])], [int(tt["term"][0])])[0]
        for recs in per_round:
            for c in recs:
                if c["no_essential"] or not c["live"][0]:
                    continue
                mine = docs0[(docs0 >= c["dlo"]) & (docs0 < c["dhi"])]
                hit = np.isin(mine, c["edocs"])
                if hit.any() and (~hit).any():
                    return True
    return False


def _first_bit(c, s):
    return s["kind"] == "whole" and s["hits"] == 1 and s["fd"] in c["edocs"] and (s["fd"] - c["wbase"]) % 32 == 0


def _last_bit(c, s):
    return s["kind"] == "whole" and s["hits"] == 1 and s["ld"] in c["edocs"] and s["ld"] - c["wbase"] == M.SPAN - 1


EDGES = {
    # accumulators
    "R_ess==512 uncut, 512 docs": lambda P: any(c["R_ess"] == 512 and not c["cut"] and c["ndocs"] == 512 for *_, c in P.real()),
    "R_ess==513 cut, a list clamped to 1, a list cut inside a slot": lambda P: any(
        c["R_ess"] == 513 and c["by_acc"] and any(c["rem"][t] == 1 and c["chunk"][t] == 1 for t in range(len(c["rem"])))
        and any(c["chunk"][t] < c["rem"][t] and c["chunk"][t] % 64 for t in range(len(c["rem"]))) for *_, c in P.real()),
    "a cut round of >= 3 chunks": lambda P: any(len(recs) >= 3 and recs[0]["by_acc"] for _, _, _, pr in P.traced for recs in pr),
    "ndocs==1": lambda P: any(c["ndocs"] == 1 for *_, c in P.real()),
    # slots and batches
    "S==8": lambda P: any(c["S"] == 8 for *_, c in P.real()),
    "S==9": lambda P: any(c["S"] == 9 for *_, c in P.real()),
    "S==16": lambda P: any(c["S"] == 16 for *_, c in P.real()),
    "S==17": lambda P: any(c["S"] == 17 for *_, c in P.real()),
    "nb_a==1": lambda P: any(c["nb_a"] == 1 for *_, c in P.real()),
    "nb_a==2": lambda P: any(c["nb_a"] == 2 for *_, c in P.real()),
    "nb_a==3": lambda P: any(c["nb_a"] == 3 for *_, c in P.real()),
    "nb_a==4": lambda P: any(c["nb_a"] == 4 for *_, c in P.real()),
    "a list with 64 postings in a round": lambda P: any(n == 0 and 64 in c["rem"] for _, _, n, c in P.real()),
    "a list with 65 postings in a round": lambda P: any(n == 0 and 65 in c["rem"] for _, _, n, c in P.real()),
    "first list empty in a round": lambda P: _empty_list_at(P, "first"),
    "middle list empty in a round": lambda P: _empty_list_at(P, "middle"),
    "last list empty in a round": lambda P: _empty_list_at(P, "last"),
    "T==32, one posting per list": lambda P: any(len(c["rem"]) == 32 and (c["rem"] == 1).all() for *_, c in P.real()),
    "T==5 classified": lambda P: P.facts.pruned and any(P.n_terms(i) == 5 and int(P.sqs[i]["skip_mask"]) for i in range(len(P.sqs))),
    "T==9": lambda P: any(P.n_terms(i) == 9 for i in range(len(P.sqs))),
    "T==32": lambda P: any(P.n_terms(i) == 32 for i in range(len(P.sqs))),
    # window
    "dhi-wbase==16384 uncut": lambda P: any(c["dhi"] - c["wbase"] == M.SPAN and not c["cut"] for *_, c in P.real()),
    "dhi-wbase==16385": lambda P: any(c["rdhi"] - c["wbase"] == M.SPAN + 1 and c["by_window"] and c["dlo"] % 32 == 0
                                      for *_, c in P.real()),
    "rdhi-dlo<=16384 but dlo%32!=0 cuts": lambda P: any(c["rdhi"] - c["dlo"] <= M.SPAN and c["dlo"] % 32 and c["by_window"]
                                                         for *_, c in P.real()),
    "docs at window bits 0, 31, 32, 16383": lambda P: any(
        {0, 31, 32, M.SPAN - 1} <= set((c["edocs"] - c["wbase"]).tolist()) for *_, c in P.real()),
    "a chunk cut by the accumulator rule and the window": lambda P: any(c["by_acc"] and c["by_window"] for *_, c in P.real()),
    "next chunk several empty windows on": lambda P: any(
        recs[n]["by_window"] and not recs[n + 1]["no_essential"] and recs[n + 1]["wbase"] - recs[n]["dhi"] >= 3 * M.SPAN
        for _, _, _, pr in P.traced for recs in pr for n in range(len(recs) - 1)),
    # MaxScore and block skipping
    "no essential posting left in a round": lambda P: any(c["no_essential"] and c["n_skipped"] > 0 for *_, c in P.chunks()),
    "S_all in 61..63 with share>=1: marked cut, nothing cut off": lambda P: any(
        61 <= c["S_all"] <= 63 and c["share"] >= 1 and c["cut"] and (c["consumed"] == c["rem"]).all() for *_, c in P.real()),
    "the slot rule alone lowers share": lambda P: any(c["by_slots"] and not c["by_acc"] and c["share"] < 1 and
                                                      (c["chunk"] < c["rem"]).any() for *_, c in P.real()),
    "a probed slot past the cut": lambda P: _slots(P, lambda c, s: s["kind"] == "past"),
    "a whole probed slot with 0 hits": lambda P: _slots(P, lambda c, s: s["kind"] == "whole" and s["hits"] == 0),
    "a whole slot whose only hit is its first doc, at a bit with x&31==0": lambda P: _slots(P, _first_bit),
    "a whole slot whose only hit is its last doc, the window's last": lambda P: _slots(P, _last_bit),
    "a straddling slot is kept": lambda P: _slots(P, lambda c, s: s["kind"] == "straddling" and not s["skipped"]),
    "a skipped slot among the first 8": lambda P: any(not c["first8_same"] and c["kept"] > 0 for *_, c in P.real()),
    "skipped slots only behind the first 8": lambda P: any(c["first8_same"] and c["kept"] < c["S"] for *_, c in P.real()),
    "nb drops": lambda P: any(c["nb_after"] < c["nb"] for *_, c in P.real()),
    "a skipped whole slot under a cut": lambda P: any(
        c["cut"] and any(s["skipped"] and s["kind"] == "whole" for s in c["slots"]) for *_, c in P.real()),
    "a non-essential list before the essential one, docs present and absent": _ess_before,
    # plans
    "MODE 2": lambda P: P.facts.multi and P.facts.plan_batch and not P.facts.nested and not P.facts.deep and
    {int(x) & 0xFF for x in P.sqs["plan"]} == {1, 2} and any(float(x) > 0 for x in P.sqs["tie"]),
    "MODE 3": lambda P: P.facts.multi and P.facts.plan_batch and P.facts.nested and not P.facts.deep and
    all(int(x) >= 2 for x in P.sqs["n_groups"]),
    "MODE 4": lambda P: P.facts.multi and P.facts.plan_batch and P.facts.deep and
    all(int(x) == MAX_PLAN_DEPTH for x in P.sqs["depth"]),
    "a negative weight": lambda P: any(w < 0 for i in range(len(P.sqs)) for w in P.leaf_lists(i)[1]),
    "an idle leaf in a round's later chunk": lambda P: _idle_leaves(P, {3}),
    "an idle group": lambda P: _idle_leaves(P, {3, 4}),
    "an idle node": lambda P: _idle_leaves(P, {3, 4}),
    # slices and segments
    "n_rounds not a multiple of rounds_per_slice": lambda P: any(int(s["n_rounds"]) % int(s["rounds_per_slice"]) for s in P.sqs),
    ">= 3 slices": lambda P: any(int(s["n_slices"]) >= 3 for s in P.sqs),
    "two segments, a term absent from one": lambda P: len(P.W.segs) == 2 and len(P.sqs) == 2 * P.nq and
    len({P.n_terms(i) for i in range(len(P.sqs))}) == 2,
}

# every edge named above must stay promised by a world: dropping it from a world's list fails the suite
REQUIRED = set(EDGES)


def check_edges(P):
    """every edge the world promises at (strategy, k) is in the trace"""
    W = P.W
    promised = P.k in W.edge_ks and P.strategy in W.edges
    if promised or W.always_multi:
        assert P.facts.multi == 1, f"world {W.name}: k={P.k} strategy={P.strategy}: not on the many-term kernel"
    if not promised:
        return
    for name in W.edges.get(P.strategy, ()):
        assert EDGES[name](P), f"world {W.name}: k={P.k} strategy={P.strategy}: edge not reached: {name}"


def check_model(P):
    """the model against itself: a round's chunks consume exactly the round's range of every list"""
    for i, bounds, _, per_round in P.traced:
        for r, recs in enumerate(per_round):
            got = sum((c["consumed"] for c in recs), np.zeros(bounds.shape[1], dtype=np.int64))
            assert (got == bounds[r + 1] - bounds[r]).all(), f"world {P.W.name}: sub-query {i} round {r}: {got} consumed"
        assert (bounds[-1] == [int(x) for x in P.terms[int(P.sqs[i]["term_begin"]):][:bounds.shape[1]]["df"]]).all()


@pytest.mark.parametrize("world", MW.WORLDS, ids=lambda f: f.__name__)
def test_world_reaches_its_edges(lib, world):
    W = world()
    for strategy in sorted(set(W.strategies) | {MW.BM25}):
        for k in MW.ALL_KS:
            P = WorldPlan(lib, W, k, strategy)
            check_edges(P)
            check_model(P)
            if W.n_rounds is not None and k in W.edge_ks and strategy in W.edges:
                assert [int(s["n_rounds"]) for s in P.sqs[:len(W.segs)]] == W.n_rounds, (W.name, k, strategy)


@pytest.mark.parametrize("world", MW.WORLDS, ids=lambda f: f.__name__)
def test_exhaustive_run_scores_every_doc_once(lib, world):
    """Bm25 classifies nothing: the chunks' docs add up to the distinct docs of each query's lists, per segment"""
    W = world()
    P = WorldPlan(lib, W, 11, MW.BM25)
    assert not P.facts.pruned and (P.skipped == 0).all()
    check_model(P)
    for q in range(P.nq):
        want = 0
        for s, seg in enumerate(W.segs):
            ids = [int(t) for t in W.terms[int(W.offs[q]):int(W.offs[q + 1]), s] if t != MW.NO_TERM]
            want += len(np.unique(np.concatenate(M.lists_of(seg, ids))))
        assert int(P.scored[q]) == want, f"world {W.name}: query {q}"


def test_every_listed_edge_is_promised_by_a_world():
    promised = {name for w in MW.WORLDS for names in w().edges.values() for name in names}
    assert promised <= set(EDGES), promised - set(EDGES)
    assert REQUIRED <= promised, f"edges no world promises: {sorted(REQUIRED - promised)}"


def test_round_without_an_essential_posting_cannot_be_planned(lib):
    """A planned round always holds a posting of the splitter, which is essential (n_rounds <= its df, and boundary j
    lies at its posting j * stride): the kernel's `R_ess == 0` exit is reachable only after a cut, for the rest of a
    round.  That is the form the worlds promise ("no essential posting left in a round")."""
    for world in MW.WORLDS:
        W = world()
        for strategy in W.strategies:
            P = WorldPlan(lib, W, 1, strategy)
            for i, bounds, _, per_round in P.traced:
                sq = P.sqs[i]
                lg = int(sq["longest"])
                assert (int(sq["ess_mask"]) >> lg) & 1
                assert int(sq["n_rounds"]) <= int(bounds[-1][lg])
                for r, recs in enumerate(per_round):
                    if bounds[r + 1].sum() > bounds[r].sum():
                        assert bounds[r + 1][lg] > bounds[r][lg] and not recs[0]["no_essential"]
