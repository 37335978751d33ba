"""CPU proof that the worlds of tests/fewterm_worlds.py reach the edges of score_uniform4_kernel they are named for.

Every world is planned with the plan library (tests/test_multi_worlds.py: plan_lib, WorldPlan) under its tuning, at
every k it names and every strategy; tests/fewterm_model.py then restates the kernel's cuts, lanes, chunks, filter and
queue over that plan, and a predicate per edge name looks for the edge in the trace, by exact count.
tests/test_gpu_fewterm_edges.py repeats the same on the plan the device reports, then runs the batch.

Three edges of the issue's list cannot be formed and are stated as what can:
  * "bound + 1 equal to the round's end": the list that sets a chunk's bound keeps a later posting of the round, whose
    doc lies between bound + 1 and the round's end, so bound + 1 < end in every cut chunk (asserted below);
  * "8 * mlanes >= rem for every list" under need > 64: then sum(ceil(rem / 8)) <= sum(mlanes) <= 64; the chunk that is
    the rest of its round is the one with need <= 64, and that is the edge promised;
  * "one receiver block" of the binary-search join: that join starts at 65 entries = two blocks."""
import numpy as np
import pytest

from tests import fewterm_model as F
from tests import fewterm_worlds as FW
from tests.test_multi_worlds import WorldPlan, plan_lib

DOC_END = F.DOC_END


@pytest.fixture(scope="module")
def lib():
    return plan_lib()


_traces = {}


class FewPlan:
    """A world planned at (k, strategy) and traced by the model; filter_id: the id its doc filter got"""

    def __init__(self, lib, W, k, strategy, tuning=None, champs=None, filter_id=0):
        qf, live = None, b""
        if W.masks is not None:
            qf, live = np.full(W.nq, filter_id, dtype=np.int32), bytes([0] * filter_id + [1])
        if champs is None and not W.tuning.get("champions", 1):     # an index without champions: no seed
            champs = [np.zeros((s.n_terms, 68), dtype=np.float32) for s in W.segs]
        P = WorldPlan(lib, W, k, strategy, tuning=tuning, champs=champs, q_filter=qf, filter_live=live, multi_trace=False)
        self.W, self.k, self.strategy, self.facts = W, k, strategy, P.facts
        self.sqs, self.terms, self.q_postings, self.nq = P.sqs, P.terms, P.q_postings, P.nq
        key = (W.name, self.sqs[["seg", "term_begin", "n_terms", "n_rounds", "rounds_per_slice", "longest"]].tobytes(),
               self.terms[["off", "df", "term"]].tobytes())
        if key not in _traces:       # (the structure does not depend on k or the strategy: traced once)
            _traces[key] = F.trace(W.segs, self.sqs, self.terms, W.ml)
        self.traced = _traces[key]
        self.docs, self.postings = F.counters(W.segs, self.traced, self.nq)

    def tt(self, sub):
        b = int(self.sqs[sub["i"]]["term_begin"])
        return self.terms[b:b + sub["T"]]

    def lists(self, sub):
        return F.lists_of(self.W.segs[sub["seg"]], sub["terms"])

    def slices(self):
        return [(sub, sl) for sub in self.traced for sl in sub["slices"]]

    def rounds(self):
        return [(sub, sl, r, rd) for sub, sl in self.slices() for r, rd in enumerate(sl["rounds"])]

    def waves(self):
        return [(sub, sl, r, rd, n, w) for sub, sl, r, rd in self.rounds() for n, w in enumerate(rd["waves"])]

    def chunks(self):
        return [(sub, sl, r, rd, n, c) for sub, sl, r, rd in self.rounds() for n, c in enumerate(rd["chunks"])]

    def cut_chunks(self):
        return [x for x in self.chunks() if x[5]["need"] > F.LANES]


# ---- predicates ------------------------------------------------------------------------------------------------
def _slice_of(n):
    return lambda P: any(sl["n_r"] == n for _, sl in P.slices())


def _row(T, ml):
    return lambda P: P.W.ml == ml and P.facts.max_terms <= (4 if ml == 4 else 8) and any(sub["T"] == T for sub in P.traced)


def _row_full(words):
    return lambda P: F.cut_words(P.W.ml) == words and any((sl["n_r"] + 1) * sub["T"] == words and (sub["T"] > 4) == (words == 128)
                                                           for sub, sl in P.slices())


def _trailing_empty(P):
    return any(sl["n_r"] >= 2 and sl["r0"] + sl["n_r"] == sub["n_rounds"] and sl["rounds"][-1]["lanes"]["total"] == 0 and
               sl["rend"][-2] == DOC_END and sl["rounds"][-2]["lanes"]["total"] > 0 for sub, sl in P.slices())


def _list_in_slice(where):
    def pred(P):
        for sub, sl in P.slices():
            df = [int(x) for x in P.tt(sub)["df"]]
            for t in range(sub["T"]):
                lo, hi = int(sl["b"][0, t]), int(sl["b"][-1, t])
                if lo == hi and {"none": True, "before": lo == df[t], "behind": hi == 0}[where] and sub["T"] > 1:
                    if where == "none" or sl["rounds"][0]["lanes"]["total"] > 0:
                        return True
        return False
    return pred


def _boundary_doc_everywhere(P):
    for sub in P.traced:
        L = P.lists(sub)
        if sub["T"] < 2:
            continue
        for j in range(1, sub["n_rounds"]):
            pos = int(sub["b"][j, sub["longest"]])
            if pos >= len(L[sub["longest"]]):
                continue
            doc = int(L[sub["longest"]][pos])
            if all(int(sub["b"][j, t]) < len(L[t]) and int(L[t][sub["b"][j, t]]) == doc for t in range(sub["T"])):
                return True   # the cut of every list points AT the doc: it belongs to the later round in all of them
    return False


def _path(name):
    return lambda P: any(sl["n_r"] >= F.TWO_PHASE_MIN and name in sl["paths"].values() for _, sl in P.slices())


def _coincide(P):
    return any(sl["n_r"] >= F.TWO_PHASE_MIN and sub["T"] > 1 and (sl["b"][0] == sl["b"][-1]).any() for sub, sl in P.slices())


def _lanes(n):
    """64 lanes: one planned wave; 65: streamed in chunks"""
    return lambda P: any(rd["lanes"]["total"] == n and len(rd["chunks"]) >= 2 if n > 64 else
                         rd["lanes"]["total"] == n and not rd["chunks"] and len(rd["waves"]) == 1 for *_, rd in P.rounds())


def _empty_between(P):
    for *_, rd in P.rounds():
        c, fb = rd["lanes"]["c"], rd["lanes"]["first_bytes"]
        for t in range(1, len(c) - 1):
            if c[t] == 0 and c[:t].sum() and c[t + 1:].sum() and fb[t] == fb[t + 1]:
                return True
    return False


def _both_words(P):
    return any(len(rd["lanes"]["c"]) == 8 and (rd["lanes"]["c"][5:] > 0).any() and (rd["lanes"]["c"][1:5] > 0).any()
               for *_, rd in P.rounds())


def _clamped(P):
    return any(rd["lanes"]["c"].sum() >= 2040 and rd["lanes"]["hdr_lanes"] == 255 and rd["lanes"]["total"] > 255 and
               rd["lanes"]["first_bytes"].max() == 127 and rd["lanes"]["first"].max() > 127 for *_, rd in P.rounds())


def _one_finishes(P):
    return any(((c["rem"] > 0) & (c["consumed"] == c["rem"])).any() and (c["consumed"] < c["rem"]).any()
               for *_, c in P.cut_chunks())


def _nne_falls(P):
    return any(a["nne"] > b["nne"] for *_, rd in P.rounds() for a, b in zip(rd["chunks"], rd["chunks"][1:]))


def _share_zero(P):
    return any(((c["rem"] > 0) & (c["share"] < 1) & (c["mlanes"] == 1)).any() for *_, c in P.cut_chunks())


def _rest_of_round(P):
    return any(n >= 1 and c["need"] <= F.LANES and c["bound"] == DOC_END and (c["chunk"] == c["rem"]).all() and
               c["end"] == rd["end"] for _, _, _, rd, n, c in P.chunks())


def _bound_doc(offset):
    def pred(P):
        for sub, _, _, _, _, c in P.cut_chunks():
            if c["bound"] != DOC_END and c["end"] == c["bound"] + 1 and \
                    all(c["bound"] + offset in set(x.tolist()) for x in P.lists(sub)):
                return True     # (end = bound + 1: the bound doc is this chunk's in every list, the one above the next's)
        return False
    return pred


def _overfull_at(where):
    return lambda P: any(rd["lanes"]["overfull"] and r == (0 if where == "first" else sl["n_r"] - 1) and sl["n_r"] > 1
                         for _, sl, r, rd in P.rounds())


def _queued(w, doc, lst):
    hit = (w["qdoc"] == doc) & (w["qlst"] == lst)
    return bool(hit.any()), bool(w["partner"][hit].any()) if hit.any() else False


def _loaded(w, doc, lst):
    return bool(((w["doc"] == doc) & (w["lst"] == lst)).any())


def _alias_edges():
    def alias(P):
        m = P.W.marks
        return any(_queued(w, m["d1"], 0) == (True, False) and _queued(w, m["d1"] + m["Pd"], 1) == (True, False)
                   for *_, w in P.waves())

    def partners(P):
        m = P.W.marks
        return any(_queued(w, m["d2"], 0) == (True, True) and _queued(w, m["d2"], 1) == (True, True) and
                   _queued(w, m["d2"] + m["Pd"], 2) == (True, False) for *_, w in P.waves())

    def neighbours(P):
        m = P.W.marks
        return any(_loaded(w, m["d3"], 0) and _loaded(w, m["d3"] + 1024, 1) and not _queued(w, m["d3"], 0)[0] and
                   not _queued(w, m["d3"] + 1024, 1)[0] for *_, w in P.waves())

    def tail(P):
        m = P.W.marks
        for *_, w in P.waves():
            at = (w["doc"] == m["tail"]) & (w["lst"] == 1)
            if at.any() and not w["mine"][at].any() and m["tail"] >= w["end"] and _queued(w, m["d4"], 0) == (True, False):
                return True
        return False

    def same_list(P):
        m = P.W.marks
        return any(_loaded(w, m["d5"], 0) and _loaded(w, m["d5"] + m["Pd"], 0) and not _queued(w, m["d5"], 0)[0] and
                   not _queued(w, m["d5"] + m["Pd"], 0)[0] for *_, w in P.waves())

    names = ["an alias at doc + period is queued without a partner",
             "partners in A and B with an alias in C: the join sums A and B only",
             "doc and doc + 1024: neighbouring fields, no interaction",
             "an alias with a posting behind the round's end in a lane's tail",
             "two postings of one list that alias each other are not queued"]
    out = {}
    for name, fn in zip(names, [alias, partners, neighbours, tail, same_list]):
        out[name] = lambda P, fn=fn: P.W.ml == 4 and F.period(4) == P.W.marks["Pd"] and fn(P)
        out[name + " (8 list bits)"] = lambda P, fn=fn: P.W.ml == 8 and F.period(8) == P.W.marks["Pd"] and fn(P)
    return out


def _queue(n):
    return lambda P: any(w["n"] == n for *_, w in P.waves())


def _blocks(n):
    return lambda P: any(w["n"] > F.JOIN_PAIRS and -(-w["n"] // 64) == n for *_, w in P.waves())


def _doc_in_lists(w, T, want):
    """a queued doc held by exactly the lists `want`"""
    by_doc = {}
    for d, t in zip(w["qdoc"].tolist(), w["qlst"].tolist()):
        by_doc.setdefault(d, set()).add(t)
    return any(v == want for v in by_doc.values())


def _all_lists(P):
    return any(sub["T"] >= 3 and _doc_in_lists(w, sub["T"], set(range(sub["T"]))) for sub, *_, w in P.waves())


def _first_last(P):
    return any(sub["T"] >= 3 and _doc_in_lists(w, sub["T"], {0, sub["T"] - 1}) for sub, *_, w in P.waves())


def _dense_gap(P):
    for *_, w in P.waves():
        s = w["seg_len"]
        if w["n"] > F.JOIN_PAIRS and any(s[t] == 0 and s[:t].sum() and s[t + 1:].sum() for t in range(1, len(s) - 1)):
            return True
    return False


def _longest_segment(n):
    return lambda P: any(w["n"] > F.JOIN_PAIRS and w["seg_len"].max() == n for *_, w in P.waves())


def _sentinel_alias(P):
    for sub, _, _, _, _, w in P.waves():
        pad = (w["doc"] == DOC_END) & ~w["mine"]
        if w["n"] == 1 and pad.any() and F.field_key(int(w["qdoc"][0]), P.W.ml) == F.field_key(DOC_END, P.W.ml) and \
                int(w["qlst"][0]) not in set(w["lst"][pad].tolist()):
            return True
    return False


def _pad_overlay(P):
    """the 4-bit instance's filter after a wave's loads: a word behind the queue, where the all-pairs join's last group
    reads an entry's doc, equals a queued doc, and the word beside it (the entry's score) is not zero"""
    for *_, w in P.waves():
        n = w["n"]
        if P.W.ml != 4 or not 0 < n <= F.JOIN_PAIRS or n % 8 == 0:
            continue
        flt = np.zeros(F.FILTER_WORDS, dtype=np.int64)
        real = w["doc"] != DOC_END
        np.bitwise_or.at(flt, w["doc"][real] % F.FILTER_WORDS, 1 << (w["lst"][real] + 4 * ((w["doc"][real] // F.FILTER_WORDS) % 8)))
        if any(int(flt[2 * p]) in set(w["qdoc"].tolist()) and flt[2 * p + 1] for p in range(n, (n + 7) & ~7)):
            return True
    return False


def _q72(P):
    return any(sub["T"] == 8 and w["n"] == 72 and (w["seg_len"] > 0).all() for sub, *_, w in P.waves())


# plans: query q of PLANS8, its sub-query in segment 0
def _plan_sub(P, q):
    return [sub for sub in P.traced if sub["q"] == q and sub["seg"] == 0][0]


def _both_joins(P, q):
    ns = [w["n"] for sub, *_, w in P.waves() if sub is _plan_sub(P, q)]
    return any(0 < n <= F.JOIN_PAIRS for n in ns) and any(n > F.JOIN_PAIRS for n in ns)


def _plan_is(q, kind, pred=lambda leaf, sq: True):
    def check(P):
        sub = _plan_sub(P, q)
        sq = P.sqs[sub["i"]]
        leaf = [int(x) for x in P.tt(sub)["leaf"]]
        return P.facts.uniform and P.facts.plan_batch and int(sq["plan"]) & 0xFF == kind and _both_joins(P, q) and pred(leaf, sq)
    return check


def _idle_leaf(P):
    for sub, _, _, rd in P.rounds():
        if int(P.sqs[sub["i"]]["plan"]) & 0xFF == 0 or sub["seg"] != 0:
            continue
        leaf = np.array([int(x) for x in P.tt(sub)["leaf"]])
        c = rd["lanes"]["c"]
        if any(c[leaf == lf].sum() == 0 for lf in set(leaf.tolist())) and c.sum():
            return True
    return False


def _min_match(second_leaf):
    def check(P):
        for sub, *_, w in P.waves():
            sq = P.sqs[sub["i"]]
            if int(sq["plan"]) >> 8 != 2 or float(sq["theta0"]) != 0.0:
                continue
            leaf = [int(x) for x in P.tt(sub)["leaf"]]
            want = {0, 1, 2} if second_leaf else {0, 1}
            if leaf[0] == leaf[1] != leaf[2] and _doc_in_lists(w, sub["T"], want):
                return True
        return False
    return check


def _negative_weight(P):
    return any(int(P.sqs[sub["i"]]["plan"]) & 0xFF and (P.tt(sub)["weight"] < 0).any() for sub in P.traced)


def _absent_leaf(P):
    for q in range(P.nq):
        subs = [sub for sub in P.traced if sub["q"] == q]
        if len(subs) == 2 and subs[0]["T"] != subs[1]["T"]:
            short = min(subs, key=lambda s: s["T"])
            sq = P.sqs[short["i"]]
            if float(sq["max_init"]) == 0.0 and int(sq["plan"]) & 0xFF == 2 and len(set(P.tt(short)["leaf"].tolist())) < int(sq["n_leaves"]):
                return True
    return False


def _scores(P, sub):
    """f32 weight * impact of every posting of a sub-query's lists, as the kernel settles them"""
    from tests import stage_ref
    seg = P.W.segs[sub["seg"]]
    imp = stage_ref.impacts_np(seg)
    offs = np.asarray(seg.term_offsets, dtype=np.int64)
    return [(imp[offs[t]:offs[t + 1]] * np.float32(w)).astype(np.float32) for t, w in zip(sub["terms"], P.tt(sub)["weight"])]


def _tie_after_compaction(P):
    """The first round of a slice without a seed, replayed as the kernel takes it: the singles register by register into
    the top-k buffer of 64 * (KREGS + 1) entries, which compacts to the k best when the next register's singles do not
    fit; then a queued entry that no other list holds (its sum is its own score) has exactly the score bits of the
    compacted threshold and a lower doc id."""
    if P.k > 256:
        return False
    cap = 64 * (next(r for r in (1, 2, 4) if 64 * r >= P.k) + 1)
    for sub, sl in P.slices():
        rd = sl["rounds"][0]
        if float(P.sqs[sub["i"]]["theta0"]) != 0.0 or rd["chunks"]:
            continue
        w, sc = rd["waves"][0], _scores(P, sub)
        bits = np.array([int(sc[t][p:p + 1].view(np.uint32)[0]) if m else 0 for t, p, m in zip(w["lst"], w["pos"], w["mine"])])
        single = w["mine"] & (w["doc"] < w["end"]) & (w["x"] == 0)
        held, th = [], None
        for jj in range(F.NS):
            at = np.nonzero(single & (np.arange(len(single)) % F.NS == jj))[0]
            cand = [(-int(bits[a]), int(w["doc"][a])) for a in at]
            if len(held) + len(cand) > cap:
                held = sorted(held)[:P.k]
                th = held[P.k - 1] if len(held) >= P.k else th
            held += [c for c in cand if th is None or c < th]
        if th is None:
            continue
        for a in np.nonzero(w["queued"])[0]:
            alone = int((w["qdoc"] == w["doc"][a]).sum()) == 1
            if alone and -int(bits[a]) == th[0] and int(w["doc"][a]) < th[1]:
                return True
    return False


def _ulp_singles(P):
    """the seed theta0 of the plan has the bits of one list's weighted impact; another list's lie one below"""
    sub = P.traced[0]
    th = int(np.float32(P.sqs[0]["theta0"]).view(np.uint32))
    sc = _scores(P, sub)
    L = P.lists(sub)
    shared = set(L[0].tolist()) & set(L[1].tolist())
    return th > 0 and not shared and th in set(sc[0].view(np.uint32).tolist()) and th - 1 in set(sc[1].view(np.uint32).tolist())


# threshold: the oracle's exhaustive rows at the world's full k show every doc's score
_rows = {}


def _all_scores(W):
    if W.name not in _rows:
        from oracle import oracle as o
        o.build()
        doc, _, score, count = o.search_batch(W.segs, W.offs, W.terms, W.w, W.full_k(), strategy=o.BM25)
        assert int(count[0]) == W.distinct_docs()[0]
        _rows[W.name] = doc[0], score[0].view(np.uint32)
    return _rows[W.name]


def _tied(P, lists_held):
    """at rank k docs with identical score bits lie on both sides; lists_held(n): what the tied docs must include"""
    doc, bits = _all_scores(P.W)
    k = P.k
    if not (k < len(bits) and bits[k - 1] == bits[k]):
        return False
    held = [sum(int(d) in set(x.tolist()) for x in P.W.query_lists(0, 0)) for d in doc[bits == bits[k]]]
    return any(lists_held(n) for n in held) and bool((np.diff(doc[bits == bits[k]].astype(np.int64)) > 0).all())


EDGES = {
    # cuts
    "a slice of 1 round": _slice_of(1), "a slice of 8 rounds": _slice_of(8), "a slice of 9 rounds": _slice_of(9),
    "a slice of 16 rounds": _slice_of(16),
    "a last slice shorter than the others": lambda P: any(len(sub["slices"]) > 1 and sub["slices"][-1]["n_r"] < sub["slices"][0]["n_r"]
                                                          for sub in P.traced),
    "T==1 on the 64-word row": _row(1, 4), "T==3 on the 64-word row": _row(3, 4), "T==4 on the 64-word row": _row(4, 4),
    "T==5 on the 128-word row": _row(5, 8), "T==8 on the 128-word row": _row(8, 8),
    "(rounds+1)*T==64": _row_full(64), "(rounds+1)*T==128": _row_full(128),
    "a trailing round that is empty": _trailing_empty,
    "a list with no posting inside a slice": _list_in_slice("none"),
    "a list wholly before a slice's first boundary": _list_in_slice("before"),
    "a list wholly behind a slice's last boundary": _list_in_slice("behind"),
    "a boundary doc that sits in every list": _boundary_doc_everywhere,
    "two-phase: the window holds the cut": _path("window"),
    "two-phase: the window misses and the bisection runs": _path("bisect"),
    "two-phase: first and last cut coincide": _coincide,
    # lanes
    "a round of exactly 64 lanes": _lanes(64), "a round of exactly 65 lanes": _lanes(65),
    "c==0,1,7,8,9 in one round": lambda P: any({0, 1, 7, 8, 9} <= set(rd["lanes"]["c"].tolist()) for *_, rd in P.rounds()),
    "an empty list between two non-empty ones": _empty_between,
    "both header words carry boundaries": _both_words,
    "a round of >= 2040 postings: lane count clamps at 255, a first lane at 127": _clamped,
    "rows of rounds 8.. replace those of rounds 0..7": lambda P: any(
        sl["n_r"] >= 9 and sl["rounds"][7]["lanes"]["total"] > 0 and sl["rounds"][8]["lanes"]["total"] > 0 for _, sl in P.slices()),
    "the global guess misses: its bracket widens and bisects": lambda P: any(
        "guess-bisect" in sl["paths"].values() for _, sl in P.slices()),
    # chunks
    "need==65": lambda P: any(c["need"] == 65 for *_, c in P.chunks()),
    "a chunk in which one list finishes and the others do not": _one_finishes,
    "nne falls between the chunks of a round": _nne_falls,
    "a share that rounds to zero extra lanes": _share_zero,
    "a chunk that is the rest of the round": _rest_of_round,
    "a doc held by all lists is its chunk's bound doc": _bound_doc(0),
    "a doc held by all lists one above the bound": _bound_doc(1),
    "an over-full round is a slice's last": _overfull_at("last"),
    "an over-full round is a slice's first": _overfull_at("first"),
    "an over-full round at k=257": lambda P: P.k == 257 and P.facts.cand_mode == 1 and
    any(rd["lanes"]["overfull"] for *_, rd in P.rounds()),
    # filter aliases
    **_alias_edges(),
    # join
    **{f"a queue of {n} entries": _queue(n) for n in FW.JOIN4_QUEUES},
    "a queue of 72 entries over 8 lists": _q72,
    "a filter word behind the queue equals a queued doc": _pad_overlay,
    "two receiver blocks": _blocks(2), "three receiver blocks": _blocks(3),
    "a doc in all T lists": _all_lists, "a doc in the first and last list only": _first_last,
    "dense join: a list with no queued entry between two that have some": _dense_gap,
    "a longest queue segment of 64": _longest_segment(64), "a longest queue segment of 65": _longest_segment(65),
    "an alias with the sentinels behind a list": _sentinel_alias,
    # plans (the queries of fewterm_worlds.PLANS8)
    "plan: a flat Sum, both join forms": _plan_is(0, 1),
    "plan: a flat DisMax with a tie breaker, both join forms": _plan_is(1, 2, lambda leaf, sq: float(sq["tie"]) > 0),
    "plan: all lists in one leaf": _plan_is(2, 1, lambda leaf, sq: len(set(leaf)) == 1 and len(leaf) == 8),
    "plan: every list its own leaf": _plan_is(3, 2, lambda leaf, sq: len(set(leaf)) == 8),
    "plan: a leaf boundary between lists 4 and 5": _plan_is(4, 2, lambda leaf, sq: len(set(leaf[:4])) == 1 and
                                                            len(set(leaf[4:])) == 1 and leaf[3] != leaf[4]),
    "plan: a leaf none of whose lists has a lane in the round": _idle_leaf,
    "plan: min_match 2, a doc in two lists of one leaf only": _min_match(False),
    "plan: min_match 2, the same with a second leaf": _min_match(True),
    "plan: a negative weight": _negative_weight,
    "plan: a leaf whose term is absent from one of two segments": _absent_leaf,
    # threshold
    "threshold: identical score bits on both sides of rank k": lambda P: _tied(P, lambda n: True),
    "threshold: a single tied with the doc at rank k": lambda P: _tied(P, lambda n: n == 1),
    "threshold: a joined doc tied with the doc at rank k": lambda P: _tied(P, lambda n: n >= 2),
    "threshold: a joined entry meets a compacted threshold of its own score bits with a lower doc id": _tie_after_compaction,
    "threshold: a single with the seed's bits and a single one ulp below": _ulp_singles,
    "threshold: the champion seed on": lambda P: all(float(s["theta0"]) > 0 for s in P.sqs),
    "threshold: the champion seed off": lambda P: all(float(s["theta0"]) == 0 for s in P.sqs),
    "threshold: k=257 with a seed": lambda P: P.facts.cand_mode == 1 and all(float(s["theta0"]) > 0 for s in P.sqs),
    "threshold: k=257 without a seed": lambda P: P.facts.cand_mode == 1 and all(float(s["theta0"]) == 0 for s in P.sqs),
    "threshold: a doc filter keeps the seed off": lambda P: all(int(s["filter"]) != 0 and float(s["theta0"]) == 0 for s in P.sqs),
}

# edges that exist at some k only (the others hold at every k a world runs at)
EDGE_KS = {
    "an over-full round at k=257": (257,),
    "threshold: a joined entry meets a compacted threshold of its own score bits with a lower doc id": (1, 64, 65),
    "threshold: a single with the seed's bits and a single one ulp below": (1,),
    "threshold: identical score bits on both sides of rank k": FW.THRESHOLD_KS,
    "threshold: a joined doc tied with the doc at rank k": (3, 30),
    "threshold: a single tied with the doc at rank k": (90,),
    "threshold: the champion seed on": tuple(k for k in FW.ALL_KS + FW.THRESHOLD_KS),
    "threshold: k=257 with a seed": (257,), "threshold: k=257 without a seed": (257,),
}

# every edge named above must stay promised by a world: dropping it from a world's list fails the suite
REQUIRED = set(EDGES)


def check_edges(P):
    """the plan runs on the few-term kernel and every edge the world promises at this k is in the trace"""
    W = P.W
    what = f"world {W.name}: k={P.k} strategy={P.strategy}"
    assert P.facts.uniform == 1 and P.facts.multi == 0, f"{what}: not on the few-term kernel"
    assert P.facts.pruned == 0 and P.facts.max_terms <= W.ml and (W.ml == 8) == (P.facts.max_terms > 4), what
    assert bool(P.facts.plan_batch) == (W.plans is not None), what
    for name in W.edges:
        if P.k in EDGE_KS.get(name, (P.k,)):
            assert EDGES[name](P), f"{what}: edge not reached: {name}"
    if W.n_rounds is not None:
        assert [int(s["n_rounds"]) for s in P.sqs] == W.n_rounds, what
        assert [int(s["n_slices"]) for s in P.sqs] == W.n_slices, what
        assert all(int(s["longest"]) == 0 for s in P.sqs), what


def check_model(P):
    """the model against itself (beside the assertions of trace() and chunks()): every posting of a slice falls in
    exactly one round or chunk, a cut chunk ends below its round's end, the cuts equal their plain statement"""
    for sub in P.traced:
        L = P.lists(sub)
        assert (sub["b"] == F.plain_cuts(L, sub["longest"], sub["n_rounds"])).all(), f"world {P.W.name}: sub-query {sub['i']}"
        for sl in sub["slices"]:
            seen = [np.zeros(len(x), dtype=np.int64) for x in L]
            for rd in sl["rounds"]:
                for n, w in enumerate(rd["waves"]):
                    taken = w["mine"] & (w["doc"] < w["end"])
                    if rd["chunks"]:
                        c = rd["chunks"][n]
                        assert c["bound"] == DOC_END or c["bound"] + 1 < rd["end"], "a cut chunk ends below its round's end"
                        for t in range(sub["T"]):    # the list whose last loaded doc is the bound consumes all it loaded
                            assert c["lastdoc"][t] != c["bound"] or c["bound"] == DOC_END or c["consumed"][t] == c["chunk"][t]
                        assert [int((taken & (w["lst"] == t)).sum()) for t in range(sub["T"])] == c["consumed"].tolist()
                    for t in range(sub["T"]):
                        np.add.at(seen[t], w["pos"][taken & (w["lst"] == t)], 1)
                    # a queued posting is one of the wave's own, and partners come in whole groups
                    assert (w["doc"][w["queued"]] < w["end"]).all() and w["n"] == len(w["qdoc"])
            for t in range(sub["T"]):
                lo, hi = int(sl["b"][0, t]), int(sl["b"][-1, t])
                assert (seen[t][lo:hi] == 1).all() and seen[t][:lo].sum() == 0 and seen[t][hi:].sum() == 0, \
                    f"world {P.W.name}: sub-query {sub['i']} slice at round {sl['r0']} list {t}"


@pytest.mark.parametrize("world", FW.WORLDS, ids=lambda f: f.__name__)
def test_world_reaches_its_edges(lib, world):
    W = world()
    for strategy in W.strategies:
        for k in W.ks:
            P = FewPlan(lib, W, k, strategy)
            check_edges(P)
    check_model(P)


@pytest.mark.parametrize("world", FW.WORLDS, ids=lambda f: f.__name__)
def test_counters_the_model_predicts(lib, world):
    """scored_docs = the distinct docs of a query's lists, postings_advanced = its postings = what the planner counts"""
    W = world()
    P = FewPlan(lib, W, 11, FW.BM25)
    assert P.docs.tolist() == W.distinct_docs()
    assert P.postings.tolist() == P.q_postings.astype(np.int64).tolist()
    for sub in P.traced:      # every doc of the sub-query is owned by exactly one wave
        docs = sum(len(np.unique(w["doc"][w["mine"] & (w["doc"] < w["end"])])) for s2, *_, w in P.waves() if s2 is sub)
        assert docs == len(np.unique(np.concatenate(P.lists(sub))))


def test_every_listed_edge_is_promised_by_a_world():
    promised = {name for w in FW.WORLDS for name in w().edges}
    assert promised <= set(EDGES), promised - set(EDGES)
    assert REQUIRED <= promised, f"edges no world promises: {sorted(REQUIRED - promised)}"
    assert set(EDGE_KS) <= set(EDGES)
    for w in FW.WORLDS:      # an edge tied to some k is promised by worlds that run at one of them
        for name in w().edges:
            assert set(EDGE_KS.get(name, w().ks)) & set(w().ks), (w().name, name)


def test_cuts_equal_their_plain_statement_whatever_path_finds_them(lib):
    """the three search paths of the prologue (global guess, interpolation window, bisection) and np.searchsorted give
    the same cut points, in every slice of every world; every path is taken somewhere"""
    taken = set()
    for world in FW.WORLDS:
        W = world()
        P = FewPlan(lib, W, 11, FW.BM25)
        for sub in P.traced:
            assert (sub["b"] == F.plain_cuts(P.lists(sub), sub["longest"], sub["n_rounds"])).all(), (W.name, sub["i"])
            for sl in sub["slices"]:
                taken |= set(sl["paths"].values())
    assert taken >= {"first", "last", "longest", "guess", "guess-bisect", "window", "bisect"}, taken
