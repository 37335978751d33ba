// slg_plan.cpp — host planner of a query batch (see slg_plan.hpp).  Host-only C++17.
#include "slg_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <atomic>
#include <cmath>
#include <cstring>
#include <exception>
#include <thread>

namespace slgplan {

namespace {

#define PLAN_REQUIRE(cond, msg)                          \
  do {                                                   \
    if (!(cond)) throw SlgError(SLG_ERR_INVALID, (msg)); \
  } while (0)

inline uint32_t full_mask(uint32_t n) { return n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u); }
static_assert(slg::kMaxPlanDepth == SLG_MAX_PLAN_DEPTH, "the kernels' level arrays and the ABI's depth limit");
constexpr uint32_t kMaxPlanNodes = 255;  // leaves / groups of a two-level plan (8-bit fields of TermRef::gmeta)

// ---- score trees given node by node (slg_score_plans::q_node_offsets) ---------------------------
struct TreeShape {
  uint32_t n_leaf = 0, deepest = 0;  // leaves, depth of the deepest one (the root: 0)
};

// The one walk over a query's tree (pre-order): depth of every node, leaves, deepest leaf.
// kCheck = validate_batch's walk: it refuses a malformed tree before anything indexes through it;
// resolve_tree walks the trees that passed.
template <bool kCheck>
TreeShape walk_tree(const slg_score_plans &pl, uint32_t q, uint32_t *depth_of) {
  const uint32_t n0 = pl.q_node_offsets[q], nn = pl.q_node_offsets[q + 1] - n0;
  const int32_t *kind = pl.node_kind + n0;
  const uint32_t *par = pl.node_parent + n0;
  [[maybe_unused]] uint32_t kids[2 * kMaxPlanNodes + 1];
  TreeShape t;
  for (uint32_t i = 0; i < nn; i++) {
    const int kd = kind[i];
    if constexpr (kCheck) {
      PLAN_REQUIRE(kd == SLG_PLAN_SUM || kd == SLG_PLAN_DISMAX || kd == SLG_PLAN_LEAF, "unknown node kind in query " + std::to_string(q));
      kids[i] = 0;
      if (i != 0) {
        PLAN_REQUIRE(par[i] < i, "node_parent must name an earlier node (pre-order) in query " + std::to_string(q));
        PLAN_REQUIRE(kind[par[i]] != SLG_PLAN_LEAF, "a leaf node has a child in query " + std::to_string(q));
      }
    }
    depth_of[i] = i == 0 ? 0u : depth_of[par[i]] + 1u;
    if constexpr (kCheck)
      if (i != 0) {
        // pre-order: the parent is the last node before i whose depth is smaller
        PLAN_REQUIRE(par[i] == i - 1 || depth_of[i - 1] >= depth_of[i], "nodes are not in pre-order in query " + std::to_string(q));
        kids[par[i]]++;
      }
    if (kd == SLG_PLAN_LEAF) {
      t.n_leaf++;
      t.deepest = std::max(t.deepest, depth_of[i]);
    } else if (kCheck && kd == SLG_PLAN_DISMAX) {
      const float tie = pl.node_tie[n0 + i];
      PLAN_REQUIRE(tie >= 0.0f && tie <= 1.0f, "tie breaker outside [0, 1] in query " + std::to_string(q));
    }
  }
  if constexpr (kCheck)
    for (uint32_t i = 0; i < nn; i++)
      if (kind[i] != SLG_PLAN_LEAF && kids[i] == 0)
        throw SlgError(SLG_ERR_UNSUPPORTED, "a Sum / DisMax node without children in query " + std::to_string(q));
  return t;
}

// ---- validation of the caller's arrays (cheap, before anything indexes through them) ------------
struct BatchFacts {
  uint32_t total_terms = 0;
  uint32_t max_nt = 0;           // most terms of any query
  bool plans_requested = false;  // some query can need a score plan (leaf close on the device)
  bool min_match = false;        // some query has minimum_should_match > 1 (slg_score_plans::q_min_match)
  bool nested_requested = false; // some query names groups of leaves
};

BatchFacts validate_batch(const BatchIn &in) {
  BatchFacts f;
  PLAN_REQUIRE(in.nq == 0 || in.q_offsets != nullptr, "q_offsets is NULL");
  // (strategy, k and the term count per query: also made per request by slg_coalesce.hip check_row)
  PLAN_REQUIRE(in.strategy == SLG_STRATEGY_BM25 || in.strategy == SLG_STRATEGY_WAND ||
                   in.strategy == SLG_STRATEGY_BMW,
               "unknown strategy");
  if (in.k > SLG_MAX_K) throw SlgError(SLG_ERR_UNSUPPORTED, "k > SLG_MAX_K (" + std::to_string(SLG_MAX_K) + ")");
  f.total_terms = in.nq ? in.q_offsets[in.nq] : 0;
  PLAN_REQUIRE(f.total_terms == 0 || (in.q_term_ids && in.q_weights), "q_term_ids/q_weights is NULL");
  for (uint32_t q = 0; q < in.nq; q++) {
    PLAN_REQUIRE(in.q_offsets[q + 1] >= in.q_offsets[q] && in.q_offsets[q + 1] <= f.total_terms,
                 "q_offsets not monotone");
    const uint32_t nt = in.q_offsets[q + 1] - in.q_offsets[q];
    if (nt > SLG_MAX_QUERY_TERMS)
      throw SlgError(SLG_ERR_UNSUPPORTED, "query " + std::to_string(q) + " has more than " +
                                              std::to_string(SLG_MAX_QUERY_TERMS) + " terms");
    f.max_nt = std::max(f.max_nt, nt);
  }
  const slg_score_plans &pl = in.plans;
  if (pl.q_min_match)
    for (uint32_t q = 0; q < in.nq; q++)
      if (pl.q_min_match[q] > 1u) {
        if (pl.q_min_match[q] > 255u) throw SlgError(SLG_ERR_UNSUPPORTED, "minimum_should_match > 255 in query " + std::to_string(q));
        f.min_match = true;
        f.plans_requested = true;  // (counted per leaf in the plan kernel's join)
      }
  const bool trees = pl.q_node_offsets != nullptr;
  PLAN_REQUIRE(!trees || (pl.node_kind && pl.node_tie && pl.node_parent), "score trees need node_kind, node_tie and node_parent");
  if (trees) {
    for (uint32_t q = 0; q < in.nq; q++) {
      PLAN_REQUIRE(pl.q_node_offsets[q + 1] >= pl.q_node_offsets[q], "q_node_offsets not monotone");
      const uint32_t nn = pl.q_node_offsets[q + 1] - pl.q_node_offsets[q];
      PLAN_REQUIRE(nn >= 1, "a score tree has no node in query " + std::to_string(q));
      if (nn > 2 * kMaxPlanNodes)
        throw SlgError(SLG_ERR_UNSUPPORTED, "score tree of query " + std::to_string(q) + " has too many nodes");
      uint32_t depth_of[2 * kMaxPlanNodes + 1];
      const TreeShape tree = walk_tree<true>(pl, q, depth_of);
      if (tree.n_leaf > kMaxPlanNodes) throw SlgError(SLG_ERR_UNSUPPORTED, "score tree of query " + std::to_string(q) + " has too many leaves");
      if (tree.deepest > SLG_MAX_PLAN_DEPTH)
        throw SlgError(SLG_ERR_UNSUPPORTED, "score tree of query " + std::to_string(q) + " is deeper than SLG_MAX_PLAN_DEPTH");
      const uint32_t t0 = in.q_offsets[q], nt = in.q_offsets[q + 1] - t0;
      for (uint32_t i = 0; i < nt; i++)
        PLAN_REQUIRE((pl.q_leaf ? pl.q_leaf[t0 + i] : i) < tree.n_leaf, "a term names a leaf the tree does not have in query " + std::to_string(q));
      f.plans_requested = true;  // (resolved per query: a one-level tree of single-term leaves still is the flat sum)
      if (tree.deepest >= 2) f.nested_requested = true;
    }
    return f;
  }
  const bool groups = pl.leaf_group != nullptr;
  PLAN_REQUIRE(!groups || (pl.q_leaf_offsets && pl.q_group_offsets && pl.group_plan && pl.group_tie && pl.q_nleaves),
               "two-level plans need q_nleaves, q_leaf_offsets, q_group_offsets, group_plan and group_tie");
  for (uint32_t q = 0; q < in.nq; q++) {
    if (pl.q_plan && pl.q_plan[q] == SLG_PLAN_DISMAX) f.plans_requested = true;
    const uint32_t t0 = in.q_offsets[q], nt = in.q_offsets[q + 1] - t0;
    if (pl.q_leaf && !f.plans_requested)
      for (uint32_t i = 0; i < nt && !f.plans_requested; i++)
        for (uint32_t j = 0; j < i; j++)
          if (pl.q_leaf[t0 + i] == pl.q_leaf[t0 + j]) {
            f.plans_requested = true;
            break;
          }
    if (groups) {
      PLAN_REQUIRE(pl.q_leaf_offsets[q + 1] >= pl.q_leaf_offsets[q] && pl.q_group_offsets[q + 1] >= pl.q_group_offsets[q],
                   "q_leaf_offsets / q_group_offsets not monotone");
      const uint32_t nl = pl.q_leaf_offsets[q + 1] - pl.q_leaf_offsets[q];
      const uint32_t ng = pl.q_group_offsets[q + 1] - pl.q_group_offsets[q];
      PLAN_REQUIRE(nl == pl.q_nleaves[q], "q_leaf_offsets disagrees with q_nleaves in query " + std::to_string(q));
      // (the descriptors keep a group's id and its leaf count in 8 bits each; leaves without a
      //  term are legal — a DisMax counts them as 0.0 — so the limits are not the term limit)
      if (nl > kMaxPlanNodes || ng > kMaxPlanNodes)
        throw SlgError(SLG_ERR_UNSUPPORTED, "query " + std::to_string(q) + " has more than " +
                                                std::to_string(kMaxPlanNodes) + " leaves or groups");
      uint32_t prev = 0;
      bool is_flat = ng == nl;  // every leaf its own Sum group == the flat plan
      for (uint32_t l = 0; l < nl; l++) {
        const uint32_t g = pl.leaf_group[pl.q_leaf_offsets[q] + l];
        PLAN_REQUIRE(g < ng, "leaf_group out of range in query " + std::to_string(q));
        // leaves are numbered in the plan's traversal order, so a group's leaves are consecutive
        PLAN_REQUIRE(l == 0 || g == prev || g == prev + 1, "leaf_group must be non-decreasing without gaps");
        PLAN_REQUIRE(l != 0 || g == 0, "leaf_group must start at group 0");
        prev = g;
        if (g != l) is_flat = false;
      }
      PLAN_REQUIRE(nl == 0 || prev + 1 == ng, "a group has no leaf in query " + std::to_string(q));
      for (uint32_t g = 0; g < ng; g++) {
        const int gk = pl.group_plan[pl.q_group_offsets[q] + g];
        const float gt = pl.group_tie[pl.q_group_offsets[q] + g];
        PLAN_REQUIRE(gk == SLG_PLAN_SUM || gk == SLG_PLAN_DISMAX, "unknown group plan in query " + std::to_string(q));
        PLAN_REQUIRE(gt >= 0.0f && gt <= 1.0f, "tie breaker outside [0, 1] in query " + std::to_string(q));
        if (gk == SLG_PLAN_DISMAX) is_flat = false;
      }
      if (!is_flat && nl) {
        f.nested_requested = true;
        f.plans_requested = true;
      }
    }
  }
  return f;
}

// ---- pass 1: sub-queries (query x segment) and their terms ---------------------------------------
// Per query (plan_queries): resolve_plan -> per segment: build_subquery -> seed_and_classify.

// Score plan of one query (query/planner.rs:113-153), resolved from whichever form the caller used: root
// over leaves (q_plan / q_leaf), root over groups of leaves (leaf_group / group_plan), or a tree given node
// by node, which becomes one of the first two when it has one or two levels and a canonical node table
// otherwise.  One object serves every query of a plan_queries call: resolve_plan assigns the scalars and
// pointers per query, the arrays are scratch that only the queries needing them write.
struct QueryPlan {
  int kind;  // the root: SLG_PLAN_SUM | SLG_PLAN_DISMAX
  float tie;
  uint32_t min_match, n_leaves;
  // two-level plan: group of every leaf, leaves per group (nested: it is not the flat plan in disguise)
  bool groups, nested;
  uint32_t n_groups;
  const uint32_t *lgroup;  // (these three: the caller's arrays, or tree_* below)
  const int32_t *gplan;
  const float *gtie;
  uint32_t leaves_in_group[kMaxPlanNodes + 1];  // (zeroed only for queries with groups: 1 KB per query otherwise)
  // deep tree: levels of internal nodes (0: none), first canonical node, canonical node every leaf hangs off
  uint32_t depth, node_begin;
  uint32_t leaf_node[kMaxPlanNodes + 1];
  // the group view of a two-level tree; depth of every node of the tree
  uint32_t tree_lgroup[kMaxPlanNodes + 1];
  int32_t tree_gplan[kMaxPlanNodes + 1];
  float tree_gtie[kMaxPlanNodes + 1];
  uint32_t depth_of[2 * kMaxPlanNodes + 1];
};

// deep tree: canonical node table — the internal nodes in pre-order, and under every leaf that
// hangs above the deepest level a chain of one-child Sum nodes down to it
void build_node_table(const slg_score_plans &pl, uint32_t q, std::vector<slg::PlanNode> &nodes, QueryPlan &p) {
  const uint32_t n0 = pl.q_node_offsets[q], nn = pl.q_node_offsets[q + 1] - n0;
  const int32_t *kind = pl.node_kind + n0;
  const float *ntie = pl.node_tie + n0;
  const uint32_t *par = pl.node_parent + n0;
  p.node_begin = (uint32_t)nodes.size();
  uint32_t canon[2 * kMaxPlanNodes + 1];  // original internal node -> canonical index
  uint32_t lf = 0;
  for (uint32_t i = 0; i < nn; i++) {
    if (kind[i] != SLG_PLAN_LEAF) {
      const bool dismax = kind[i] == SLG_PLAN_DISMAX;
      canon[i] = (uint32_t)nodes.size() - p.node_begin;
      nodes.push_back(slg::PlanNode{i == 0 ? 0u : canon[par[i]], 0u, dismax ? 1u : 0u, dismax ? ntie[i] : 0.0f});
      if (i != 0) nodes[p.node_begin + canon[par[i]]].n_children++;
    } else {
      uint32_t above = canon[par[i]];
      nodes[p.node_begin + above].n_children++;
      for (uint32_t d = p.depth_of[i]; d < p.depth; d++) {  // pad: Sum of one child
        nodes.push_back(slg::PlanNode{above, 1u, 0u, 0.0f});
        above = (uint32_t)nodes.size() - 1u - p.node_begin;
      }
      p.leaf_node[lf++] = above;
    }
  }
}

// a tree given node by node (validate_batch has walked it): root, leaves, and the group view or node table
void resolve_tree(const slg_score_plans &pl, uint32_t q, std::vector<slg::PlanNode> &nodes, QueryPlan &p) {
  const uint32_t n0 = pl.q_node_offsets[q], nn = pl.q_node_offsets[q + 1] - n0;
  const int32_t *kind = pl.node_kind + n0;
  const float *ntie = pl.node_tie + n0;
  const TreeShape tree = walk_tree<false>(pl, q, p.depth_of);
  p.n_leaves = tree.n_leaf;
  p.kind = kind[0] == SLG_PLAN_LEAF ? SLG_PLAN_SUM : kind[0];  // (the plan is one leaf: Sum of one leaf)
  p.tie = kind[0] == SLG_PLAN_DISMAX ? ntie[0] : 0.0f;
  if (tree.deepest > 2) {
    p.depth = tree.deepest;
    build_node_table(pl, q, nodes, p);
  } else if (tree.deepest == 2) {  // root over groups (one level: root over leaves, nothing to add)
    p.groups = true;
    p.n_groups = 0;
    uint32_t lf = 0;
    for (uint32_t i = 1; i < nn; i++) {
      if (p.depth_of[i] == 1) {  // a child of the root: a group (a bare leaf = a Sum group of one leaf)
        p.tree_gplan[p.n_groups] = kind[i] == SLG_PLAN_DISMAX ? SLG_PLAN_DISMAX : SLG_PLAN_SUM;
        p.tree_gtie[p.n_groups] = kind[i] == SLG_PLAN_DISMAX ? ntie[i] : 0.0f;
        p.n_groups++;
      }
      if (kind[i] == SLG_PLAN_LEAF) p.tree_lgroup[lf++] = p.n_groups - 1u;
    }
    p.lgroup = p.tree_lgroup;
    p.gplan = p.tree_gplan;
    p.gtie = p.tree_gtie;
  }
}

// step 1: the score plan of query q.  nodes: where a deep tree's canonical node table is appended
void resolve_plan(const BatchIn &in, uint32_t q, std::vector<slg::PlanNode> &nodes, QueryPlan &p) {
  const slg_score_plans &pl = in.plans;
  p.kind = pl.q_plan ? pl.q_plan[q] : SLG_PLAN_SUM;
  p.tie = pl.q_tie ? pl.q_tie[q] : 0.0f;
  p.min_match = pl.q_min_match ? pl.q_min_match[q] : 0u;
  p.n_leaves = pl.q_nleaves ? pl.q_nleaves[q] : 0;
  p.groups = pl.leaf_group != nullptr && pl.q_node_offsets == nullptr;
  p.lgroup = p.groups ? pl.leaf_group + pl.q_leaf_offsets[q] : nullptr;
  p.n_groups = p.groups ? pl.q_group_offsets[q + 1] - pl.q_group_offsets[q] : 0u;
  p.gplan = p.groups ? pl.group_plan + pl.q_group_offsets[q] : nullptr;
  p.gtie = p.groups ? pl.group_tie + pl.q_group_offsets[q] : nullptr;
  p.depth = p.node_begin = 0;
  if (pl.q_node_offsets) {
    resolve_tree(pl, q, nodes, p);
  } else {
    // (plan, tie and leaf: checks on ONE query that slg_coalesce.hip check_row also makes per request — keep the two together)
    PLAN_REQUIRE(p.kind == SLG_PLAN_SUM || p.kind == SLG_PLAN_DISMAX,
                 "unknown score plan in query " + std::to_string(q));
    // validate_tie_breaker (query/planner.rs:850-856); the threshold seed and the pruning bounds
    // also rely on it: with tie in [0, 1] a DisMax is >= each of its non-negative leaves
    PLAN_REQUIRE(p.tie >= 0.0f && p.tie <= 1.0f, "tie breaker outside [0, 1] in query " + std::to_string(q));
  }
  const uint32_t t0 = in.q_offsets[q], nt = in.q_offsets[q + 1] - t0;
  for (uint32_t i = 0; i < nt; i++) {
    const uint32_t lf = pl.q_leaf ? pl.q_leaf[t0 + i] : i;
    PLAN_REQUIRE(lf < 0x80000000u, "leaf index >= 2^31 in query " + std::to_string(q));
    p.n_leaves = std::max(p.n_leaves, lf + 1u);
  }
  p.nested = false;
  if (p.groups) {
    std::memset(p.leaves_in_group, 0, sizeof(p.leaves_in_group));
    if (!pl.q_node_offsets)
      PLAN_REQUIRE(p.n_leaves == pl.q_nleaves[q], "a term names a leaf beyond q_nleaves in query " + std::to_string(q));
    for (uint32_t l = 0; l < p.n_leaves; l++) p.leaves_in_group[p.lgroup[l]]++;
    for (uint32_t g = 0; g < p.n_groups; g++)
      if (p.leaves_in_group[g] != 1 || p.gplan[g] == SLG_PLAN_DISMAX) p.nested = true;
  }
}

// what pass 2 and the accounting need of a sub-query beside its RoundQuery
struct SqCount {
  uint64_t ess, all;     // postings of the essential lists (what the round planner cuts), of all lists
  uint32_t longest_all;  // longest list of the sub-query, classification aside
};

struct Pass1Out {
  std::vector<slg::RoundQuery> sqs;
  std::vector<slg::TermRef> terms;
  std::vector<SqCount> counts;  // [sqs.size()]
  double skip_est = 0.0;        // postings block skipping is expected to leave unread
  uint64_t n_postings = 0, n_ess = 0;
  uint32_t max_terms = 0;
  bool any_plan = false, any_filter = false, any_nested = false, any_deep = false;
  std::vector<slg::PlanNode> nodes;  // canonical node tables of this part's deep trees
};

struct Pass1Ctx {
  const std::vector<SegView> &segs;
  const slg_tuning &tn;
  const BatchIn &in;
  const BatchFacts &facts;
  bool maxscore_on;
  std::vector<uint64_t> &q_postings;
};

// threshold seed theta0 = max_t w_t * champ[t][rank(k)]: an exact lower bound of the k-th best score
// whenever no weight is negative (a doc's total is then >= each of its contributions: Sum, or
// DisMax with tie in [0, 1], at either level of the plan) and no doc filter can reject the champions
float threshold_seed(const SegView &sh, const slg::TermRef *t, uint32_t n, uint32_t k, uint32_t fq) {
  if (!sh.champ || k > 1024u || fq != 0) return 0.0f;
  float seed = 0.0f;
  for (uint32_t i = 0; i < n; i++) {
    if (!(t[i].weight >= 0.0f)) return 0.0f;
    if (t[i].weight > 0.0f)
      seed = std::max(seed, t[i].weight * sh.champ[(size_t)t[i].term * slg::kChampions + slg::champ_index(k)]);
  }
  return seed;
}

// MaxScore classification (strategies Wand / Bmw; exact): lists taken in ascending order of their
// maximum contribution ub_t = w_t * champ[t][0] are non-essential while the running sum of ub stays
// below theta0: a doc found only in them totals < theta0 and cannot reach the top-k
uint32_t classify_essential(const SegView &sh, const slg::TermRef *t, uint32_t n, float theta0) {
  uint32_t ess_mask = full_mask(n);
  std::vector<std::pair<float, uint32_t>> ub(n);
  for (uint32_t i = 0; i < n; i++) ub[i] = {t[i].weight * sh.champ[(size_t)t[i].term * slg::kChampions], i};
  std::sort(ub.begin(), ub.end());
  double acc = 0.0;
  for (uint32_t i = 0; i + 1 < n; i++) {  // at least one list stays essential
    acc += (double)ub[i].first;
    // margin: f32 sums of the real contributions may round up by a few ulps
    if (acc * (1.0 + 1e-5) < (double)theta0)
      ess_mask &= ~(1u << ub[i].second);
    else
      break;
  }
  return ess_mask;
}

// step 2: the term list of (query q, segment sq.seg), appended to `terms` and sorted by leaf, and the
// plan fields of sq.  false: no term of the query has a posting in the segment (no sub-query)
bool build_subquery(const Pass1Ctx &c, const QueryPlan &p, uint32_t q, std::vector<slg::TermRef> &terms,
                    slg::RoundQuery &sq) {
  const BatchIn &in = c.in;
  const slg_score_plans &pl = in.plans;
  const uint32_t n_segs = (uint32_t)c.segs.size();
  const SegView &sh = c.segs[sq.seg];
  const uint32_t t0 = in.q_offsets[q], nt = in.q_offsets[q + 1] - t0;
  sq.term_begin = (uint32_t)terms.size();
  for (uint32_t i = 0; i < nt; i++) {
    const uint32_t tid = in.q_term_ids[(size_t)(t0 + i) * n_segs + sq.seg];
    if (tid == SLG_NO_TERM) continue;
    // (this and the weight check below: checks on ONE query that slg_coalesce.hip check_row also makes per request — keep the two together)
    PLAN_REQUIRE(tid < sh.n_terms, "term id out of range in query " + std::to_string(q));
    const uint32_t df = (uint32_t)(sh.term_offsets[tid + 1] - sh.term_offsets[tid]);
    if (df == 0) continue;  // wand.rs:441 filter(postings.len() > 0)
    const float w = in.q_weights[t0 + i];
    PLAN_REQUIRE(std::isfinite(w), "non-finite weight in query " + std::to_string(q));
    slg::TermRef tr{};
    tr.off = sh.term_offsets[tid] + (uint64_t)slg::kListPad * tid;  // padded layout (SegDev)
    tr.df = df;
    tr.weight = w;
    tr.term = tid;
    tr.leaf = pl.q_leaf ? pl.q_leaf[t0 + i] : i;
    if (p.depth) {
      tr.gmeta = p.leaf_node[tr.leaf];  // the canonical node the leaf hangs off
    } else if (p.nested) {
      const uint32_t g = p.lgroup[tr.leaf];
      tr.gmeta = g | (p.leaves_in_group[g] << 8) | ((p.gplan[g] == SLG_PLAN_DISMAX ? 1u : 0u) << 16);
      tr.gtie = p.gtie[g];
    }
    terms.push_back(tr);
  }
  sq.n_terms = (uint32_t)terms.size() - sq.term_begin;
  if (sq.n_terms == 0) return false;
  slg::TermRef *first = terms.data() + sq.term_begin;
  // Lists go to the device sorted by leaf (stable: a leaf's terms keep the term order in
  // which the reference adds them, wand.rs:488-497; a group's leaves are consecutive, so the
  // lists are sorted by group too).  plan 0 = the flat term-order sum, which is what Sum
  // gives when no leaf holds two terms.
  if (pl.q_leaf)  // (without leaves given, leaf = term position: already in order)
    std::stable_sort(first, first + sq.n_terms,
                     [](const slg::TermRef &a, const slg::TermRef &b) { return a.leaf < b.leaf; });
  bool shared = false;
  uint32_t present = 0;
  for (uint32_t i = 0; i < sq.n_terms; i++) {
    const bool fresh = i == 0 || first[i].leaf != first[i - 1].leaf;
    present += fresh ? 1u : 0u;
    shared = shared || !fresh;
  }
  sq.plan = p.kind == SLG_PLAN_DISMAX ? 2u : ((shared || p.nested || p.depth) ? 1u : 0u);
  if (p.min_match > 1u) {  // leaves are counted in the plan kernel's leaf close: Sum of leaves, bits 8.. = the count asked for
    if (sq.plan == 0u) sq.plan = 1u;
    sq.plan |= p.min_match << 8;
  }
  sq.tie = p.tie;
  sq.max_init = present < p.n_leaves ? 0.0f : -INFINITY;
  sq.n_leaves = p.n_leaves;
  sq.n_groups = p.nested ? p.n_groups : 0u;
  sq.depth = p.depth;
  sq.node_begin = p.node_begin;
  return true;
}

// step 3: seed and classify the sub-query whose lists are t[0 .. sq.n_terms): theta0, ess_mask, longest,
// skip_mask (its expected saving is added to skip_est, list by list); returns its posting counts
SqCount seed_and_classify(const Pass1Ctx &c, const slg::TermRef *t, uint32_t k, uint32_t min_match,
                          slg::RoundQuery &sq, double &skip_est) {
  const SegView &sh = c.segs[sq.seg];
  // (minimum_should_match > 1: the champions behind the seed are single postings — docs the matcher may reject)
  sq.theta0 = min_match > 1u ? 0.0f : threshold_seed(sh, t, sq.n_terms, k, sq.filter);
  // MaxScore: by default for batches with a query of >= 5 terms (plan_batch drops the
  // classification again when block skipping has nothing to gain);
  // slg_tuning.pruning = 1 / 0 forces it on / off.  Never with score plans in the batch (the
  // plan kernels have no classified path).
  uint32_t ess_mask = full_mask(sq.n_terms);
  if (c.in.strategy != SLG_STRATEGY_BM25 && sq.theta0 > 0.0f && !c.facts.plans_requested && sq.n_terms > 1 &&
      c.maxscore_on)
    ess_mask = classify_essential(sh, t, sq.n_terms, sq.theta0);
  sq.ess_mask = ess_mask;
  // the round planner works on the essential lists only
  SqCount n{0, 0, 0};
  uint32_t longest = 0, longest_df = 0, longest_all_df = 0;
  for (uint32_t i = 0; i < sq.n_terms; i++) {
    const uint32_t df = t[i].df;
    n.all += df;
    if (df > longest_all_df) {
      longest_all_df = df;
      n.longest_all = i;
    }
    if (!((ess_mask >> i) & 1u)) continue;
    n.ess += df;
    if (df > longest_df) {
      longest_df = df;
      longest = i;
    }
  }
  sq.longest = longest;
  // block skipping pays where a 64-posting block of a non-essential list usually holds no
  // candidate doc: a block spans 64 * N / df docs, which hold 64 * P / df essential postings
  // on average; blocks are tested only below 2 (>= e^-2 = 13 % of them can be skipped).
  // Config 3's lists are all of similar density (>= 64 per block): no test, no cost.
  sq.skip_mask = 0;
  if (c.tn.block_max)
    for (uint32_t i = 0; i < sq.n_terms && i < 32; i++) {
      const uint64_t df = t[i].df;
      if (!((ess_mask >> i) & 1u) && 64ull * n.ess < 2ull * df) {
        sq.skip_mask |= 1u << i;
        skip_est += (double)df * std::exp(-64.0 * (double)n.ess / (double)df);  // blocks without a candidate doc
      }
    }
  return n;
}

void plan_queries(const Pass1Ctx &c, const uint32_t q_lo, const uint32_t q_hi, Pass1Out &o) {
  const BatchIn &in = c.in;
  const uint32_t n_segs = (uint32_t)c.segs.size();
  const uint32_t k = planning_k(in);
  o.sqs.reserve((size_t)(q_hi - q_lo) * n_segs);
  o.terms.reserve((size_t)(in.q_offsets[q_hi] - in.q_offsets[q_lo]) * n_segs);
  o.counts.reserve(o.sqs.capacity());
  // the champion table is tens of MB (config 2: 71 MB) and a query touches one line of it per term
  // (cold for queries that were not planned just before): the lines of the query 8 ahead are
  // requested while this one is planned
  auto prefetch_query = [&](const uint32_t q) {
    const uint32_t t0 = in.q_offsets[q], nt = in.q_offsets[q + 1] - t0;
    for (uint32_t i = 0; i < nt; i++)
      for (uint32_t s = 0; s < n_segs; s++) {
        const uint32_t tid = in.q_term_ids[(size_t)(t0 + i) * n_segs + s];
        const SegView &sh = c.segs[s];
        if (tid == SLG_NO_TERM || tid >= sh.n_terms) continue;
        __builtin_prefetch(&sh.term_offsets[tid]);
        if (sh.champ && k <= 1024u) {
          __builtin_prefetch(&sh.champ[(size_t)tid * slg::kChampions + slg::champ_index(k)]);
          if (c.maxscore_on) __builtin_prefetch(&sh.champ[(size_t)tid * slg::kChampions]);
        }
      }
  };
  QueryPlan plan;  // (one for the whole call: see QueryPlan)
  for (uint32_t q = q_lo; q < std::min(q_hi, q_lo + 8u); q++) prefetch_query(q);
  for (uint32_t q = q_lo; q < q_hi; q++) {
    if (q + 8u < q_hi) prefetch_query(q + 8u);
    uint32_t fq = 0;  // doc filter of the query (0 none, id + 1)
    if (in.q_filter && in.q_filter[q] >= 0) {
      // (a check on ONE query that slg_coalesce.hip check_row also makes per request — keep the two together)
      PLAN_REQUIRE((size_t)in.q_filter[q] < in.n_filters && in.filter_live[in.q_filter[q]],
                   "unknown filter id in query " + std::to_string(q));
      fq = (uint32_t)in.q_filter[q] + 1u;
      o.any_filter = true;
    }
    resolve_plan(in, q, o.nodes, plan);
    if (k == 0) continue;  // wand.rs:413-416: k == 0 and no collector => no work
    for (uint32_t s = 0; s < n_segs; s++) {
      slg::RoundQuery sq{};
      sq.q = q;
      sq.seg = s;
      sq.filter = fq;
      if (!build_subquery(c, plan, q, o.terms, sq)) continue;
      if (sq.plan) o.any_plan = true;
      if (plan.nested) o.any_nested = true;
      if (plan.depth) o.any_deep = true;
      const SqCount n = seed_and_classify(c, o.terms.data() + sq.term_begin, k, plan.min_match, sq, o.skip_est);
      c.q_postings[q] += n.all;
      o.n_postings += n.all;
      o.n_ess += n.ess;
      o.max_terms = std::max(o.max_terms, sq.n_terms);
      o.sqs.push_back(sq);
      o.counts.push_back(n);
    }
  }
}

// ---- pass 2: rounds of about one register set of postings, slices of consecutive rounds ----------
// postings per round of a few-term sub-query.  The kernel's blocked layout (slg_score_uni4.hpp):
// a list is padded to whole lanes of 8 postings, a round has 64 lanes.  A round that needs more
// lanes is streamed in chunks at 2-3x the cost, so the target follows the sub-query's own mix of
// list lengths: the largest R whose expected lanes stay under 64 with `sigmas` to spare.  The
// longest list is cut at exact strides (its count is R * f); every other list's count c is roughly
// Poisson around R * f: ceil(c / 8) has mean c/8 + 7/16 and variance c/64 + 1/12.
uint32_t uniform_round_target(const slg::RoundQuery &sq, const slg::TermRef *t, uint64_t P, const slg_tuning &tn) {
  const uint32_t n = sq.n_terms;
  const double Pd = (double)P;
  // sigmas to spare: 1.0 / 1.6 / 2.0 / 2.5 / 3.0 / 3.5 / 4.0 / 5.0 -> 0.0874 / 0.0791 / 0.0762 /
  // 0.0744 / 0.0728 / 0.0727 / 0.0734 / 0.0752 ms on config 2 (an over-full round costs 2-3 rounds)
  const double sigmas = tn.uniform_sigma_x100 ? tn.uniform_sigma_x100 / 100.0 : 3.2;
  uint32_t dflt = (uint32_t)slg::kUniCap;
  if (!tn.uniform_round_target && n > 1) {
    // lanes a round of R postings is expected to need, plus `sigmas` standard deviations
    auto lanes_needed = [&](const uint32_t R) {
      double mu = 0.0, var = 0.0;
      for (uint32_t j = 0; j < n; j++) {
        const double c = (double)R * (double)t[j].df / Pd;
        if (j == sq.longest) {
          mu += std::ceil(c / 8.0);
        } else {
          mu += c / 8.0 + 7.0 / 16.0;
          var += c / 64.0 + 1.0 / 12.0;
        }
      }
      return mu + sigmas * std::sqrt(var);
    };
    // the largest R (steps of 8) that stays under 64.3 lanes.  With f = the longest list's share of
    // the postings: mu ~ R/8 + b, var = c R + d (b = 7/16 (n-1) + 1/2, c = (1-f)/64, d = (n-1)/12);
    // R/8 + b + s sqrt(c R + d) = 64.3 is a quadratic in y = sqrt(c R + d); the root is then
    // corrected against the exact count (the ceil) in steps of 8 — usually two evaluations (a scan
    // over all 53 candidates cost 70 ms of planning on config 4's 65 536 sub-queries)
    const double f = (double)t[sq.longest].df / Pd;
    const double b = 7.0 / 16.0 * (n - 1) + 0.5, c = (1.0 - f) / 64.0, d = (n - 1) / 12.0;
    double x = (64.3 - b) * 8.0;
    if (c > 1e-9) {
      const double qa = 1.0 / (8.0 * c), qc = b - 64.3 - d / (8.0 * c);
      const double y = (-sigmas + std::sqrt(sigmas * sigmas - 4.0 * qa * qc)) / (2.0 * qa);
      x = (y * y - d) / c;
    }
    uint32_t R = (uint32_t)std::min(std::max(x, 64.0), (double)slg::kUniCap) & ~7u;
    while (R > 64 && lanes_needed(R) > 64.3) R -= 8;
    while (R + 8 <= (uint32_t)slg::kUniCap && lanes_needed(R + 8) <= 64.3) R += 8;
    dflt = R;
  }
  return std::max<uint32_t>(48, std::min<uint32_t>(tn.uniform_round_target ? tn.uniform_round_target : dflt,
                                                   (uint32_t)slg::kUniCap));
}

// the many-term kernel's bitmap covers a window of kSpan docs: a round whose essential postings are
// spread over more is cut into chunks, each paying the round's fixed costs.  Sparse sub-queries get
// rounds that fit the window (postings per round <= 0.85 * kSpan * density of the essential lists)
// Threads a large batch's planning may use: the CPUs this process may run on (the cgroup's quota where there
// is one: a container shows every CPU of its host — the GPU boxes 256 for a quota of 16), divided among
// the plan_batch calls running at this moment (config 4's harness has four caller threads planning at
// once: 4 x 8 planner threads on 16 CPUs made one box plan a batch in 42 ms instead of 19), at most 8.
std::atomic<int> g_plans_running{0};
uint32_t cpu_budget() {
  static const uint32_t quota = [] {
    uint32_t n = std::max(1u, std::thread::hardware_concurrency());
    if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char a[32] = {0};
      unsigned long long period = 0;
      if (std::fscanf(f, "%31s %llu", a, &period) == 2 && period > 0 && std::strcmp(a, "max") != 0) {
        const unsigned long long q = std::strtoull(a, nullptr, 10);
        if (q > 0) n = std::min<uint32_t>(n, (uint32_t)std::max<unsigned long long>(1, (q + period - 1) / period));
      }
      std::fclose(f);
    }
    return n;
  }();
  return quota;
}
uint32_t planner_threads() {
  const int running = std::max(1, g_plans_running.load(std::memory_order_relaxed));
  return std::max<uint32_t>(1, std::min<uint32_t>(8, cpu_budget() / (uint32_t)running));
}

// fn(t, lo, hi) for each of n_thr contiguous ranges [lo, hi) of [0, n), t = the range's number: every range
// on a thread of its own, a single one on the caller's.  A range that throws ends alone; once all have
// ended the exception of the lowest range is rethrown
template <typename Fn>
void fan_out(size_t n, size_t n_thr, Fn fn) {
  if (n_thr <= 1) return fn((size_t)0, (size_t)0, n);
  std::vector<std::exception_ptr> errs(n_thr);
  std::vector<std::thread> pool;
  for (size_t t = 0; t < n_thr; t++)
    pool.emplace_back([&, t] {
      try {
        fn(t, n * t / n_thr, n * (t + 1) / n_thr);
      } catch (...) {
        errs[t] = std::current_exception();
      }
    });
  for (auto &th : pool) th.join();
  for (auto &e : errs)
    if (e) std::rethrow_exception(e);
}

uint32_t multi_round_target(uint64_t P, uint32_t n_docs, const slg_tuning &tn) {
  uint32_t target = std::max<uint32_t>(64, std::min<uint32_t>(tn.multi_round_target, (uint32_t)slg::kMultiCap));
  const double dens = (double)P / (double)std::max<uint32_t>(1u, n_docs);
  const double fit = 0.85 * (double)slg::kSpan * dens;  // (0.65 / 0.75 / 0.85 / 0.95 / 1.0 measured on config 3:
                                                         //  7.88 / 7.54 / 7.35 / 7.76 / 8.20 ms; no rule: 8.69)
  if (fit < (double)target) target = (uint32_t)std::max(64.0, fit);
  return target;
}

void plan_rounds(const std::vector<SegView> &segs, const slg_tuning &tn, uint32_t k,
                 const std::vector<SqCount> &counts, Plan &out) {
  auto &sqs = out.sqs;
  const uint32_t probe_target = std::max<uint32_t>((uint32_t)slg::kMultiCap, tn.probe_target);
  // rounds per slice: short slices pack the tail of the launch better (one wave per slice).  The
  // few-term kernel's slices are cheap to start (threshold seed + buffered top-k) as long as k is
  // small: every slice writes k candidates for the merge (measured: config 2 k=11 best at 4,
  // config 3 k=101 best at 8).
  const bool rps_pinned = tn.rounds_per_slice != 0;
  const uint32_t max_rps = std::max<uint32_t>(
      1, std::min<uint32_t>(rps_pinned ? tn.rounds_per_slice
                                       : (out.uniform && k <= 64 ? (uint32_t)slg::kUniRoundsPerSlice
                                                                 : (uint32_t)slg::kDefaultRoundsPerSlice),
                            (uint32_t)slg::kMaxRoundsPerSlice));
  // longest slices: 8 rounds on the few-term kernel (measured on config 2: the heaviest
  // sub-queries' 16-round slices were the tail of the launch), 16 on the many-term kernel and on the
  // 5..8-list form for large k (config 3, k = 101: 5.03 ms at 16, 5.11 at 8), 6 on that form for
  // k <= 64 (multi-field workload, k = 11: the 15-round slices of the dense sub-queries ran 125 us
  // of a 144-us launch; 0.165 ms at 15, 0.124 at 6, 0.135 at 4)
  const bool blocked8 = out.uniform && out.max_terms > (uint32_t)slg::kUniMaxLists;
  const uint32_t rps_cap = std::max<uint32_t>(
      max_rps, tn.max_rounds_per_slice ? tn.max_rounds_per_slice
                                       : (out.uniform && !blocked8 ? 8u
                                          : (blocked8 && k <= 64 ? 6u : (uint32_t)slg::kMaxRoundsPerSlice)));
  const uint32_t slices_per_sq = tn.slices_per_subquery;
  const bool slice_lists = !out.cand_mode;
  // the round targets are independent per sub-query: large batches (config 4: 65 536 sub-queries)
  // compute them on several threads; the offsets below are a serial prefix
  std::vector<uint32_t> targets(sqs.size());
  fan_out(sqs.size(), sqs.size() >= 8192 ? planner_threads() : 1, [&](size_t, size_t a, size_t b) {
    for (size_t i = a; i < b; i++) {
      const slg::RoundQuery &sq = sqs[i];
      const slg::TermRef *t = out.terms.data() + sq.term_begin;
      targets[i] = out.uniform ? uniform_round_target(sq, t, counts[i].ess, tn)
                               : multi_round_target(counts[i].ess, segs[sq.seg].n_docs, tn);
    }
  });
  for (size_t i = 0; i < sqs.size(); i++) {
    slg::RoundQuery &sq = sqs[i];
    const slg::TermRef *t = out.terms.data() + sq.term_begin;
    const uint32_t dfL = t[sq.longest].df;
    const uint32_t round_target = targets[i];
    // a round holds <= ~round_target postings of the essential lists (register slots) and
    // <= ~probe_target postings overall (non-essential lists are streamed per round), so
    // slices stay balanced whatever the mix
    uint64_t nr = (counts[i].ess + round_target - 1) / round_target;
    nr = std::max<uint64_t>(nr, (counts[i].all + probe_target - 1) / probe_target);
    nr = std::max<uint64_t>(1, std::min<uint64_t>(nr, dfL));
    // sub-queries with many rounds get longer slices (fewer candidate lists for the merge,
    // whose time is set by the heaviest query); they are launched first (slice_order below)
    uint32_t want_rps = max_rps;
    if (!rps_pinned)
      want_rps = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(max_rps, (nr + slices_per_sq - 1) / slices_per_sq), rps_cap);
    // (the few-term kernel keeps a slice's cut points in one row of 64 words, 128 in the 5..8-list
    //  instance of the blocked form: (rps+1)*T <= 64 / 128)
    const uint32_t row = blocked8 && sq.n_terms > (uint32_t)slg::kUniMaxLists ? 128u : 64u;
    const uint32_t rps = out.multi ? std::max<uint32_t>(1, want_rps)
                                   : std::max<uint32_t>(1, std::min<uint32_t>(want_rps, row / sq.n_terms - 1));
    const uint64_t S = (nr + rps - 1) / rps;
    // (the per-slice candidate lists, n_slices * k entries indexed with 32 bits, exist only for
    //  k <= 256; larger k goes through the candidate array, one slot per posting)
    PLAN_REQUIRE(nr < 0x7FFFFFFFull && out.slice_sq.size() + S < 0x7FFFFFFFull &&
                     (!slice_lists ||
                      (out.slice_sq.size() + S) * (uint64_t)std::max<uint32_t>(k, 1) < 0xFFFFFFFFull),
                 "batch too large (rounds)");
    sq.n_rounds = (uint32_t)nr;
    sq.rounds_per_slice = rps;
    sq.slice_begin = (uint32_t)out.slice_sq.size();
    sq.n_slices = (uint32_t)S;
    PLAN_REQUIRE(out.n_bounds + (nr + 1) * sq.n_terms < 0xFFFFFFFFull, "batch too large (bounds)");
    sq.bounds_begin = (uint32_t)out.n_bounds;
    sq.rdoc_begin = (uint32_t)out.n_bnd;
    sq.bnd_begin = (uint32_t)out.n_bnd;
    out.n_bounds += (nr + 1) * sq.n_terms;
    out.n_bnd += nr + 1;
    out.n_rounds += nr;
    out.slice_sq.insert(out.slice_sq.end(), (size_t)S, (uint32_t)i);
    out.slice_seg.insert(out.slice_seg.end(), (size_t)S, sq.seg);
  }
}

// launch order: slices with the most rounds first (counting sort, stable), so the short ones fill
// the tail of the launch
void order_slices(const slg_tuning &tn, Plan &out) {
  out.slice_order.resize(out.slice_sq.size());
  std::vector<uint32_t> nrounds(out.slice_sq.size());
  uint32_t hist[slg::kMaxRoundsPerSlice + 2] = {0};
  for (const slg::RoundQuery &sq : out.sqs)
    for (uint32_t j = 0; j < sq.n_slices; j++) {
      const uint32_t r0 = j * sq.rounds_per_slice;
      const uint32_t n = std::min<uint32_t>(sq.rounds_per_slice, sq.n_rounds - r0);
      nrounds[sq.slice_begin + j] = n;
      hist[slg::kMaxRoundsPerSlice - n + 1]++;  // bucket 0 = most rounds
    }
  for (int i = 1; i <= slg::kMaxRoundsPerSlice + 1; i++) hist[i] += hist[i - 1];
  const bool lpt = tn.slice_order != 0;
  for (size_t sidx = 0; sidx < out.slice_sq.size(); sidx++)
    out.slice_order[lpt ? hist[slg::kMaxRoundsPerSlice - nrounds[sidx]]++ : sidx] = (uint32_t)sidx;
}

// stitching: dst += src, which is spent (the first part is taken whole: one part = no copy)
template <typename T>
void append(std::vector<T> &dst, std::vector<T> &src) {
  if (dst.empty())
    dst.swap(src);
  else
    dst.insert(dst.end(), src.begin(), src.end());
}

template <typename T>
size_t place(size_t &cursor, size_t count) {
  cursor = (cursor + 15) & ~(size_t)15;
  const size_t at = cursor;
  cursor += count * sizeof(T);
  return at;
}

}  // namespace

void Plan::layout() {
  size_t cur = 0;
  o_sq = place<slg::RoundQuery>(cur, sqs.size());
  o_terms = place<slg::TermRef>(cur, terms.size());
  o_slice = place<uint32_t>(cur, slice_sq.size());
  o_sseg = place<uint32_t>(cur, slice_seg.size());
  o_sord = place<uint32_t>(cur, slice_order.size());
  o_q = place<slg::QueryRef>(cur, qrefs.size());
  o_bc = place<uint32_t>(cur, bnd_coarse.size());
  o_nodes = place<slg::PlanNode>(cur, nodes.size());
  image_bytes = (cur + 15) & ~(size_t)15;
}

void Plan::pack(unsigned char *hb) const {
  if (!sqs.empty()) std::memcpy(hb + o_sq, sqs.data(), sqs.size() * sizeof(slg::RoundQuery));
  if (!terms.empty()) std::memcpy(hb + o_terms, terms.data(), terms.size() * sizeof(slg::TermRef));
  if (!slice_sq.empty()) std::memcpy(hb + o_slice, slice_sq.data(), slice_sq.size() * 4);
  if (!slice_seg.empty()) std::memcpy(hb + o_sseg, slice_seg.data(), slice_seg.size() * 4);
  if (!slice_order.empty()) std::memcpy(hb + o_sord, slice_order.data(), slice_order.size() * 4);
  if (!qrefs.empty()) std::memcpy(hb + o_q, qrefs.data(), qrefs.size() * sizeof(slg::QueryRef));
  if (!bnd_coarse.empty()) std::memcpy(hb + o_bc, bnd_coarse.data(), bnd_coarse.size() * 4);
  if (!nodes.empty()) std::memcpy(hb + o_nodes, nodes.data(), nodes.size() * sizeof(slg::PlanNode));
}

void plan_batch(const std::vector<SegView> &segs, const slg_tuning &tn, const BatchIn &in, Plan &out) {
  struct Running {
    Running() { g_plans_running.fetch_add(1, std::memory_order_relaxed); }
    ~Running() { g_plans_running.fetch_sub(1, std::memory_order_relaxed); }
  } running;
  const uint32_t nq = in.nq, k = planning_k(in);
  const uint32_t n_segs = (uint32_t)segs.size();
  const BatchFacts facts = validate_batch(in);
  out = Plan();
  out.q_postings.assign(nq, 0);
  // MaxScore classification: on request, or (auto) for batches with a query of more than 4 terms
  const bool maxscore_on =
      tn.pruning >= 0 ? tn.pruning != 0 : facts.max_nt > std::min<uint32_t>(tn.uniform_max_terms, slg::kUniMaxLists);
  Pass1Ctx ctx{segs, tn, in, facts, maxscore_on, out.q_postings};

  // Pass 1 is per query: large batches (config 4: 8192 queries x 8 segments = 65K sub-queries,
  // 15 ms on one thread, mostly cache misses in the champion tables) are planned by several
  // threads, each into its own vectors, stitched together in query order afterwards.
  std::vector<SqCount> counts;
  double skip_est = 0.0;
  bool any_plan = false, any_filter = false;
  {
    uint32_t n_thr = 1;
    if ((uint64_t)nq * n_segs >= 8192) n_thr = std::max<uint32_t>(1, std::min<uint32_t>(planner_threads(), nq / 512));
    std::vector<Pass1Out> parts(n_thr);
    fan_out(nq, n_thr, [&](size_t t, size_t lo, size_t hi) { plan_queries(ctx, (uint32_t)lo, (uint32_t)hi, parts[t]); });
    for (Pass1Out &pt : parts) {
      const uint32_t term_base = (uint32_t)out.terms.size(), node_base = (uint32_t)out.nodes.size();
      if (term_base || node_base)
        for (auto &sq : pt.sqs) {
          sq.term_begin += term_base;
          if (sq.depth) sq.node_begin += node_base;
        }
      append(out.sqs, pt.sqs);
      append(out.terms, pt.terms);
      append(counts, pt.counts);
      append(out.nodes, pt.nodes);
      skip_est += pt.skip_est;
      out.n_postings += pt.n_postings;
      out.n_postings_essential += pt.n_ess;
      out.n_postings_nonessential += pt.n_postings - pt.n_ess;
      out.max_terms = std::max(out.max_terms, pt.max_terms);
      any_plan = any_plan || pt.any_plan;
      any_filter = any_filter || pt.any_filter;
      out.nested = out.nested || pt.any_nested;
      out.deep = out.deep || pt.any_deep;
    }
  }

  // Classified lists only pay through block skipping (the many-term kernel loads a non-essential
  // list as it loads any other; what it saves is the blocks without a candidate doc).  A batch the
  // few-term kernel could take keeps its classification only if the expected skipped postings are
  // worth the slower kernel (config 3: lists of similar density, nothing to skip -> few-term kernel;
  // a stop word next to rare terms: 74 % skipped -> many-term kernel).  slg_tuning.pruning = 1 keeps
  // the classification whatever the estimate.
  if (tn.pruning < 0 && out.max_terms <= tn.uniform_max_terms && !any_plan &&
      skip_est < 0.15 * (double)out.n_postings) {
    for (size_t i = 0; i < out.sqs.size(); i++) {
      slg::RoundQuery &sq = out.sqs[i];
      sq.ess_mask = full_mask(sq.n_terms);
      sq.skip_mask = 0;
      sq.longest = counts[i].longest_all;
      counts[i].ess = counts[i].all;
    }
    out.n_postings_essential = out.n_postings;
    out.n_postings_nonessential = 0;
  }
  // which kernel: the few-term kernel (slg_score_uni4.hpp) takes batches of <= 8 lists per sub-query
  // without non-essential lists — flat sums, and (its plan instantiation) flat score
  // plans: Sum / DisMax over leaves of one or more terms, i.e. every multi-field query string
  // (api/reader.rs:2576-2586: `fields: None` = all text fields).  Two-level plans, more lists and
  // classified batches run on the many-term kernel
  const bool plans_fit = !any_plan || (!out.nested && !out.deep && tn.uniform_plans != 0);
  out.uniform = out.max_terms <= tn.uniform_max_terms && plans_fit;
  if (facts.min_match && !out.uniform)
    throw SlgError(SLG_ERR_UNSUPPORTED,
                   "minimum_should_match > 1 needs a flat score plan and at most 8 scored lists per segment in every query "
                   "of the batch (the few-term kernel's plan instantiation)");
  for (const slg::RoundQuery &sq : out.sqs)
    if (sq.ess_mask != full_mask(sq.n_terms)) {
      out.pruned = true;
      out.uniform = false;
    }
  out.multi = !out.uniform;
  out.plan_batch = any_plan;
  // large k: per-slice top-k lists would be mostly the slice itself; keep every doc above the
  // seed threshold instead (one candidate slot per posting) and select per query afterwards
  out.cand_mode = k > 256;

  plan_rounds(segs, tn, k, counts, out);

  if (out.cand_mode)
    for (size_t i = 0; i < out.sqs.size(); i++) {
      out.sqs[i].cand_lo = (uint32_t)out.cand_total;
      out.sqs[i].cand_hi = (uint32_t)(out.cand_total >> 32);
      out.cand_total += counts[i].all;
    }
  out.qrefs.assign(nq, slg::QueryRef{0, 0});
  for (const slg::RoundQuery &sq : out.sqs) {  // (in query order; every sub-query has a slice)
    slg::QueryRef &qr = out.qrefs[sq.q];
    if (qr.slice_end == 0) qr.slice_begin = sq.slice_begin;
    qr.slice_end = sq.slice_begin + sq.n_slices;
  }
  order_slices(tn, out);
  // sub-query of every 32nd round boundary (partition_rounds_kernel walks from there)
  out.bnd_coarse.resize((size_t)((out.n_bnd + 31) / 32));
  {
    size_t i = 0;
    for (size_t c = 0; c < out.bnd_coarse.size(); c++) {
      const uint64_t bb = (uint64_t)c * 32;
      while (i + 1 < out.sqs.size() && out.sqs[i + 1].bnd_begin <= bb) i++;
      out.bnd_coarse[c] = (uint32_t)i;
    }
  }
  if (any_filter) {
    out.q_filter.assign(nq, 0u);
    for (uint32_t q = 0; q < nq; q++)
      if (in.q_filter[q] >= 0) out.q_filter[q] = (uint32_t)in.q_filter[q] + 1u;
  }
  out.layout();
}

// ---- query rescore ---------------------------------------------------------------------------------
static_assert(slg::kRescoreMaxWindow == SLG_MAX_RESCORE_WINDOW, "the kernel's rows per lane and the ABI's window limit");

void check_rescore(const slg_rescore_spec *spec, uint32_t nq, uint32_t k) {
  PLAN_REQUIRE(spec != nullptr, "rescore spec is NULL");
  if (nq == 0) return;
  PLAN_REQUIRE(spec->q_offsets != nullptr, "rescore q_offsets is NULL");
  PLAN_REQUIRE(spec->q_window != nullptr, "rescore q_window is NULL");
  const uint32_t total = spec->q_offsets[nq];
  PLAN_REQUIRE(total == 0 || (spec->q_term_ids && spec->q_weights), "rescore q_term_ids/q_weights is NULL");
  for (uint32_t q = 0; q < nq; q++) {
    const std::string in_q = " in rescore query " + std::to_string(q);
    PLAN_REQUIRE(spec->q_offsets[q + 1] >= spec->q_offsets[q] && spec->q_offsets[q + 1] <= total,
                 "rescore q_offsets not monotone");
    const uint32_t t0 = spec->q_offsets[q], nt = spec->q_offsets[q + 1] - t0;
    PLAN_REQUIRE(nt <= SLG_MAX_QUERY_TERMS, "more than " + std::to_string(SLG_MAX_QUERY_TERMS) + " terms" + in_q);
    const int32_t mode = spec->q_mode ? spec->q_mode[q] : SLG_RESCORE_TOTAL;
    PLAN_REQUIRE(mode >= SLG_RESCORE_TOTAL && mode <= SLG_RESCORE_MIN, "unknown score mode" + in_q);
    const int32_t plan = spec->q_plan ? spec->q_plan[q] : SLG_PLAN_SUM;
    PLAN_REQUIRE(plan == SLG_PLAN_SUM || plan == SLG_PLAN_DISMAX, "unknown score plan" + in_q);
    const float tie = spec->q_tie ? spec->q_tie[q] : 0.0f;
    PLAN_REQUIRE(tie >= 0.0f && tie <= 1.0f, "tie breaker outside [0, 1]" + in_q);  // (also: NaN)
    for (uint32_t i = 0; i < nt; i++) {
      PLAN_REQUIRE(std::isfinite(spec->q_weights[t0 + i]), "non-finite weight" + in_q);
      PLAN_REQUIRE(!spec->q_leaf || spec->q_leaf[t0 + i] < 0x80000000u, "leaf index >= 2^31" + in_q);
    }
  }
  for (uint32_t q = 0; q < nq; q++)
    if (std::min(spec->q_window[q], k) > SLG_MAX_RESCORE_WINDOW)  // (a window never reaches past the k rows)
      throw SlgError(SLG_ERR_UNSUPPORTED, "rescore window of query " + std::to_string(q) + " > SLG_MAX_RESCORE_WINDOW");
}

namespace {
// The list of term `tid` in a segment: off in the padded layout (SegDev), ubase its first posting in the
// unpadded order, df its length.  false (nothing written): SLG_NO_TERM, the segment has no such term.
// what: "rescore" / "bool" / "phrase", for the message of an id out of range
bool resolve_term(const SegView &sh, uint32_t tid, const char *what, uint32_t q, uint64_t &off, uint64_t &ubase,
                  uint32_t &df) {
  if (tid == SLG_NO_TERM) return false;
  PLAN_REQUIRE(tid < sh.n_terms, std::string("term id out of range in ") + what + " query " + std::to_string(q));
  ubase = sh.term_offsets[tid];
  off = ubase + (uint64_t)slg::kListPad * tid;
  df = (uint32_t)(sh.term_offsets[tid + 1] - ubase);
  return true;
}
bool clause_kind_known(int32_t kind) {
  return kind == SLG_BOOL_MUST || kind == SLG_BOOL_SHOULD || kind == SLG_BOOL_MUST_NOT;
}
// a bool or phrase batch states its minimum in q_min_should: the score plans must not state one too
void require_no_min_match(const slg_score_plans *plans, uint32_t q, const char *what, const std::string &in_q) {
  PLAN_REQUIRE(!plans || !plans->q_min_match || plans->q_min_match[q] <= 1u,
               std::string("q_min_match > 1 in the score plans of a ") + what + " batch (q_min_should states it)" + in_q);
}
}  // namespace

void plan_rescore(const std::vector<SegView> &segs, uint32_t nq, uint32_t k, const slg_rescore_spec &spec,
                  RescorePlan &out) {
  const uint32_t n_segs = (uint32_t)segs.size();
  out.queries.assign(nq, slg::RescoreQuery{});
  out.terms.clear();
  out.terms.reserve((size_t)(nq ? spec.q_offsets[nq] : 0) * n_segs);
  for (uint32_t q = 0; q < nq; q++) {
    const uint32_t t0 = spec.q_offsets[q], nt = spec.q_offsets[q + 1] - t0;
    slg::RescoreQuery &rq = out.queries[q];
    rq.term_begin = t0;
    rq.n_terms = nt;
    rq.window = spec.q_window[q];
    rq.mode = spec.q_mode ? (uint32_t)spec.q_mode[q] : (uint32_t)SLG_RESCORE_TOTAL;
    rq.plan = spec.q_plan && spec.q_plan[q] == SLG_PLAN_DISMAX ? 1u : 0u;
    rq.tie = spec.q_tie ? spec.q_tie[q] : 0.0f;
    rq.n_leaves = spec.q_nleaves ? spec.q_nleaves[q] : 0u;
    rq.min_match = std::max(spec.q_min_match ? spec.q_min_match[q] : 0u, 1u);
    if ((uint64_t)nt * n_segs > slg::kRescoreMaxTable)
      throw SlgError(SLG_ERR_UNSUPPORTED, "rescore query " + std::to_string(q) + ": terms x segments exceed " +
                                              std::to_string(slg::kRescoreMaxTable) + " table entries");
    // the query's terms by leaf (stable: a leaf's terms keep the term order their scores are added in)
    uint32_t order[SLG_MAX_QUERY_TERMS];
    for (uint32_t i = 0; i < nt; i++) {
      order[i] = i;
      rq.n_leaves = std::max(rq.n_leaves, (spec.q_leaf ? spec.q_leaf[t0 + i] : i) + 1u);
    }
    if (spec.q_leaf)
      std::stable_sort(order, order + nt,
                       [&](uint32_t a, uint32_t b) { return spec.q_leaf[t0 + a] < spec.q_leaf[t0 + b]; });
    for (uint32_t j = 0; j < nt; j++) {
      const uint32_t i = order[j];
      for (uint32_t s = 0; s < n_segs; s++) {
        slg::RescoreTerm rt{};
        rt.weight = spec.q_weights[t0 + i];
        rt.leaf = spec.q_leaf ? spec.q_leaf[t0 + i] : i;
        uint64_t ubase;
        resolve_term(segs[s], spec.q_term_ids[(size_t)(t0 + i) * n_segs + s], "rescore", q, rt.off, ubase, rt.df);
        out.terms.push_back(rt);
      }
    }
    if (nt) {
      out.max_window = std::max(out.max_window, std::min(rq.window, k));
      out.max_table = std::max(out.max_table, nt * n_segs);
    }
  }
}

// ---- boolean queries -------------------------------------------------------------------------------
static_assert(slg::kBoolMaxGroups == SLG_MAX_BOOL_GROUPS && slg::kBoolMaxTerms == SLG_MAX_BOOL_TERMS,
              "the kernel's group masks and the ABI's limits");

void check_bool(const slg_bool_spec *spec, uint32_t nq, const slg_score_plans *plans) {
  PLAN_REQUIRE(spec != nullptr, "bool spec is NULL");
  if (nq == 0) return;
  PLAN_REQUIRE(spec->c_offsets != nullptr, "bool c_offsets is NULL");
  PLAN_REQUIRE(spec->g_offsets != nullptr, "bool g_offsets is NULL");
  for (uint32_t q = 0; q < nq; q++) {
    PLAN_REQUIRE(spec->c_offsets[q + 1] >= spec->c_offsets[q], "bool c_offsets not monotone");
    PLAN_REQUIRE(spec->g_offsets[q + 1] >= spec->g_offsets[q], "bool g_offsets not monotone");
  }
  PLAN_REQUIRE(spec->c_offsets[nq] == spec->c_offsets[0] || (spec->c_term_ids && spec->c_group),
               "bool c_term_ids/c_group is NULL");
  PLAN_REQUIRE(spec->g_offsets[nq] == spec->g_offsets[0] || spec->g_kind, "bool g_kind is NULL");
  for (uint32_t q = 0; q < nq; q++) {
    const std::string in_q = " in bool query " + std::to_string(q);
    const uint32_t t0 = spec->c_offsets[q], nt = spec->c_offsets[q + 1] - t0;
    const uint32_t g0 = spec->g_offsets[q], ng = spec->g_offsets[q + 1] - g0;
    uint32_t next = 0;  // the group a new group's first term must name
    for (uint32_t i = 0; i < nt; i++) {
      const uint32_t g = spec->c_group[t0 + i];
      PLAN_REQUIRE(g < ng, "c_group names a group the query does not have" + in_q);
      PLAN_REQUIRE(g == next || (next > 0 && g == next - 1), "c_group decreases or skips a group" + in_q);
      if (g == next) next++;
    }
    PLAN_REQUIRE(next == ng, "a group without a term" + in_q);
    for (uint32_t g = 0; g < ng; g++) {
      const int32_t kind = spec->g_kind[g0 + g];
      PLAN_REQUIRE(clause_kind_known(kind), "unknown clause kind" + in_q);
    }
    require_no_min_match(plans, q, "bool", in_q);
  }
  for (uint32_t q = 0; q < nq; q++) {
    if (spec->g_offsets[q + 1] - spec->g_offsets[q] > SLG_MAX_BOOL_GROUPS)
      throw SlgError(SLG_ERR_UNSUPPORTED, "bool query " + std::to_string(q) + " has more than SLG_MAX_BOOL_GROUPS groups");
    if (spec->c_offsets[q + 1] - spec->c_offsets[q] > SLG_MAX_BOOL_TERMS)
      throw SlgError(SLG_ERR_UNSUPPORTED, "bool query " + std::to_string(q) + " has more than SLG_MAX_BOOL_TERMS clause terms");
  }
}

void plan_bool(const std::vector<SegView> &segs, uint32_t nq, const slg_bool_spec &spec, BoolPlan &out) {
  const uint32_t n_segs = (uint32_t)segs.size();
  out.queries.assign(nq, slg::BoolQuery{});
  out.terms.clear();
  out.n_groups = 0;
  if (nq == 0) return;
  const uint32_t c_base = spec.c_offsets[0];
  out.terms.reserve((size_t)(spec.c_offsets[nq] - c_base) * n_segs);
  for (uint32_t q = 0; q < nq; q++) {
    const uint32_t t0 = spec.c_offsets[q], nt = spec.c_offsets[q + 1] - t0;
    const uint32_t g0 = spec.g_offsets[q], ng = spec.g_offsets[q + 1] - g0;
    slg::BoolQuery &bq = out.queries[q];
    bq.term_begin = t0 - c_base;
    bq.n_terms = nt;
    bq.min_should = ng && spec.q_min_should ? spec.q_min_should[q] : 0u;
    out.n_groups += ng;
    for (uint32_t g = 0; g < ng; g++) {
      const int32_t kind = spec.g_kind[g0 + g];
      (kind == SLG_BOOL_MUST ? bq.must_mask : kind == SLG_BOOL_MUST_NOT ? bq.must_not_mask : bq.should_mask) |= 1u << g;
    }
    // the row's order: MUST, MUST_NOT, SHOULD (stable inside a kind)
    uint32_t order[SLG_MAX_BOOL_TERMS], n = 0;
    for (const int32_t kind : {SLG_BOOL_MUST, SLG_BOOL_MUST_NOT, SLG_BOOL_SHOULD}) {
      for (uint32_t i = 0; i < nt; i++)
        if (spec.g_kind[g0 + spec.c_group[t0 + i]] == kind) order[n++] = i;
      if (kind == SLG_BOOL_MUST) bq.n_must = n;
      if (kind == SLG_BOOL_MUST_NOT) bq.n_must_not = n - bq.n_must;
    }
    for (uint32_t s = 0; s < n_segs; s++) {
      for (uint32_t j = 0; j < nt; j++) {
        const uint32_t i = order[j];
        slg::BoolTerm bt{};
        bt.group = spec.c_group[t0 + i];
        uint64_t ubase;
        resolve_term(segs[s], spec.c_term_ids[(size_t)(t0 + i) * n_segs + s], "bool", q, bt.off, ubase, bt.df);
        out.terms.push_back(bt);
      }
    }
  }
}

// ---- phrase queries ---------------------------------------------------------------------------------
static_assert(slg::kPhraseMaxTerms == SLG_MAX_PHRASE_TERMS && slg::kPhraseMaxVariants == SLG_MAX_PHRASE_VARIANTS &&
                  slg::kPhraseMaxQueryTerms == SLG_MAX_PHRASE_QUERY_TERMS && slg::kPhraseMaxSlop == SLG_MAX_PHRASE_SLOP,
              "the kernel's unrolled cursors and span arithmetic and the ABI's limits");

void check_positions(uint64_t n_postings, const uint64_t *pos_offsets, const uint32_t *positions) {
  PLAN_REQUIRE(pos_offsets != nullptr, "pos_offsets is NULL");
  PLAN_REQUIRE(pos_offsets[0] == 0, "pos_offsets does not start at 0");
  for (uint64_t i = 0; i < n_postings; i++)
    PLAN_REQUIRE(pos_offsets[i + 1] >= pos_offsets[i], "pos_offsets not monotone");
  const uint64_t total = pos_offsets[n_postings];
  if (total > 0xFFFFFFFFull)
    throw SlgError(SLG_ERR_UNSUPPORTED, "more than 2^32 - 1 positions in a segment");
  PLAN_REQUIRE(total == 0 || positions != nullptr, "positions is NULL");
  for (uint64_t i = 0; i < n_postings; i++) {
    uint32_t prev = 0;
    for (uint64_t j = pos_offsets[i]; j < pos_offsets[i + 1]; j++) {
      const uint32_t v = positions[j];
      PLAN_REQUIRE(v < slg::kPositionEnd, "a position is >= 2^31 (posting " + std::to_string(i) + ")");
      PLAN_REQUIRE(v >= prev, "positions decrease inside posting " + std::to_string(i));
      prev = v;
    }
  }
}

void check_phrase(const slg_bool_spec *boolean, const slg_phrase_spec *spec, uint32_t nq, const slg_score_plans *plans) {
  PLAN_REQUIRE(spec != nullptr, "phrase spec is NULL");
  PLAN_REQUIRE(!boolean || boolean->q_min_should == nullptr,
               "bool q_min_should beside a phrase spec (the phrase spec's q_min_should states it)");
  if (nq != 0) {
    PLAN_REQUIRE(spec->p_offsets != nullptr, "phrase p_offsets is NULL");
    for (uint32_t q = 0; q < nq; q++)
      PLAN_REQUIRE(spec->p_offsets[q + 1] >= spec->p_offsets[q], "phrase p_offsets not monotone");
    const uint32_t p0 = spec->p_offsets[0], p1 = spec->p_offsets[nq];
    if (p1 > p0) {
      PLAN_REQUIRE(spec->p_kind && spec->p_slop, "phrase p_kind/p_slop is NULL");
      PLAN_REQUIRE(spec->v_offsets != nullptr, "phrase v_offsets is NULL");
      for (uint32_t p = p0; p < p1; p++)
        PLAN_REQUIRE(spec->v_offsets[p + 1] >= spec->v_offsets[p], "phrase v_offsets not monotone");
      const uint32_t v0 = spec->v_offsets[p0], v1 = spec->v_offsets[p1];
      if (v1 > v0) {
        PLAN_REQUIRE(spec->t_offsets != nullptr, "phrase t_offsets is NULL");
        for (uint32_t v = v0; v < v1; v++) {
          PLAN_REQUIRE(spec->t_offsets[v + 1] >= spec->t_offsets[v], "phrase t_offsets not monotone");
          PLAN_REQUIRE(spec->t_offsets[v + 1] > spec->t_offsets[v], "a phrase variant without a term");
        }
        PLAN_REQUIRE(spec->t_term_ids != nullptr, "phrase t_term_ids is NULL");
      }
      for (uint32_t p = p0; p < p1; p++) {
        const int32_t kind = spec->p_kind[p];
        PLAN_REQUIRE(clause_kind_known(kind), "unknown phrase kind (phrase " + std::to_string(p) + ")");
      }
    }
    for (uint32_t q = 0; q < nq; q++) require_no_min_match(plans, q, "phrase", " in query " + std::to_string(q));
  }
  if (boolean) check_bool(boolean, nq, plans);
  for (uint32_t q = 0; q < nq; q++) {
    const std::string in_q = "phrase query " + std::to_string(q);
    const uint32_t p0 = spec->p_offsets[q], p1 = spec->p_offsets[q + 1];
    uint64_t q_terms = 0;
    for (uint32_t p = p0; p < p1; p++) {
      const uint32_t v0 = spec->v_offsets[p], v1 = spec->v_offsets[p + 1];
      if (v1 - v0 > SLG_MAX_PHRASE_VARIANTS)
        throw SlgError(SLG_ERR_UNSUPPORTED, in_q + " has a phrase of more than SLG_MAX_PHRASE_VARIANTS variants");
      for (uint32_t v = v0; v < v1; v++) {
        const uint32_t n = spec->t_offsets[v + 1] - spec->t_offsets[v];
        if (n > SLG_MAX_PHRASE_TERMS)
          throw SlgError(SLG_ERR_UNSUPPORTED, in_q + " has a variant of more than SLG_MAX_PHRASE_TERMS terms");
        q_terms += n;
      }
      if (spec->p_slop[p] > SLG_MAX_PHRASE_SLOP)
        throw SlgError(SLG_ERR_UNSUPPORTED, in_q + " has a slop above SLG_MAX_PHRASE_SLOP");
    }
    if (q_terms > SLG_MAX_PHRASE_QUERY_TERMS)
      throw SlgError(SLG_ERR_UNSUPPORTED, in_q + " has more than SLG_MAX_PHRASE_QUERY_TERMS variant terms");
    const uint32_t n_tg = boolean ? boolean->g_offsets[q + 1] - boolean->g_offsets[q] : 0u;
    if ((uint64_t)n_tg + (p1 - p0) > SLG_MAX_BOOL_GROUPS)
      throw SlgError(SLG_ERR_UNSUPPORTED, in_q + " has more than SLG_MAX_BOOL_GROUPS term and phrase groups");
  }
}

void plan_phrase(const std::vector<SegView> &segs, uint32_t nq, const slg_bool_spec *boolean, const slg_phrase_spec &spec,
                 PhrasePlan &out) {
  const uint32_t n_segs = (uint32_t)segs.size();
  if (boolean) {
    plan_bool(segs, nq, *boolean, out.bools);
  } else {
    out.bools.queries.assign(nq, slg::BoolQuery{});
    out.bools.terms.clear();
    out.bools.n_groups = 0;
  }
  out.queries.assign(nq, slg::PhraseQuery{});
  out.vars.clear();
  out.terms.clear();
  uint32_t term_begin = 0;
  for (uint32_t q = 0; q < nq; q++) {
    const uint32_t p0 = spec.p_offsets[q], np = spec.p_offsets[q + 1] - p0;
    const uint32_t n_tg = boolean ? boolean->g_offsets[q + 1] - boolean->g_offsets[q] : 0u;
    slg::BoolQuery &bq = out.bools.queries[q];
    slg::PhraseQuery &pq = out.queries[q];
    bq.min_should = (n_tg + np) && spec.q_min_should ? spec.q_min_should[q] : 0u;
    out.bools.n_groups += np;
    pq.n_term_groups = n_tg;
    pq.var_begin = (uint32_t)out.vars.size();
    pq.term_begin = term_begin;
    // where each variant's terms start in the row (the spec's order), then the variants by kind
    uint32_t t_begin[SLG_MAX_BOOL_GROUPS][SLG_MAX_PHRASE_VARIANTS], n_terms = 0;
    for (uint32_t pi = 0; pi < np; pi++)
      for (uint32_t v = spec.v_offsets[p0 + pi]; v < spec.v_offsets[p0 + pi + 1]; v++) {
        t_begin[pi][v - spec.v_offsets[p0 + pi]] = n_terms;
        n_terms += spec.t_offsets[v + 1] - spec.t_offsets[v];
      }
    pq.n_terms = n_terms;
    for (const int32_t kind : {SLG_BOOL_MUST, SLG_BOOL_MUST_NOT, SLG_BOOL_SHOULD})
      for (uint32_t pi = 0; pi < np; pi++) {
        if (spec.p_kind[p0 + pi] != kind) continue;
        const uint32_t g = n_tg + pi;
        (kind == SLG_BOOL_MUST ? bq.must_mask : kind == SLG_BOOL_MUST_NOT ? bq.must_not_mask : bq.should_mask) |= 1u << g;
        const uint32_t v0 = spec.v_offsets[p0 + pi], v1 = spec.v_offsets[p0 + pi + 1];
        for (uint32_t v = v0; v < v1; v++) {
          slg::PhraseVar pv{};
          pv.t_begin = t_begin[pi][v - v0];
          pv.n_last = (spec.t_offsets[v + 1] - spec.t_offsets[v]) | (v + 1 == v1 ? 0x100u : 0u);
          pv.group = g;
          pv.slop = spec.p_slop[p0 + pi];
          out.vars.push_back(pv);
        }
      }
    pq.n_vars = (uint32_t)out.vars.size() - pq.var_begin;
    for (uint32_t s = 0; s < n_segs; s++) {
      const SegView &sh = segs[s];
      for (uint32_t pi = 0; pi < np; pi++)
        for (uint32_t v = spec.v_offsets[p0 + pi]; v < spec.v_offsets[p0 + pi + 1]; v++) {
          const uint32_t t0 = spec.t_offsets[v], n = spec.t_offsets[v + 1] - t0;
          bool survives = sh.has_positions;  // (no positions: every posting's position list is empty)
          slg::PhraseTerm row[SLG_MAX_PHRASE_TERMS];
          for (uint32_t i = 0; i < n; i++) {
            row[i] = slg::PhraseTerm{};
            survives = resolve_term(sh, spec.t_term_ids[(size_t)(t0 + i) * n_segs + s], "phrase", q, row[i].off,
                                    row[i].ubase, row[i].df) &&
                       survives && row[i].df != 0;
          }
          for (uint32_t i = 0; i < n; i++) {
            if (!survives) row[i].df = 0;  // dropped in this segment: the kernel reads the first term's df
            out.terms.push_back(row[i]);
          }
        }
    }
    term_begin += n_terms;
  }
}

// ---- function_score ------------------------------------------------------------------------------------
static_assert(slg::kFscoreMaxFuncs == SLG_MAX_FSCORE_FUNCS, "the kernel's limit and the ABI's");
static_assert(sizeof(slg::FscoreQuery) == 32 && sizeof(slg::FscoreFn) == 64, "records the kernel reads in whole words");

// ---- field collapsing ------------------------------------------------------------------------------
void check_collapse(const slg_collapse_spec *spec, uint32_t k) {
  PLAN_REQUIRE(spec != nullptr, "collapse spec is NULL");
  PLAN_REQUIRE(spec->group_limit >= 1, "collapse group_limit is 0");
  PLAN_REQUIRE(spec->group_limit <= k, "collapse group_limit > k");
  if (const slg_sort_spec *in = spec->inner_sort) {
    for (uint32_t i = 0; i < std::min<uint32_t>(in->n_parts, SLG_MAX_SORT_PARTS); i++) {
      PLAN_REQUIRE(in->order[i] == SLG_ORDER_ASC || in->order[i] == SLG_ORDER_DESC,
                   "unknown sort order in inner sort part " + std::to_string(i));
      PLAN_REQUIRE(in->field[i] >= 0 || in->field[i] == SLG_SORT_SCORE,
                   "unknown sort field id in inner sort part " + std::to_string(i));
    }
  }
  if (k > SLG_MAX_COLLAPSE_ROWS) throw SlgError(SLG_ERR_UNSUPPORTED, "collapse batch with k > SLG_MAX_COLLAPSE_ROWS");
  if (spec->inner_size > 0 && (uint64_t)spec->inner_from + spec->inner_size > SLG_MAX_INNER_HITS)
    throw SlgError(SLG_ERR_UNSUPPORTED, "collapse inner_from + inner_size > SLG_MAX_INNER_HITS");
  if (spec->inner_sort && spec->inner_sort->n_parts > SLG_MAX_SORT_PARTS)
    throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_SORT_PARTS inner sort parts");
}

// ---- top_hits ------------------------------------------------------------------------------------------
void check_top_hits(const slg_top_hits_spec *spec, const slg_agg_spec *aggs) {
  PLAN_REQUIRE(spec != nullptr, "top_hits spec is NULL");
  PLAN_REQUIRE(spec->n_nodes >= 1, "a top_hits spec needs at least one node");
  const uint32_t nn = std::min<uint32_t>(spec->n_nodes, SLG_MAX_TOP_HITS_NODES);
  auto name = [](uint32_t i) { return "top_hits node " + std::to_string(i); };
  for (uint32_t i = 0; i < nn; i++) {
    const slg_top_hits_node &n = spec->nodes[i];
    if (n.parent != -1) {
      PLAN_REQUIRE(aggs != nullptr, name(i) + ": a child node needs an aggregation spec");
      PLAN_REQUIRE(n.parent >= 0 && (uint32_t)n.parent < aggs->n_nodes && (uint32_t)n.parent < SLG_MAX_AGGS,
                   name(i) + ": parent is not a node of the aggregation spec");
      const int32_t kind = aggs->nodes[n.parent].kind;
      PLAN_REQUIRE(kind == SLG_AGG_TERMS || kind == SLG_AGG_HISTOGRAM || kind == SLG_AGG_RANGE ||
                       kind == SLG_AGG_DATE_HISTOGRAM || kind == SLG_AGG_FILTER,
                   name(i) + ": parent is not a bucket node (terms, histogram, range, date_histogram, filter)");
    }
    for (uint32_t j = 0; j < std::min<uint32_t>(n.sort.n_parts, SLG_MAX_SORT_PARTS); j++) {
      PLAN_REQUIRE(n.sort.order[j] == SLG_ORDER_ASC || n.sort.order[j] == SLG_ORDER_DESC,
                   name(i) + ": unknown sort order in part " + std::to_string(j));
      PLAN_REQUIRE(n.sort.field[j] >= 0 || n.sort.field[j] == SLG_SORT_SCORE,
                   name(i) + ": unknown sort field id in part " + std::to_string(j));
    }
  }
  if (spec->n_nodes > SLG_MAX_TOP_HITS_NODES)
    throw SlgError(SLG_ERR_UNSUPPORTED, "more than SLG_MAX_TOP_HITS_NODES top_hits nodes");
  for (uint32_t i = 0; i < nn; i++) {
    const slg_top_hits_node &n = spec->nodes[i];
    if (n.size == 0) throw SlgError(SLG_ERR_UNSUPPORTED, name(i) + ": size is 0 (nothing to select: CPU path)");
    if ((uint64_t)n.from + n.size > SLG_MAX_TOP_HITS)
      throw SlgError(SLG_ERR_UNSUPPORTED, name(i) + ": from + size > SLG_MAX_TOP_HITS (CPU path)");
    if (n.sort.n_parts > SLG_MAX_SORT_PARTS)
      throw SlgError(SLG_ERR_UNSUPPORTED, name(i) + ": more than SLG_MAX_SORT_PARTS sort parts");
    if (n.parent != -1 && aggs->nodes[n.parent].parent != -1)
      throw SlgError(SLG_ERR_UNSUPPORTED, name(i) + ": parent is itself a child (a third level: CPU path)");
  }
}

void check_fscore(const slg_fscore_spec *spec, uint32_t nq) {
  PLAN_REQUIRE(spec != nullptr, "fscore spec is NULL");
  if (nq == 0) return;
  PLAN_REQUIRE(spec->q_fn_offsets != nullptr, "fscore q_fn_offsets is NULL");
  PLAN_REQUIRE(spec->q_score_mode && spec->q_boost_mode, "fscore q_score_mode/q_boost_mode is NULL");
  PLAN_REQUIRE(spec->q_flags != nullptr, "fscore q_flags is NULL");
  PLAN_REQUIRE(spec->q_boost != nullptr, "fscore q_boost is NULL");
  for (uint32_t q = 0; q < nq; q++)
    PLAN_REQUIRE(spec->q_fn_offsets[q + 1] >= spec->q_fn_offsets[q], "fscore q_fn_offsets not monotone");
  const uint32_t f_lo = spec->q_fn_offsets[0], f_hi = spec->q_fn_offsets[nq];
  PLAN_REQUIRE(f_hi == f_lo || (spec->f_kind && spec->f_field && spec->f_filter && spec->f_weight && spec->f_modifier &&
                                spec->f_decay_fn && spec->f_missing && spec->f_origin && spec->f_scale && spec->f_offset &&
                                spec->f_decay),
               "an fscore f_ array is NULL");
  for (uint32_t q = 0; q < nq; q++) {
    const std::string in_q = " in fscore query " + std::to_string(q);
    const int32_t sm = spec->q_score_mode[q], bm = spec->q_boost_mode[q];
    PLAN_REQUIRE(sm >= SLG_FSCORE_MODE_SUM && sm <= SLG_FSCORE_MODE_AVG, "unknown score mode" + in_q);
    PLAN_REQUIRE(bm >= SLG_FSCORE_BOOST_MULTIPLY && bm <= SLG_FSCORE_BOOST_MIN, "unknown boost mode" + in_q);
    const uint32_t flags = spec->q_flags[q];
    PLAN_REQUIRE((flags & ~(SLG_FSCORE_HAS_MAX_BOOST | SLG_FSCORE_HAS_MIN_SCORE)) == 0u, "unknown flag" + in_q);
    PLAN_REQUIRE(!(flags & SLG_FSCORE_HAS_MAX_BOOST) || spec->q_max_boost, "fscore q_max_boost is NULL");
    PLAN_REQUIRE(!(flags & SLG_FSCORE_HAS_MIN_SCORE) || spec->q_min_score, "fscore q_min_score is NULL");
    for (uint32_t f = spec->q_fn_offsets[q]; f < spec->q_fn_offsets[q + 1]; f++) {
      const int32_t kind = spec->f_kind[f];
      PLAN_REQUIRE(kind >= SLG_FSCORE_WEIGHT && kind <= SLG_FSCORE_DECAY, "unknown function kind" + in_q);
      PLAN_REQUIRE(spec->f_filter[f] >= -1, "negative filter id other than -1" + in_q);
      if (kind != SLG_FSCORE_DECAY)
        PLAN_REQUIRE(std::isfinite(spec->f_weight[f]),
                     (kind == SLG_FSCORE_WEIGHT ? "non-finite weight" : "non-finite factor") + in_q);
      if (kind == SLG_FSCORE_FIELD_VALUE_FACTOR) {
        const int32_t m = spec->f_modifier[f];
        PLAN_REQUIRE(m >= SLG_FSCORE_MOD_NONE && m <= SLG_FSCORE_MOD_RECIPROCAL, "unknown modifier" + in_q);
      }
      if (kind == SLG_FSCORE_DECAY) {
        const int32_t d = spec->f_decay_fn[f];
        PLAN_REQUIRE(d >= SLG_FSCORE_DECAY_EXP && d <= SLG_FSCORE_DECAY_LINEAR, "unknown decay function" + in_q);
        PLAN_REQUIRE(std::isfinite(spec->f_scale[f]), "decay scale must be finite" + in_q);
        PLAN_REQUIRE(spec->f_scale[f] > 0.0, "decay scale must be > 0" + in_q);
        PLAN_REQUIRE(spec->f_decay[f] > 0.0 && spec->f_decay[f] <= 1.0, "decay factor outside (0, 1]" + in_q);  // (also: NaN)
      }
    }
  }
  for (uint32_t q = 0; q < nq; q++)
    if (spec->q_fn_offsets[q + 1] - spec->q_fn_offsets[q] > SLG_MAX_FSCORE_FUNCS)
      throw SlgError(SLG_ERR_UNSUPPORTED, "fscore query " + std::to_string(q) + " has more than SLG_MAX_FSCORE_FUNCS functions");
}

// ---- registered aggregation fields (function_score, filter trees; aggregations and collapse on the device side) ----
const FscoreFieldView &agg_field(const std::vector<FscoreFieldView> &fields, int32_t id, const std::string &before,
                                 const std::string &after) {
  const auto it = std::find_if(fields.begin(), fields.end(), [id](const FscoreFieldView &v) { return v.id == id; });
  PLAN_REQUIRE(it != fields.end(), before + "unknown agg field id " + std::to_string(id) + after);
  return *it;
}
const slg::ColumnDev *agg_field_rows(const FscoreFieldView &field, uint32_t n_segs, const std::string &before,
                                     const std::string &after) {
  for (uint32_t s = 0; s < n_segs; s++)
    PLAN_REQUIRE(s < field.per_seg.size() && field.per_seg[s].vals != nullptr,
                 before + "agg field " + std::to_string(field.id) + " has no column for segment " + std::to_string(s) +
                     " (added after the field was registered)" + after);
  return field.per_seg.data();
}

namespace {
// the row of `id` in a table whose rows are numbered in order of first use
uint32_t row_of(std::vector<int32_t> &rows, int32_t id) {
  const auto it = std::find(rows.begin(), rows.end(), id);
  if (it != rows.end()) return (uint32_t)(it - rows.begin());
  rows.push_back(id);
  return (uint32_t)rows.size() - 1u;
}
// the two tables of such rows: the columns of the (checked) fields and the reject bitmaps of the filters, [row][n_segs]
void fill_tables(const std::vector<FscoreFieldView> &fields, const std::vector<int32_t> &used_fields,
                 const uint32_t *const *reject, const std::vector<int32_t> &used_filters, uint32_t n_segs,
                 std::vector<slg::ColumnDev> &cols, std::vector<const uint32_t *> &filters) {
  for (const int32_t id : used_fields) {
    const slg::ColumnDev *rows = agg_field_rows(agg_field(fields, id, "", ""), n_segs, "", "");
    cols.insert(cols.end(), rows, rows + n_segs);
  }
  for (const int32_t f : used_filters) filters.insert(filters.end(), reject + (size_t)f * n_segs, reject + ((size_t)f + 1) * n_segs);
}
}  // namespace

void plan_fscore(const std::vector<FscoreFieldView> &fields, const uint32_t *const *reject, const char *filter_live,
                 size_t n_filters, uint32_t n_segs, uint32_t nq, const slg_fscore_spec &spec, FscorePlan &out) {
  out = FscorePlan{};
  out.queries.assign(nq, slg::FscoreQuery{});
  if (nq == 0) return;
  const uint32_t f_base = spec.q_fn_offsets[0];
  std::vector<int32_t> used_fields, used_filters;  // the rows of the two tables, in order of first use
  std::string unsupported;                         // (reported behind every invalid argument)
  for (uint32_t q = 0; q < nq; q++) {
    const std::string in_q = " in fscore query " + std::to_string(q);
    const uint32_t f0 = spec.q_fn_offsets[q], nf = spec.q_fn_offsets[q + 1] - f0;
    slg::FscoreQuery &fq = out.queries[q];
    const uint32_t flags = spec.q_flags[q];
    fq.fn_begin = f0 - f_base;
    fq.n_fns = nf;
    fq.modes = (uint32_t)spec.q_score_mode[q] | ((uint32_t)spec.q_boost_mode[q] << 8) | (flags << 16);
    fq.max_boost = (flags & SLG_FSCORE_HAS_MAX_BOOST) ? spec.q_max_boost[q] : 0.0f;
    fq.min_score = (flags & SLG_FSCORE_HAS_MIN_SCORE) ? spec.q_min_score[q] : 0.0f;
    fq.boost = spec.q_boost[q];
    fq.work = (nf != 0u || flags != 0u || !(fq.boost == 1.0f)) ? 1u : 0u;
    out.n_work += fq.work;
    for (uint32_t f = f0; f < f0 + nf; f++) {
      slg::FscoreFn fn{};
      const int32_t kind = spec.f_kind[f];
      fn.kinds = (uint32_t)kind;
      fn.weight = spec.f_weight[f];
      fn.field = kind != SLG_FSCORE_WEIGHT ? spec.f_field[f] : -1;
      if (spec.f_filter[f] >= 0) {
        PLAN_REQUIRE((size_t)spec.f_filter[f] < n_filters && filter_live[spec.f_filter[f]],
                     "unknown filter id " + std::to_string(spec.f_filter[f]) + in_q);
        fn.filter = row_of(used_filters, spec.f_filter[f]) + 1u;
      }
      if (kind != SLG_FSCORE_WEIGHT) {
        const int32_t id = spec.f_field[f];
        const FscoreFieldView &fv = agg_field(fields, id, "", in_q);
        PLAN_REQUIRE(!fv.keyword, "agg field " + std::to_string(id) + " is a keyword field" + in_q);
        agg_field_rows(fv, n_segs, "", "");
        if (fv.non_finite && unsupported.empty())
          unsupported = "agg field " + std::to_string(id) + " holds a non-finite value (CPU path)" + in_q;
        fn.col = row_of(used_fields, id);
      }
      if (kind == SLG_FSCORE_FIELD_VALUE_FACTOR) {
        const int32_t m = spec.f_modifier[f];
        fn.kinds |= (uint32_t)m << 8;
        fn.missing = spec.f_missing[f];
        out.full = out.full || m == SLG_FSCORE_MOD_LOG || m == SLG_FSCORE_MOD_LOG1P || m == SLG_FSCORE_MOD_LOG2P;
      } else if (kind == SLG_FSCORE_DECAY) {
        const int32_t d = spec.f_decay_fn[f];
        fn.kinds |= (uint32_t)d << 16;
        fn.origin = spec.f_origin[f];
        fn.scale = spec.f_scale[f];
        fn.offset = spec.f_offset[f];
        fn.decay = spec.f_decay[f];
        out.full = out.full || d != SLG_FSCORE_DECAY_LINEAR;
      }
      out.fns.push_back(fn);
    }
  }
  if (!unsupported.empty()) throw SlgError(SLG_ERR_UNSUPPORTED, unsupported);
  fill_tables(fields, used_fields, reject, used_filters, n_segs, out.cols, out.filters);
}

// ---- scan batches ------------------------------------------------------------------------------------------
static_assert(slg::kScanMatchAll == SLG_SCAN_MATCH_ALL && slg::kScanConstant == SLG_SCAN_CONSTANT &&
                  slg::kScanRankFeature == SLG_SCAN_RANK_FEATURE, "header kinds");
static_assert(slg::kScanModNone == SLG_SCAN_MOD_NONE && slg::kScanModLog == SLG_SCAN_MOD_LOG &&
                  slg::kScanModLog1p == SLG_SCAN_MOD_LOG1P && slg::kScanModSqrt == SLG_SCAN_MOD_SQRT &&
                  slg::kScanModReciprocal == SLG_SCAN_MOD_RECIPROCAL, "header modifiers");
static_assert(sizeof(slg::ScanQuery) == 32 && sizeof(slg::ScanSlice) == 32, "records the kernel reads in whole words");

void check_scan(const slg_scan_spec *spec, uint32_t nq, uint32_t k) {
  PLAN_REQUIRE(spec != nullptr, "scan spec is NULL");
  if (nq != 0) {
    PLAN_REQUIRE(spec->q_kind != nullptr, "scan q_kind is NULL");
    PLAN_REQUIRE(spec->q_filter != nullptr, "scan q_filter is NULL");
    PLAN_REQUIRE(spec->q_score != nullptr, "scan q_score is NULL");
    PLAN_REQUIRE(spec->q_field && spec->q_modifier && spec->q_missing && spec->q_boost,
                 "scan q_field/q_modifier/q_missing/q_boost is NULL");
  }
  for (uint32_t q = 0; q < nq; q++) {
    const std::string in_q = " in scan query " + std::to_string(q);
    const int32_t kind = spec->q_kind[q];
    PLAN_REQUIRE(kind >= SLG_SCAN_MATCH_ALL && kind <= SLG_SCAN_RANK_FEATURE, "unknown scan kind" + in_q);
    PLAN_REQUIRE(spec->q_filter[q] >= -1, "negative filter id other than -1" + in_q);
    if (kind == SLG_SCAN_CONSTANT) PLAN_REQUIRE(std::isfinite(spec->q_score[q]), "non-finite score" + in_q);
    if (kind == SLG_SCAN_RANK_FEATURE) {
      const int32_t m = spec->q_modifier[q];
      PLAN_REQUIRE(m >= SLG_SCAN_MOD_NONE && m <= SLG_SCAN_MOD_RECIPROCAL, "unknown modifier" + in_q);
      PLAN_REQUIRE(std::isfinite(spec->q_missing[q]), "non-finite missing" + in_q);
      PLAN_REQUIRE(std::isfinite(spec->q_boost[q]), "non-finite boost" + in_q);
    }
  }
  if (k > SLG_MAX_K) throw SlgError(SLG_ERR_UNSUPPORTED, "k > SLG_MAX_K");
}

void plan_scan(const std::vector<uint32_t> &seg_docs, const std::vector<FscoreFieldView> &fields,
               const char *filter_live, size_t n_filters, uint32_t nq, const slg_scan_spec &spec,
               const int32_t *q_filter, bool full_regions, uint32_t k, ScanPlan &out) {
  out = ScanPlan{};
  const uint32_t n_segs = (uint32_t)seg_docs.size();
  out.queries.assign(nq, slg::ScanQuery{});
  out.qrefs.assign(nq, slg::QueryRef{0, 0});
  std::vector<int32_t> used_fields;  // the rows of the column table, in order of first use
  std::string unsupported;           // (reported behind every invalid argument)
  bool any_root = false;
  for (uint32_t q = 0; q < nq; q++) {
    const std::string in_q = " in scan query " + std::to_string(q);
    slg::ScanQuery &sq = out.queries[q];
    sq.kind = (uint32_t)spec.q_kind[q];
    sq.score = 1.0f;
    if (q_filter && q_filter[q] != -1) {
      PLAN_REQUIRE(q_filter[q] >= 0 && (size_t)q_filter[q] < n_filters && filter_live[q_filter[q]],
                   "unknown filter id " + std::to_string(q_filter[q]) + " in q_filter of query " + std::to_string(q));
      any_root = true;
    }
    if (spec.q_filter[q] >= 0) {
      PLAN_REQUIRE((size_t)spec.q_filter[q] < n_filters && filter_live[spec.q_filter[q]],
                   "unknown filter id " + std::to_string(spec.q_filter[q]) + in_q);
      sq.filter = (uint32_t)spec.q_filter[q] + 1u;
    }
    if (sq.kind == slg::kScanConstant) sq.score = spec.q_score[q];
    if (sq.kind == slg::kScanRankFeature) {
      const int32_t id = spec.q_field[q];
      const FscoreFieldView &fv = agg_field(fields, id, "", in_q);
      PLAN_REQUIRE(!fv.keyword, "agg field " + std::to_string(id) + " is a keyword field" + in_q);
      agg_field_rows(fv, n_segs, "", in_q);
      if (fv.non_finite && unsupported.empty())
        unsupported = "agg field " + std::to_string(id) + " holds a non-finite value (CPU path)" + in_q;
      sq.col = row_of(used_fields, id);
      sq.modifier = (uint32_t)spec.q_modifier[q];
      sq.missing = spec.q_missing[q];
      sq.boost = spec.q_boost[q];
      out.full = out.full || sq.modifier == slg::kScanModLog || sq.modifier == slg::kScanModLog1p;
    }
  }
  if (!unsupported.empty()) throw SlgError(SLG_ERR_UNSUPPORTED, unsupported);
  for (const int32_t id : used_fields) {
    const slg::ColumnDev *rows = agg_field_rows(agg_field(fields, id, "", ""), n_segs, "", "");
    out.cols.insert(out.cols.end(), rows, rows + n_segs);
  }
  if (any_root) {
    out.q_filter.assign(nq, 0u);
    for (uint32_t q = 0; q < nq; q++)
      if (q_filter[q] >= 0) out.q_filter[q] = (uint32_t)q_filter[q] + 1u;
  }
  // the slices: per query, per segment with docs, kScanSliceDocs docs each; the regions lie in slice order
  uint64_t per_query = 0;
  for (const uint32_t n : seg_docs) per_query += ((uint64_t)n + slg::kScanSliceDocs - 1) / slg::kScanSliceDocs;
  if (per_query * nq > 0xFFFFFFF0ull) throw SlgError(SLG_ERR_UNSUPPORTED, "a scan batch of more than 2^32 slices");
  out.slices.reserve((size_t)(per_query * nq));
  for (uint32_t q = 0; q < nq; q++) {
    const bool truncated = !full_regions && out.queries[q].kind != slg::kScanRankFeature;
    out.qrefs[q].slice_begin = (uint32_t)out.slices.size();
    for (uint32_t s = 0; s < n_segs; s++)
      for (uint64_t first = 0; first < seg_docs[s]; first += slg::kScanSliceDocs) {
        slg::ScanSlice sl{};
        sl.q = q;
        sl.seg = s;
        sl.first_doc = (uint32_t)first;
        sl.n_docs = (uint32_t)std::min<uint64_t>(slg::kScanSliceDocs, seg_docs[s] - first);
        sl.cap = truncated ? std::min(sl.n_docs, k) : sl.n_docs;
        out.slices.push_back(sl);
        out.slice_seg.push_back(s);
        out.slice_cbeg.push_back(out.cand_total);
        out.cand_total += sl.cap;
      }
    out.qrefs[q].slice_end = (uint32_t)out.slices.size();
  }
}

// ---- script_score ------------------------------------------------------------------------------------------
static_assert(slg::kScriptMaxInstrs == SLG_MAX_SCRIPT_INSTRS && slg::kScriptMaxDepth == SLG_MAX_SCRIPT_DEPTH &&
                  slg::kScriptMaxFields == SLG_MAX_SCRIPT_FIELDS, "the kernel's limits and the ABI's");
static_assert(sizeof(slg::ScriptQuery) == 64 && sizeof(slg::ScriptInstr) == 16, "records the kernel reads in whole words");

void check_script_order(int order) {
  PLAN_REQUIRE(order == SLG_SCRIPT_OUTER || order == SLG_SCRIPT_INNER, "unknown script order");
}

void check_script(const slg_script_spec *spec, uint32_t nq, ScriptShape &shape) {
  shape = ScriptShape{};
  PLAN_REQUIRE(spec != nullptr, "script spec is NULL");
  shape.max_depth.assign(nq, 0u);
  if (nq == 0) return;
  PLAN_REQUIRE(spec->p_offsets != nullptr, "script p_offsets is NULL");
  PLAN_REQUIRE(spec->q_boost != nullptr, "script q_boost is NULL");
  for (uint32_t q = 0; q < nq; q++)
    PLAN_REQUIRE(spec->p_offsets[q + 1] >= spec->p_offsets[q], "script p_offsets not monotone");
  const uint32_t i_lo = spec->p_offsets[0], i_hi = spec->p_offsets[nq];
  PLAN_REQUIRE(i_hi == i_lo || (spec->i_op && spec->i_arg), "script i_op/i_arg is NULL");
  shape.at.assign(i_hi - i_lo, 0u);
  std::string unsupported;  // (reported behind every invalid argument)
  const auto refuse = [&](const std::string &what) {
    if (unsupported.empty()) unsupported = what;
  };
  for (uint32_t q = 0; q < nq; q++) {
    const std::string in_q = " in script query " + std::to_string(q);
    PLAN_REQUIRE(std::isfinite(spec->q_boost[q]), "non-finite q_boost" + in_q);
    const uint32_t i0 = spec->p_offsets[q], n = spec->p_offsets[q + 1] - i0;
    if (n > SLG_MAX_SCRIPT_INSTRS) refuse("more than SLG_MAX_SCRIPT_INSTRS instructions" + in_q);
    uint32_t depth = 0, deepest = 0;
    bool underflow = false;
    std::vector<int32_t> seen;  // the distinct fields
    for (uint32_t i = i0; i < i0 + n; i++) {
      const int32_t op = spec->i_op[i];
      PLAN_REQUIRE(op >= SLG_SCRIPT_PUSH_CONST && op <= SLG_SCRIPT_NEG, "unknown script op" + in_q);
      const uint32_t pops = op <= SLG_SCRIPT_PUSH_SCORE ? 0u : (op == SLG_SCRIPT_NEG ? 1u : 2u);
      if (op == SLG_SCRIPT_PUSH_CONST) {
        PLAN_REQUIRE(spec->i_arg[i] >= 0 && (uint32_t)spec->i_arg[i] < spec->n_consts, "const index >= n_consts" + in_q);
        PLAN_REQUIRE(spec->consts != nullptr, "script consts is NULL");
        if (!std::isfinite(spec->consts[spec->i_arg[i]])) refuse("non-finite constant (CPU path)" + in_q);
      } else if (op == SLG_SCRIPT_PUSH_FIELD) {
        row_of(seen, spec->i_arg[i]);
      }
      if (depth < pops) {  // (the walk goes on for the invalid arguments behind it)
        underflow = true;
        depth = pops;
      }
      depth -= pops;
      shape.at[i - i_lo] = (uint8_t)std::min<uint32_t>(depth, 255u);
      depth++;
      deepest = std::max(deepest, depth);
    }
    if (n != 0 && (underflow || depth != 1)) refuse("ill-formed program: the reference returns no hit (CPU path)" + in_q);
    if (deepest > SLG_MAX_SCRIPT_DEPTH) refuse("stack deeper than SLG_MAX_SCRIPT_DEPTH" + in_q);
    if (seen.size() > SLG_MAX_SCRIPT_FIELDS) refuse("more than SLG_MAX_SCRIPT_FIELDS distinct fields" + in_q);
    shape.max_depth[q] = deepest;
    shape.batch_max_depth = std::max(shape.batch_max_depth, deepest);
  }
  if (!unsupported.empty()) throw SlgError(SLG_ERR_UNSUPPORTED, unsupported);
}

void plan_script(const std::vector<FscoreFieldView> &fields, uint32_t n_segs, uint32_t nq, const slg_script_spec &spec,
                 const ScriptShape &shape, ScriptPlan &out) {
  out = ScriptPlan{};
  out.queries.assign(nq, slg::ScriptQuery{});
  if (nq == 0) return;
  const uint32_t i_base = spec.p_offsets[0];
  std::vector<int32_t> used_fields;  // the rows of the column table, in order of first use
  std::string unsupported;           // (reported behind every invalid argument)
  for (uint32_t q = 0; q < nq; q++) {
    const std::string in_q = " in script query " + std::to_string(q);
    const uint32_t i0 = spec.p_offsets[q], n = spec.p_offsets[q + 1] - i0;
    slg::ScriptQuery &sq = out.queries[q];
    sq.instr_begin = i0 - i_base;
    sq.n_instrs = n;
    sq.boost = spec.q_boost[q];
    sq.max_depth = shape.max_depth[q];
    out.n_work += n != 0u ? 1u : 0u;
    std::vector<int32_t> mine;  // the query's distinct fields, in order of first use
    for (uint32_t i = i0; i < i0 + n; i++) {
      slg::ScriptInstr in{};
      const int32_t op = spec.i_op[i];
      in.code = (uint32_t)op | ((uint32_t)shape.at[i - i_base] << 8);
      if (op == SLG_SCRIPT_PUSH_CONST) {
        in.value = spec.consts[spec.i_arg[i]];
      } else if (op == SLG_SCRIPT_PUSH_FIELD) {
        const int32_t id = spec.i_arg[i];
        const FscoreFieldView &fv = agg_field(fields, id, "", in_q);
        PLAN_REQUIRE(!fv.keyword, "agg field " + std::to_string(id) + " is a keyword field" + in_q);
        agg_field_rows(fv, n_segs, "", "");
        if (fv.non_finite && unsupported.empty())
          unsupported = "agg field " + std::to_string(id) + " holds a non-finite value (CPU path)" + in_q;
        const uint32_t f = row_of(mine, id);
        sq.col[f] = row_of(used_fields, id);  // (f < SLG_MAX_SCRIPT_FIELDS: check_script)
        in.code |= f << 16;
      }
      out.instrs.push_back(in);
    }
    sq.n_fields = (uint32_t)mine.size();
  }
  if (!unsupported.empty()) throw SlgError(SLG_ERR_UNSUPPORTED, unsupported);
  out.max_depth = shape.batch_max_depth;
  std::vector<const uint32_t *> no_filters;
  fill_tables(fields, used_fields, nullptr, {}, n_segs, out.cols, no_filters);
}

// ---- nested boolean matchers ------------------------------------------------------------------------------
static_assert(slg::kBoolTreeMaxLeaves == SLG_MAX_BOOL_TREE_LEAVES && slg::kBoolTreeMaxNodes == SLG_MAX_BOOL_TREE_NODES &&
                  slg::kBoolTreeMaxLeaves == 32 && slg::kBoolTreeMaxNodes == 32,
              "the kernel's value masks (bits 0-31 leaves, 32-63 nodes) and the ABI's limits");
static_assert(sizeof(slg::BoolTreeQuery) == 32 && sizeof(slg::BoolTreeNode) == 32, "records the kernel reads in whole words");

void check_bool_tree(const slg_bool_tree_spec *spec, uint32_t nq, const slg_score_plans *plans) {
  PLAN_REQUIRE(spec != nullptr, "bool tree spec is NULL");
  if (nq == 0) return;
  PLAN_REQUIRE(spec->c_offsets != nullptr, "bool tree c_offsets is NULL");
  PLAN_REQUIRE(spec->g_offsets != nullptr, "bool tree g_offsets is NULL");
  PLAN_REQUIRE(spec->f_offsets != nullptr, "bool tree f_offsets is NULL");
  PLAN_REQUIRE(spec->n_offsets != nullptr, "bool tree n_offsets is NULL");
  for (uint32_t q = 0; q < nq; q++) {
    PLAN_REQUIRE(spec->c_offsets[q + 1] >= spec->c_offsets[q], "bool tree c_offsets not monotone");
    PLAN_REQUIRE(spec->g_offsets[q + 1] >= spec->g_offsets[q], "bool tree g_offsets not monotone");
    PLAN_REQUIRE(spec->f_offsets[q + 1] >= spec->f_offsets[q], "bool tree f_offsets not monotone");
    PLAN_REQUIRE(spec->n_offsets[q + 1] >= spec->n_offsets[q], "bool tree n_offsets not monotone");
  }
  PLAN_REQUIRE(spec->c_offsets[nq] == spec->c_offsets[0] || (spec->c_term_ids && spec->c_group),
               "bool tree c_term_ids/c_group is NULL");
  PLAN_REQUIRE(spec->f_offsets[nq] == spec->f_offsets[0] || spec->f_filter, "bool tree f_filter is NULL");
  const uint32_t n0 = spec->n_offsets[0], n1 = spec->n_offsets[nq];
  if (n1 != n0) {
    PLAN_REQUIRE(spec->n_min_should && spec->e_offsets, "bool tree n_min_should/e_offsets is NULL");
    for (uint32_t n = n0; n < n1; n++)
      PLAN_REQUIRE(spec->e_offsets[n + 1] >= spec->e_offsets[n], "bool tree e_offsets not monotone");
    PLAN_REQUIRE(spec->e_offsets[n1] == spec->e_offsets[n0] || (spec->e_child && spec->e_kind),
                 "bool tree e_child/e_kind is NULL");
  }
  std::string unsupported;  // (reported behind every invalid argument)
  for (uint32_t q = 0; q < nq; q++) {
    const std::string in_q = " in bool tree query " + std::to_string(q);
    const uint32_t t0 = spec->c_offsets[q], nt = spec->c_offsets[q + 1] - t0;
    const uint32_t ng = spec->g_offsets[q + 1] - spec->g_offsets[q];
    const uint32_t f0 = spec->f_offsets[q], nf = spec->f_offsets[q + 1] - f0;
    const uint32_t nb = spec->n_offsets[q], nn = spec->n_offsets[q + 1] - nb;
    uint32_t next = 0;  // the group a new group's first term must name
    for (uint32_t i = 0; i < nt; i++) {
      const uint32_t g = spec->c_group[t0 + i];
      PLAN_REQUIRE(g < ng, "c_group names a group the query does not have" + in_q);
      PLAN_REQUIRE(g == next || (next > 0 && g == next - 1), "c_group decreases or skips a group" + in_q);
      if (g == next) next++;
    }
    PLAN_REQUIRE(next == ng, "a group without a term" + in_q);
    for (uint32_t f = f0; f < f0 + nf; f++)
      PLAN_REQUIRE(spec->f_filter[f] >= 0, "unknown filter id " + std::to_string(spec->f_filter[f]) + in_q);
    const uint64_t nl = (uint64_t)ng + nf;  // leaves
    PLAN_REQUIRE(nl == 0 || nn != 0, "leaves but no node" + in_q);
    std::vector<uint32_t> refs((size_t)(nl + nn), 0u);  // how often each value is some node's child
    bool twice = false;
    for (uint32_t j = 0; j < nn; j++) {
      std::vector<uint32_t> mine;
      for (uint32_t e = spec->e_offsets[nb + j]; e < spec->e_offsets[nb + j + 1]; e++) {
        PLAN_REQUIRE(clause_kind_known(spec->e_kind[e]), "unknown child kind" + in_q);
        const uint32_t c = spec->e_child[e];
        PLAN_REQUIRE((uint64_t)c < nl + j, "a child index that is not below its node" + in_q);
        twice = twice || std::find(mine.begin(), mine.end(), c) != mine.end();
        mine.push_back(c);
        refs[c]++;
      }
    }
    for (uint64_t v = 0; v + 1 < nl + nn; v++)  // (every value but the root)
      PLAN_REQUIRE(refs[v] != 0u, std::string(v < nl ? "a leaf" : "a node other than the root") + " that no node references" + in_q);
    require_no_min_match(plans, q, "bool tree", in_q);
    if (!unsupported.empty()) continue;
    if (nl > SLG_MAX_BOOL_TREE_LEAVES) unsupported = "more than SLG_MAX_BOOL_TREE_LEAVES leaves" + in_q;
    else if (nn > SLG_MAX_BOOL_TREE_NODES) unsupported = "more than SLG_MAX_BOOL_TREE_NODES nodes" + in_q;
    else if (nt > SLG_MAX_BOOL_TERMS) unsupported = "more than SLG_MAX_BOOL_TERMS clause terms" + in_q;
    else if (twice) unsupported = "the same child twice in one node" + in_q;
  }
  if (!unsupported.empty()) throw SlgError(SLG_ERR_UNSUPPORTED, unsupported);
}

void plan_bool_tree(const std::vector<SegView> &segs, const uint32_t *const *reject, const char *filter_live,
                    size_t n_filters, uint32_t nq, const slg_bool_tree_spec &spec, BoolTreePlan &out) {
  const uint32_t n_segs = (uint32_t)segs.size();
  out = BoolTreePlan{};
  out.queries.assign(nq, slg::BoolTreeQuery{});
  if (nq == 0) return;
  const uint32_t c_base = spec.c_offsets[0];
  out.terms.reserve((size_t)(spec.c_offsets[nq] - c_base) * n_segs);
  std::vector<int32_t> used_filters;  // the rows of the filter table, in order of first use
  for (uint32_t q = 0; q < nq; q++) {
    const std::string in_q = " in bool tree query " + std::to_string(q);
    const uint32_t t0 = spec.c_offsets[q], nt = spec.c_offsets[q + 1] - t0;
    const uint32_t ng = spec.g_offsets[q + 1] - spec.g_offsets[q];
    const uint32_t f0 = spec.f_offsets[q], nf = spec.f_offsets[q + 1] - f0;
    const uint32_t nb = spec.n_offsets[q], nn = spec.n_offsets[q + 1] - nb;
    const uint32_t nl = ng + nf;
    slg::BoolTreeQuery &tq = out.queries[q];
    tq.term_begin = t0 - c_base;
    tq.n_terms = nt;
    tq.node_begin = (uint32_t)out.nodes.size();
    tq.n_nodes = nn;
    tq.n_leaves = nl;
    tq.filt_begin = (uint32_t)out.filt_rows.size();
    tq.n_filters = nf;
    for (uint32_t f = f0; f < f0 + nf; f++) {
      PLAN_REQUIRE((size_t)spec.f_filter[f] < n_filters && filter_live[spec.f_filter[f]],
                   "unknown filter id " + std::to_string(spec.f_filter[f]) + in_q);
      out.filt_rows.push_back(row_of(used_filters, spec.f_filter[f]));
    }
    // a child as a value bit: a leaf its own number, node j bit 32 + j
    const auto value_bit = [nl](uint32_t c) { return 1ull << (c < nl ? c : 32u + (c - nl)); };
    for (uint32_t j = 0; j < nn; j++) {
      slg::BoolTreeNode nd{};
      nd.min_should = spec.n_min_should[nb + j];
      for (uint32_t e = spec.e_offsets[nb + j]; e < spec.e_offsets[nb + j + 1]; e++) {
        const int32_t kind = spec.e_kind[e];
        (kind == SLG_BOOL_MUST ? nd.must : kind == SLG_BOOL_MUST_NOT ? nd.must_not : nd.should) |= value_bit(spec.e_child[e]);
      }
      out.nodes.push_back(nd);
    }
    // the values that reach the root over MUST / MUST_NOT edges only, from the root down (a parent lies above
    // its children): the leaves among them can reject on their own and go first in the row
    uint64_t direct = nn ? 1ull << (31u + nn) : 0ull;
    for (uint32_t j = nn; j-- > 0;) {
      const slg::BoolTreeNode &nd = out.nodes[tq.node_begin + j];
      if (direct & (1ull << (32u + j))) direct |= nd.must | nd.must_not;
    }
    uint32_t order[SLG_MAX_BOOL_TERMS], n = 0;
    for (const bool first : {true, false})
      for (uint32_t i = 0; i < nt; i++)
        if ((((direct >> spec.c_group[t0 + i]) & 1ull) != 0ull) == first) order[n++] = i;
    for (uint32_t s = 0; s < n_segs; s++) {
      for (uint32_t j = 0; j < nt; j++) {
        const uint32_t i = order[j];
        slg::BoolTerm bt{};
        bt.group = spec.c_group[t0 + i];
        if (i + 1 == nt || spec.c_group[t0 + i + 1] != bt.group) bt.group |= slg::kBoolTreeLeafEnd;
        uint64_t ubase;
        resolve_term(segs[s], spec.c_term_ids[(size_t)(t0 + i) * n_segs + s], "bool tree", q, bt.off, ubase, bt.df);
        out.terms.push_back(bt);
      }
    }
  }
  for (const int32_t f : used_filters)
    out.filters.insert(out.filters.end(), reject + (size_t)f * n_segs, reject + ((size_t)f + 1) * n_segs);
}

// ---- filter trees --------------------------------------------------------------------------------------
static_assert(slg::kFilterMaxNodes == SLG_MAX_FILTER_NODES && slg::kFilterMaxDepth == SLG_MAX_FILTER_DEPTH &&
                  slg::kFilterMaxTrees == SLG_MAX_FILTER_TREES, "the kernel's limits and the ABI's");
static_assert(slg::kFilterKeywordIn == SLG_FILTER_KEYWORD_IN && slg::kFilterRangeF64 == SLG_FILTER_RANGE_F64 &&
                  slg::kFilterRangeI64 == SLG_FILTER_RANGE_I64 && slg::kFilterId == SLG_FILTER_ID &&
                  slg::kFilterAnd == SLG_FILTER_AND && slg::kFilterOr == SLG_FILTER_OR &&
                  slg::kFilterNot == SLG_FILTER_NOT, "header kinds");
static_assert(sizeof(slg::FilterTreeDev) == 8 && sizeof(slg::FilterNodeDev) == 32, "records the kernel reads in whole words");

static_assert(slg::kFilterNested == SLG_FILTER_NESTED && slg::kNestedMaxScopes == SLG_MAX_NESTED_SCOPES &&
                  slg::kNestedMaxDepth == SLG_MAX_NESTED_DEPTH, "the nested kind and limits");
static_assert(sizeof(slg::NestedScopeDev) == 16 && sizeof(slg::NestedPathDev) == 40 && sizeof(slg::NestedColDev) == 24,
              "records the kernel reads in whole words");

namespace {
// The checks of one postfix program that need no index, shared by the flat trees and every scope of a nested tree
// -> the deepest evaluation stack.  nested(n, at): what a NESTED node has to satisfy; without it the kind is unknown
// here.  object_scope: FILTER_ID is refused.  node 0 of the program is node `first` of its tree
template <typename Nested>
uint64_t check_program(const slg_filter_node *nodes, uint32_t first, uint32_t n_nodes, uint32_t n_ords, bool object_scope,
                       const std::string &in_t, const Nested *nested) {
  uint64_t depth = 0, deepest = 0;  // the evaluation stack of the postfix program
  for (uint32_t i = 0; i < n_nodes; i++) {
    const slg_filter_node &n = nodes[i];
    const std::string at = " (node " + std::to_string(first + i) + ")" + in_t;
    PLAN_REQUIRE(n.kind >= SLG_FILTER_KEYWORD_IN && n.kind <= (nested ? SLG_FILTER_NESTED : SLG_FILTER_NOT),
                 "unknown filter node kind" + at);
    if (n.kind == SLG_FILTER_NOT) {
      PLAN_REQUIRE(depth >= 1u, "NOT underflows the stack" + at);
    } else if (n.kind == SLG_FILTER_AND || n.kind == SLG_FILTER_OR) {
      PLAN_REQUIRE((uint64_t)n.arity <= depth, "arity larger than the stack" + at);
      depth = depth - n.arity + 1u;
    } else {
      if (n.kind == SLG_FILTER_RANGE_F64)
        PLAN_REQUIRE(!std::isnan(n.lo_f) && !std::isnan(n.hi_f), "NaN bound" + at);
      if (n.kind == SLG_FILTER_KEYWORD_IN)
        PLAN_REQUIRE((uint64_t)n.ord_begin + n.n_ords_in <= n_ords, "ord_begin + n_ords_in > n_ords" + at);
      if (n.kind == SLG_FILTER_ID) PLAN_REQUIRE(!object_scope, "FILTER_ID in an object scope" + at);
      if (n.kind == SLG_FILTER_NESTED) (*nested)(n, at);
      depth++;
    }
    deepest = std::max(deepest, depth);
  }
  PLAN_REQUIRE(depth == 1u, "the program does not end with exactly one value" + in_t);
  return deepest;
}
using NoNested = void (*)(const slg_filter_node &, const std::string &);

// the ordinal bit set of a KEYWORD_IN node over a dictionary of n_ords keys, appended to words -> its first word
uint32_t ord_bit_set(std::vector<uint32_t> &words, const slg_filter_node &n, const uint32_t *ords, uint32_t n_ords,
                     const std::string &what, const std::string &in_t) {
  const uint32_t bits = (uint32_t)words.size();
  words.resize(words.size() + ((size_t)n_ords + 31u) / 32u, 0u);
  for (uint32_t j = 0; j < n.n_ords_in; j++) {
    const uint32_t o = ords[n.ord_begin + j];
    PLAN_REQUIRE(o < n_ords, "ordinal " + std::to_string(o) + " >= n_ords of " + what + in_t);
    words[bits + (o >> 5)] |= 1u << (o & 31u);
  }
  return bits;
}

// The doc-level nodes of filter trees against an index state's agg fields and filters: the leaf validation, the
// i64 clamping and the two row tables that the flat trees and the doc level of nested trees share
struct DocLevelNodes {
  const std::vector<FscoreFieldView> &fields;
  const char *filter_live;
  size_t n_filters;
  uint32_t n_segs;
  std::vector<uint32_t> &words;
  std::vector<int32_t> used_fields, used_filters;  // the rows of the two tables, in order of first use
  std::string unsupported;                         // (reported behind every invalid argument)

  slg::FilterNodeDev node(const slg_filter_node &n, const uint32_t *ords, const std::string &in_t) {
    constexpr double k2p53 = 9007199254740992.0;
    constexpr int64_t i2p53 = (int64_t)1 << 53;
    slg::FilterNodeDev nd{};
    nd.kind = (uint32_t)n.kind;
    if (n.kind == SLG_FILTER_AND || n.kind == SLG_FILTER_OR) {
      nd.arity = n.arity;
    } else if (n.kind == SLG_FILTER_ID) {
      const int32_t f = n.filter_id;
      PLAN_REQUIRE(f >= 0 && (size_t)f < n_filters && filter_live[f],
                   "unknown filter id " + std::to_string(f) + " (or one without a bitmap for every segment)" + in_t);
      nd.row = row_of(used_filters, f);
    } else if (n.kind != SLG_FILTER_NOT) {
      const int32_t id = n.field;
      const FscoreFieldView &fv = agg_field(fields, id, "", in_t);
      agg_field_rows(fv, n_segs, "", in_t);
      nd.row = row_of(used_fields, id);
      if (n.kind == SLG_FILTER_KEYWORD_IN) {
        PLAN_REQUIRE(fv.keyword, "agg field " + std::to_string(id) + " is not a keyword field" + in_t);
        nd.bits = ord_bit_set(words, n, ords, fv.n_ords, "agg field " + std::to_string(id), in_t);
      } else {
        PLAN_REQUIRE(!fv.keyword, "agg field " + std::to_string(id) + " is a keyword field" + in_t);
        if (n.kind == SLG_FILTER_RANGE_F64) {
          nd.lo = n.lo_f;
          nd.hi = n.hi_f;
        } else {
          PLAN_REQUIRE(fv.from_i64, "agg field " + std::to_string(id) + " was not registered from i64 values" + in_t);
          if (unsupported.empty() && (fv.i64_rounded || (fv.any_value && (fv.vmin < -k2p53 || fv.vmax > k2p53))))
            unsupported = "agg field " + std::to_string(id) + " holds an i64 value beyond +-2^53 (CPU path)" + in_t;
          // every stored value is an integer within +-2^53: a bound on the far side of it selects what the
          // clamped one does; a lower bound above 2^53 (an upper one below -2^53) selects nothing, which the
          // clamped bound would not say of a value of exactly +-2^53, so it becomes the infinity
          nd.lo = n.lo_i > i2p53 ? HUGE_VAL : (double)std::max<int64_t>(n.lo_i, -i2p53);
          nd.hi = n.hi_i < -i2p53 ? -HUGE_VAL : (double)std::min<int64_t>(n.hi_i, i2p53);
        }
      }
    }
    return nd;
  }
  // behind every node: the pending SLG_ERR_UNSUPPORTED, else the two tables
  void finish(const uint32_t *const *reject, std::vector<slg::ColumnDev> &cols, std::vector<const uint32_t *> &filters) {
    if (!unsupported.empty()) throw SlgError(SLG_ERR_UNSUPPORTED, unsupported);
    fill_tables(fields, used_fields, reject, used_filters, n_segs, cols, filters);
  }
};
}  // namespace

void check_filter_trees(const slg_filter_tree *trees, uint32_t n_trees) {
  PLAN_REQUIRE(trees != nullptr, "filter trees is NULL");
  PLAN_REQUIRE(n_trees != 0u, "n_trees is 0");
  std::string unsupported;  // (reported behind every invalid argument)
  for (uint32_t t = 0; t < n_trees; t++) {
    const slg_filter_tree &tr = trees[t];
    const std::string in_t = " in filter tree " + std::to_string(t);
    PLAN_REQUIRE(tr.n_nodes != 0u, "n_nodes is 0" + in_t);
    PLAN_REQUIRE(tr.nodes != nullptr, "nodes is NULL" + in_t);
    PLAN_REQUIRE(tr.n_ords == 0u || tr.ords != nullptr, "ords is NULL" + in_t);
    const uint64_t deepest = check_program<NoNested>(tr.nodes, 0u, tr.n_nodes, tr.n_ords, false, in_t, nullptr);
    if (unsupported.empty() && tr.n_nodes > SLG_MAX_FILTER_NODES)
      unsupported = "more than SLG_MAX_FILTER_NODES nodes" + in_t;
    if (unsupported.empty() && deepest > SLG_MAX_FILTER_DEPTH)
      unsupported = "evaluation stack deeper than SLG_MAX_FILTER_DEPTH" + in_t;
  }
  if (unsupported.empty() && n_trees > SLG_MAX_FILTER_TREES) unsupported = "more than SLG_MAX_FILTER_TREES trees in one call";
  if (!unsupported.empty()) throw SlgError(SLG_ERR_UNSUPPORTED, unsupported);
}

void plan_filter_trees(const std::vector<FscoreFieldView> &fields, const uint32_t *const *reject,
                       const char *filter_live, size_t n_filters, uint32_t n_segs, const slg_filter_tree *trees,
                       uint32_t n_trees, FilterTreePlan &out) {
  out = FilterTreePlan{};
  out.trees.reserve(n_trees);
  DocLevelNodes doc{fields, filter_live, n_filters, n_segs, out.words, {}, {}, {}};
  for (uint32_t t = 0; t < n_trees; t++) {
    const slg_filter_tree &tr = trees[t];
    const std::string in_t = " in filter tree " + std::to_string(t);
    out.trees.push_back(slg::FilterTreeDev{(uint32_t)out.nodes.size(), tr.n_nodes});
    for (uint32_t i = 0; i < tr.n_nodes; i++) out.nodes.push_back(doc.node(tr.nodes[i], tr.ords, in_t));
  }
  doc.finish(reject, out.cols, out.filters);
}

// ---- nested filter trees -------------------------------------------------------------------------------
namespace {
// the level of every scope of a checked tree: an object scope without a NESTED leaf is level 1, one with such
// leaves lies one above its highest child; the doc-level scope's entry is the tree's nesting depth
std::vector<uint32_t> scope_levels(const slg_nested_filter_tree &tr) {
  std::vector<uint32_t> level(tr.n_scopes, 0u);
  for (uint32_t s = 0; s < tr.n_scopes; s++) {
    const slg_nested_scope &sc = tr.scopes[s];
    uint32_t below = 0;
    for (uint32_t i = 0; i < sc.n_nodes; i++) {
      const slg_filter_node &n = tr.nodes[sc.node_begin + i];
      if (n.kind == SLG_FILTER_NESTED) below = std::max(below, level[n.field]);
    }
    level[s] = s + 1u == tr.n_scopes ? below : below + 1u;
  }
  return level;
}
}  // namespace

void check_nested_filter_trees(const slg_nested_filter_tree *trees, uint32_t n_trees) {
  PLAN_REQUIRE(trees != nullptr, "nested filter trees is NULL");
  PLAN_REQUIRE(n_trees != 0u, "n_trees is 0");
  std::string unsupported;  // (reported behind every invalid argument)
  for (uint32_t t = 0; t < n_trees; t++) {
    const slg_nested_filter_tree &tr = trees[t];
    const std::string in_t = " in nested filter tree " + std::to_string(t);
    PLAN_REQUIRE(tr.n_scopes != 0u, "n_scopes is 0" + in_t);
    PLAN_REQUIRE(tr.scopes != nullptr, "scopes is NULL" + in_t);
    PLAN_REQUIRE(tr.n_nodes != 0u, "n_nodes is 0" + in_t);
    PLAN_REQUIRE(tr.nodes != nullptr, "nodes is NULL" + in_t);
    PLAN_REQUIRE(tr.n_ords == 0u || tr.ords != nullptr, "ords is NULL" + in_t);
    std::vector<uint32_t> named(tr.n_scopes, 0u);  // how many NESTED nodes name each scope
    uint64_t deepest = 0, total = 0;
    for (uint32_t s = 0; s < tr.n_scopes; s++) {
      const slg_nested_scope &sc = tr.scopes[s];
      const std::string in_s = " (scope " + std::to_string(s) + ")" + in_t;
      const bool doc_level = s + 1u == tr.n_scopes;
      PLAN_REQUIRE(sc.path >= -1, "path below -1" + in_s);
      PLAN_REQUIRE(doc_level == (sc.path == -1),
                   (doc_level ? "the last scope is not the doc level" : "a scope before the last one is the doc level") + in_s);
      PLAN_REQUIRE(sc.n_nodes != 0u, "the scope's n_nodes is 0" + in_s);
      PLAN_REQUIRE((uint64_t)sc.node_begin + sc.n_nodes <= tr.n_nodes, "node_begin + n_nodes > the tree's n_nodes" + in_s);
      const auto nested = [&](const slg_filter_node &n, const std::string &at) {
        PLAN_REQUIRE(n.field >= 0 && (uint32_t)n.field < s, "a NESTED node names no earlier scope" + at);
        named[n.field]++;
      };
      deepest = std::max(deepest, check_program(tr.nodes + sc.node_begin, sc.node_begin, sc.n_nodes, tr.n_ords,
                                                !doc_level, in_s, &nested));
      total += sc.n_nodes;
    }
    for (uint32_t s = 0; s + 1u < tr.n_scopes; s++)
      PLAN_REQUIRE(named[s] == 1u, std::string(named[s] ? "a scope is named by more than one NESTED node" :
                                                          "a scope is named by no NESTED node") +
                                       " (scope " + std::to_string(s) + ")" + in_t);
    if (unsupported.empty() && total > SLG_MAX_FILTER_NODES)
      unsupported = "more than SLG_MAX_FILTER_NODES nodes over all scopes" + in_t;
    if (unsupported.empty() && deepest > SLG_MAX_FILTER_DEPTH)
      unsupported = "evaluation stack deeper than SLG_MAX_FILTER_DEPTH" + in_t;
    if (unsupported.empty() && tr.n_scopes > SLG_MAX_NESTED_SCOPES)
      unsupported = "more than SLG_MAX_NESTED_SCOPES scopes" + in_t;
    if (unsupported.empty() && scope_levels(tr).back() > SLG_MAX_NESTED_DEPTH)
      unsupported = "object scopes nested deeper than SLG_MAX_NESTED_DEPTH" + in_t;
  }
  if (unsupported.empty() && n_trees > SLG_MAX_FILTER_TREES) unsupported = "more than SLG_MAX_FILTER_TREES trees in one call";
  if (!unsupported.empty()) throw SlgError(SLG_ERR_UNSUPPORTED, unsupported);
}

void plan_nested_filter_trees(const std::vector<FscoreFieldView> &fields, const uint32_t *const *reject,
                              const char *filter_live, size_t n_filters, const std::vector<NestedPathView> &paths,
                              const std::vector<NestedFieldView> &nested_fields, uint32_t n_segs,
                              const slg_nested_filter_tree *trees, uint32_t n_trees, NestedFilterPlan &out) {
  out = NestedFilterPlan{};
  DocLevelNodes doc{fields, filter_live, n_filters, n_segs, out.words, {}, {}, {}};
  std::vector<int32_t> used_paths, used_ncols;  // the rows of the two nested tables, in order of first use
  const auto path_of = [&](int32_t id, const std::string &in_s) -> const NestedPathView & {
    const auto it = std::find_if(paths.begin(), paths.end(), [id](const NestedPathView &v) { return v.id == id; });
    PLAN_REQUIRE(it != paths.end(), "unknown nested path id " + std::to_string(id) + in_s);
    for (uint32_t s = 0; s < n_segs; s++)
      PLAN_REQUIRE(s < it->per_seg.size() && it->per_seg[s].base != nullptr,
                   "nested path " + std::to_string(id) + " has no tables for segment " + std::to_string(s) +
                       " (added after the path was registered)" + in_s);
    return *it;
  };
  // pass 1, in the caller's order (so that the first error is the first in the trees): every scope's nodes, a
  // NESTED node's row still the child's index in its own tree
  struct Scope {
    uint32_t tree, index, level, path_row;
    std::vector<slg::FilterNodeDev> nodes;
  };
  std::vector<Scope> all;
  std::vector<uint32_t> tree_first(n_trees);
  uint32_t levels = 0;
  for (uint32_t t = 0; t < n_trees; t++) {
    const slg_nested_filter_tree &tr = trees[t];
    const std::string in_t = " in nested filter tree " + std::to_string(t);
    const std::vector<uint32_t> level = scope_levels(tr);
    levels = std::max(levels, level.back());
    tree_first[t] = (uint32_t)all.size();
    for (uint32_t s = 0; s < tr.n_scopes; s++) {
      const slg_nested_scope &sc = tr.scopes[s];
      const std::string in_s = " (scope " + std::to_string(s) + ")" + in_t;
      Scope scope{t, s, level[s], 0u, {}};
      const bool doc_level = sc.path < 0;
      const NestedPathView *own = doc_level ? nullptr : &path_of(sc.path, in_s);
      if (own) scope.path_row = row_of(used_paths, sc.path);
      for (uint32_t i = 0; i < sc.n_nodes; i++) {
        const slg_filter_node &n = tr.nodes[sc.node_begin + i];
        if (n.kind == SLG_FILTER_NESTED) {
          const int32_t child = tr.scopes[n.field].path;
          const NestedPathView &cp = path_of(child, in_s);
          PLAN_REQUIRE(doc_level || cp.parent == sc.path,
                       "nested path " + std::to_string(child) + " is not registered under path " +
                           std::to_string(sc.path) + in_s);
          slg::FilterNodeDev nd{};
          nd.kind = slg::kFilterNested;
          nd.row = (uint32_t)n.field;
          scope.nodes.push_back(nd);
        } else if (doc_level || n.kind >= SLG_FILTER_AND) {
          scope.nodes.push_back(doc.node(n, tr.ords, in_s));
        } else {
          // a leaf over a nested column of this scope's path.  The column's kind must be the leaf's; a column of
          // another path is not what the reference looks up (`path.field`): nothing passes
          const int32_t id = n.field;
          const auto it = std::find_if(nested_fields.begin(), nested_fields.end(),
                                       [id](const NestedFieldView &v) { return v.id == id; });
          PLAN_REQUIRE(it != nested_fields.end(), "unknown nested field id " + std::to_string(id) + in_s);
          for (uint32_t g = 0; g < n_segs; g++)
            PLAN_REQUIRE(g < it->has.size() && it->has[g],
                         "nested field " + std::to_string(id) + " has no column for segment " + std::to_string(g) +
                             " (added after the field was registered)" + in_s);
          static const char *const kind_name[] = {"", "an f64", "an i64", "a keyword"};
          const int want = n.kind == SLG_FILTER_KEYWORD_IN ? 3 : n.kind == SLG_FILTER_RANGE_F64 ? 1 : 2;
          PLAN_REQUIRE(it->kind == want, "nested field " + std::to_string(id) + " is not " + kind_name[want] + " field" + in_s);
          slg::FilterNodeDev nd{};
          nd.kind = (uint32_t)n.kind;
          if (n.kind == SLG_FILTER_KEYWORD_IN) {
            nd.bits = ord_bit_set(out.words, n, tr.ords, it->n_ords, "nested field " + std::to_string(id), in_s);
          } else if (n.kind == SLG_FILTER_RANGE_F64) {
            nd.lo = n.lo_f;
            nd.hi = n.hi_f;
          } else {  // int64 against int64: the bounds travel in the bits of lo / hi
            std::memcpy(&nd.lo, &n.lo_i, 8);
            std::memcpy(&nd.hi, &n.hi_i, 8);
          }
          if (it->path == sc.path) {
            nd.row = row_of(used_ncols, id);
          } else {
            nd = slg::FilterNodeDev{};
            nd.kind = slg::kFilterOr;
          }
          scope.nodes.push_back(nd);
        }
      }
      all.push_back(std::move(scope));
    }
  }
  doc.finish(reject, out.cols, out.filters);
  // pass 2: the rows by level, the doc-level scopes last in tree order
  std::vector<uint32_t> row(all.size(), 0u), order;
  out.level_begin.push_back(0u);
  for (uint32_t l = 1; l <= levels + 1u; l++) {
    for (uint32_t i = 0; i < all.size(); i++) {
      const bool doc_level = all[i].index + 1u == trees[all[i].tree].n_scopes;
      if (l <= levels ? (!doc_level && all[i].level == l) : doc_level) {
        row[i] = (uint32_t)order.size();
        order.push_back(i);
      }
    }
    if (l <= levels) out.level_begin.push_back((uint32_t)order.size());
  }
  for (const uint32_t i : order) {
    const Scope &scope = all[i];
    out.scopes.push_back(slg::NestedScopeDev{(uint32_t)out.nodes.size(), (uint32_t)scope.nodes.size(), scope.path_row, 0u});
    for (slg::FilterNodeDev nd : scope.nodes) {
      if (nd.kind == slg::kFilterNested) nd.row = row[tree_first[scope.tree] + nd.row];
      out.nodes.push_back(nd);
    }
  }
  for (const int32_t id : used_paths) {
    const auto it = std::find_if(paths.begin(), paths.end(), [id](const NestedPathView &v) { return v.id == id; });
    out.paths.insert(out.paths.end(), it->per_seg.begin(), it->per_seg.begin() + n_segs);
  }
  for (const int32_t id : used_ncols) {
    const auto it = std::find_if(nested_fields.begin(), nested_fields.end(),
                                 [id](const NestedFieldView &v) { return v.id == id; });
    out.ncols.insert(out.ncols.end(), it->per_seg.begin(), it->per_seg.begin() + n_segs);
  }
}

// ---- sort keys of numeric fast fields ----------------------------------------------------------
namespace {
inline uint64_t i64_key(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }
inline uint64_t f64_key(double v) {  // f64::total_cmp order: negative values flipped whole, positive ones above them
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// Some(Greater) of a.partial_cmp(b) (None: a NaN, = Equal for min_by / max_by)
template <typename T>
inline bool greater(T a, T b) { return a > b; }

template <typename T>
void field_keys(uint32_t n_docs, const uint32_t *offsets, const T *values, uint64_t (*enc)(T), uint64_t *asc,
                uint64_t *desc, uint32_t *present) {
  for (uint32_t w = 0; w < (n_docs + 31) / 32; w++) present[w] = 0u;
  for (uint32_t d = 0; d < n_docs; d++) {
    const uint32_t a = offsets ? offsets[d] : 0u, e = offsets ? offsets[d + 1] : 0u;
    if (e <= a) {
      asc[d] = desc[d] = 0ull;
      continue;
    }
    // Iterator::min_by: cmp::min_by(acc, y) = acc unless acc > y; max_by: cmp::max_by(acc, y) = y unless acc > y
    T mn = values[a], mx = values[a];
    for (uint32_t i = a + 1; i < e; i++) {
      if (greater(mn, values[i])) mn = values[i];
      if (!greater(mx, values[i])) mx = values[i];
    }
    asc[d] = enc(mn);
    desc[d] = ~enc(mx);
    present[d >> 5] |= 1u << (d & 31u);
  }
}
}  // namespace

void sort_field_keys(int kind, uint32_t n_docs, const uint32_t *offsets, const void *values, uint64_t *asc,
                     uint64_t *desc, uint32_t *present_words) {
  if (kind == 1)
    field_keys<int64_t>(n_docs, offsets, static_cast<const int64_t *>(values), i64_key, asc, desc, present_words);
  else if (kind == 2)
    field_keys<double>(n_docs, offsets, static_cast<const double *>(values), f64_key, asc, desc, present_words);
  else
    throw SlgError(SLG_ERR_INVALID, "unknown sort field kind");
}

namespace {
uint32_t ordered_score_bits(uint32_t b) { return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u); }
}  // namespace

void cursor_key(uint32_t n_parts, const int *kind, const int32_t *order, const slg_sort_cursor &c, uint32_t *out) {
  const uint32_t parts = n_parts ? n_parts : 1u;  // (score order: part 0 is the score)
  PLAN_REQUIRE(parts <= SLG_MAX_SORT_PARTS, "more than SLG_MAX_SORT_PARTS sort parts");
  PLAN_REQUIRE((c.missing_mask >> parts) == 0u, "cursor: Missing bit beyond the sort spec");
  for (uint32_t i = parts; i < SLG_MAX_SORT_PARTS; i++)
    PLAN_REQUIRE(c.value_bits[i] == 0u, "cursor: value beyond the sort spec is not zero");
  auto score_word = [&](uint32_t i) {
    PLAN_REQUIRE(!((c.missing_mask >> i) & 1u), "cursor: Missing bit on a _score part");
    PLAN_REQUIRE((c.value_bits[i] >> 32) == 0u, "cursor: _score value has bits above the f32");
    return ordered_score_bits((uint32_t)c.value_bits[i]);
  };
  if (n_parts == 0) {
    out[0] = score_word(0);
    out[1] = ~c.segment_ord;
    out[2] = ~c.doc_id;
    return;
  }
  for (uint32_t i = 0; i < kCursorWords; i++) out[i] = 0u;
  for (uint32_t i = 0; i < n_parts; i++) {
    const bool desc = order[i] == SLG_ORDER_DESC;
    if (kind[i] == 0) {
      const uint32_t a = score_word(i);
      out[3 * i + 2] = desc ? ~a : a;
      continue;
    }
    PLAN_REQUIRE(kind[i] == 1 || kind[i] == 2, "unknown sort field kind");
    if ((c.missing_mask >> i) & 1u) {
      out[3 * i] = 1u;  // Missing: after every value in both orders, keys 0 (as the columns)
      continue;
    }
    int64_t iv;
    double dv;
    std::memcpy(&iv, &c.value_bits[i], 8);
    std::memcpy(&dv, &c.value_bits[i], 8);
    uint64_t key = kind[i] == 1 ? i64_key(iv) : f64_key(dv);
    if (desc) key = ~key;
    out[3 * i + 1] = (uint32_t)(key >> 32);
    out[3 * i + 2] = (uint32_t)key;
  }
  out[kCursorWords - 2] = c.segment_ord;
  out[kCursorWords - 1] = c.doc_id;
}

}  // namespace slgplan
