// plan_digest.cpp — stand-alone driver of the host planner (slg_plan.hpp's public interface only; no HIP,
// no Python).  It plans a fixed, seeded list of batches and prints one line per case: the error code and
// message, or a 64-bit FNV-1a digest over everything plan_batch returns (the packed image, q_postings,
// q_filter, every counter, flag and image offset of Plan).  Two builds of the planner compute the same iff
// their outputs are identical under diff; being its own program, it is also what the sanitizers run.
//   g++ -O2 -std=c++17 -pthread tools/plan_digest.cpp slg_plan.cpp -o plan_digest      (from csrc/)
//   plan_digest                      the digest lines
//   plan_digest --time [log2_vocab]  median / minimum ms of plan_batch on two batches shaped like the
//                                    benchmark's configs 2 and 3 (champion tables of 2^log2_vocab terms)
#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "../slg_plan.hpp"

namespace {

using slgplan::BatchIn;
using slgplan::Plan;
using slgplan::SegView;

constexpr uint32_t kChamp = 68;  // floats per row of a champion table (slg::kChampions)
constexpr int S = SLG_PLAN_SUM, D = SLG_PLAN_DISMAX, L = SLG_PLAN_LEAF;

struct Rng {  // splitmix64: the same numbers under every standard library
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint32_t below(uint32_t n) { return (uint32_t)((next() >> 32) % n); }
  float unit() { return (float)(next() >> 40) * (1.0f / 16777216.0f); }
};

struct Fnv {
  uint64_t h = 0xCBF29CE484222325ull;
  void bytes(const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001B3ull;
  }
  template <typename T>
  void val(T v) { bytes(&v, sizeof(v)); }
  template <typename T>
  void vec(const std::vector<T> &v) {
    val<uint64_t>(v.size());
    if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
  }
};

// ---- segments ------------------------------------------------------------------------------------
struct Seg {
  uint32_t n_docs = 0, n_terms = 0;
  std::vector<uint64_t> offs;
  std::vector<float> champ;
};

// shape 0: a mix of list lengths, every 13th term without a posting; 1: terms 0 and 1 are stop words, the
// others rare (12 .. 15 postings); 2: lists of similar density
Seg make_seg(Rng &r, uint32_t n_docs, uint32_t n_terms, bool champs, int shape = 0) {
  Seg s;
  s.n_docs = n_docs;
  s.n_terms = n_terms;
  s.offs.assign(n_terms + 1, 0);
  if (champs) s.champ.assign((size_t)n_terms * kChamp, 0.0f);
  for (uint32_t t = 0; t < n_terms; t++) {
    uint32_t df;
    if (shape == 1)
      df = t < 2 ? n_docs - n_docs / 10 : 12 + r.below(4);
    else if (shape == 2)
      df = n_docs / 4 + r.below(n_docs / 8);
    else
      df = t % 13 == 7 ? 0 : 1 + r.below(r.below(4) == 0 ? n_docs / 2 : n_docs / 20);
    s.offs[t + 1] = s.offs[t] + df;
    if (!champs || df == 0) continue;
    const float top = 1.0f + std::log((float)n_docs / (float)df) + r.unit();
    float *row = s.champ.data() + (size_t)t * kChamp;
    for (uint32_t i = 0; i < 64 && i < df; i++) row[i] = top * (1.0f - 0.004f * (float)i);
    for (uint32_t j = 0; j < 4; j++)
      if (df >= (128u << j)) row[64 + j] = top * (0.6f - 0.1f * (float)j);
  }
  return s;
}

std::vector<Seg> make_segs(uint64_t seed, uint32_t n, uint32_t n_terms, bool champs, int shape = 0) {
  Rng r{seed};
  std::vector<Seg> v;
  for (uint32_t i = 0; i < n; i++) v.push_back(make_seg(r, (shape == 1 ? 4 : 1) * (700 + 900 * i + r.below(300)), n_terms, champs, shape));
  return v;
}

slg_tuning default_tuning() {
  slg_tuning t;
  std::memset(&t, 0, sizeof(t));
  t.struct_size = sizeof(t);
  t.validate = t.champions = 1;
  t.pruning = -1;
  t.uniform_max_terms = 8;
  t.multi_round_target = 448;
  t.probe_target = 2048;
  t.slices_per_subquery = 16;
  t.cand_mode = t.slice_order = t.block_max = 1;
  t.uniform_kernel = 4;
  t.inline_cuts = -1;
  t.updatable = t.uniform_plans = 1;
  return t;
}

// ---- a batch under construction ------------------------------------------------------------------
struct Batch {
  uint32_t n_segs = 1, k = 11;
  int strategy = SLG_STRATEGY_WAND;
  bool sorted = false;
  slg_tuning tn = default_tuning();
  std::vector<uint32_t> offs{0}, tids;
  std::vector<float> w;
  std::vector<int32_t> filt;
  std::string live = std::string("\1\0\1", 3);  // filter 1 is not registered
  std::vector<uint32_t> leaf, nleaves, leaf_offs, leaf_group, group_offs, node_offs, node_parent, min_match;
  std::vector<int32_t> qplan, group_plan, node_kind;
  std::vector<float> qtie, group_tie, node_tie;
  // arrays to pass as NULL although they are filled, and q_offsets itself
  bool null_offs = false, null_tids = false, null_w = false, null_node_kind = false, null_group_plan = false;

  uint32_t nq() const { return (uint32_t)offs.size() - 1; }
  void term(const std::vector<uint32_t> &row, float weight) {
    tids.insert(tids.end(), row.begin(), row.end());
    w.push_back(weight);
  }
  void end_query() { offs.push_back((uint32_t)w.size()); }
  // nq queries of nt(q) random terms below `vocab`; no_term: one id in that many is SLG_NO_TERM;
  // wmode 0: positive weights, 1: zero and negative ones among them
  void random_queries(Rng &r, uint32_t n, const std::function<uint32_t(uint32_t)> &nt, uint32_t vocab,
                      uint32_t no_term = 0, int wmode = 0) {
    for (uint32_t q = 0; q < n; q++) {
      const uint32_t T = nt(q);
      for (uint32_t i = 0; i < T; i++) {
        std::vector<uint32_t> row(n_segs);
        for (auto &id : row) id = no_term && r.below(no_term) == 0 ? SLG_NO_TERM : r.below(vocab);
        float weight = 0.25f + 2.0f * r.unit();
        if (wmode == 1 && r.below(4) == 0) weight = r.below(2) ? 0.0f : -weight;
        term(row, weight);
      }
      end_query();
    }
  }
  void random_queries(Rng &r, uint32_t n, uint32_t T, uint32_t vocab, uint32_t no_term = 0, int wmode = 0) {
    random_queries(r, n, [T](uint32_t) { return T; }, vocab, no_term, wmode);
  }
  uint32_t terms_of(uint32_t q) const { return offs[q + 1] - offs[q]; }
};

template <typename T>
const T *ptr(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

BatchIn view(const Batch &b) {
  BatchIn in;
  in.nq = b.nq();
  in.q_offsets = b.null_offs ? nullptr : b.offs.data();
  in.q_term_ids = b.null_tids ? nullptr : ptr(b.tids);
  in.q_weights = b.null_w ? nullptr : ptr(b.w);
  in.plans.q_leaf = ptr(b.leaf);
  in.plans.q_plan = ptr(b.qplan);
  in.plans.q_tie = ptr(b.qtie);
  in.plans.q_nleaves = ptr(b.nleaves);
  in.plans.q_leaf_offsets = ptr(b.leaf_offs);
  in.plans.leaf_group = ptr(b.leaf_group);
  in.plans.q_group_offsets = ptr(b.group_offs);
  in.plans.group_plan = b.null_group_plan ? nullptr : ptr(b.group_plan);
  in.plans.group_tie = ptr(b.group_tie);
  in.plans.q_node_offsets = ptr(b.node_offs);
  in.plans.node_kind = b.null_node_kind ? nullptr : ptr(b.node_kind);
  in.plans.node_tie = ptr(b.node_tie);
  in.plans.node_parent = ptr(b.node_parent);
  in.plans.q_min_match = ptr(b.min_match);
  in.q_filter = ptr(b.filt);
  in.k = b.k;
  in.strategy = b.strategy;
  in.filter_live = b.live.data();
  in.n_filters = b.live.size();
  in.sorted = b.sorted;
  return in;
}

std::vector<SegView> views(const std::vector<Seg> &segs) {
  std::vector<SegView> v(segs.size());
  for (size_t i = 0; i < segs.size(); i++) {
    v[i].n_docs = segs[i].n_docs;
    v[i].n_terms = segs[i].n_terms;
    v[i].term_offsets = segs[i].offs.data();
    v[i].champ = segs[i].champ.empty() ? nullptr : segs[i].champ.data();
  }
  return v;
}

uint64_t digest(const Plan &p) {
  Fnv f;
  std::vector<unsigned char> img(p.image_bytes, 0);
  p.pack(img.data());
  f.vec(img);
  f.vec(p.q_postings);
  f.vec(p.q_filter);
  for (uint64_t v : {p.n_postings, p.n_postings_essential, p.n_postings_nonessential, p.n_rounds, p.n_bounds, p.n_bnd,
                     p.cand_total, (uint64_t)p.max_terms})
    f.val(v);
  for (bool v : {p.uniform, p.multi, p.plan_batch, p.nested, p.deep, p.pruned, p.cand_mode}) f.val<uint8_t>(v);
  for (size_t v : {p.o_sq, p.o_terms, p.o_slice, p.o_sseg, p.o_sord, p.o_q, p.o_bc, p.o_nodes, p.image_bytes})
    f.val<uint64_t>(v);
  for (size_t v : {p.sqs.size(), p.terms.size(), p.slice_sq.size(), p.slice_seg.size(), p.slice_order.size(),
                   p.qrefs.size(), p.bnd_coarse.size(), p.nodes.size()})
    f.val<uint64_t>(v);
  return f.h;
}

void run(const std::string &name, const std::vector<Seg> &segs, const Batch &b) {
  Plan p;
  try {
    slgplan::plan_batch(views(segs), b.tn, view(b), p);
  } catch (const slgplan::SlgError &e) {
    std::printf("%s: error %d %s\n", name.c_str(), e.code, e.what());
    return;
  }
  std::printf("%s: ok %016" PRIx64 " sq=%zu slices=%zu nodes=%zu %s%s%s%s%s%s\n", name.c_str(), digest(p), p.sqs.size(),
              p.slice_sq.size(), p.nodes.size(), p.uniform ? "uniform" : "multi", p.plan_batch ? " plans" : "",
              p.nested ? " nested" : "", p.deep ? " deep" : "", p.pruned ? " pruned" : "", p.cand_mode ? " cand" : "");
}

// ---- score plans -----------------------------------------------------------------------------------
// q_leaf: every term of every query names one of its query's n_leaf(q) leaves
void random_leaves(Batch &b, Rng &r, const std::function<uint32_t(uint32_t)> &n_leaf) {
  for (uint32_t q = 0; q < b.nq(); q++)
    for (uint32_t i = 0; i < b.terms_of(q); i++) b.leaf.push_back(r.below(n_leaf(q)));
}

// appends a random tree in pre-order whose deepest leaf is at `depth`; leaves hang at every level above it
// too when `uneven`.  Returns its leaves
uint32_t random_tree(Batch &b, Rng &r, uint32_t depth, bool uneven) {
  const uint32_t base = (uint32_t)b.node_kind.size();
  uint32_t leaves = 0;
  std::function<void(uint32_t, uint32_t, bool)> grow = [&](uint32_t d, uint32_t parent, bool spine) {
    const uint32_t me = (uint32_t)b.node_kind.size() - base;
    b.node_parent.push_back(parent);
    b.node_tie.push_back(0.0f);
    if (d == depth || (!spine && d > 0 && uneven && r.below(3) == 0)) {
      b.node_kind.push_back(L);
      leaves++;
      return;
    }
    const bool dismax = r.below(2) != 0;
    b.node_kind.push_back(dismax ? D : S);
    if (dismax) b.node_tie.back() = std::vector<float>{0.0f, 0.3f, 1.0f}[r.below(3)];
    const uint32_t kids = 1 + r.below(3), on_spine = r.below(kids);
    for (uint32_t c = 0; c < kids; c++) grow(d + 1, me, spine && c == on_spine);
  };
  if (b.node_offs.empty()) b.node_offs.push_back(0);
  grow(0, 0, true);
  b.node_offs.push_back((uint32_t)b.node_kind.size());
  return leaves;
}

// a tree written out: kinds, ties, parents
void tree(Batch &b, const std::vector<int> &kind, const std::vector<float> &tie, const std::vector<uint32_t> &parent) {
  if (b.node_offs.empty()) b.node_offs.push_back(0);
  b.node_kind.insert(b.node_kind.end(), kind.begin(), kind.end());
  b.node_tie.insert(b.node_tie.end(), tie.begin(), tie.end());
  b.node_parent.insert(b.node_parent.end(), parent.begin(), parent.end());
  b.node_offs.push_back((uint32_t)b.node_kind.size());
}

// trees of depth depth(q) over queries already in b, and the q_leaf that goes with them
void random_trees(Batch &b, Rng &r, const std::function<uint32_t(uint32_t)> &depth, bool uneven = true) {
  std::vector<uint32_t> n_leaf;
  for (uint32_t q = 0; q < b.nq(); q++) n_leaf.push_back(random_tree(b, r, depth(q), uneven));
  random_leaves(b, r, [&](uint32_t q) { return n_leaf[q]; });
}

// two-level plans in the caller's form: query q has nl(q) leaves in groups of 1 .. 3 consecutive leaves
// (flat: one Sum group per leaf); leaves beyond the ones the terms name have no term
void two_level(Batch &b, Rng &r, const std::function<uint32_t(uint32_t)> &nl, bool flat, bool dismax_groups) {
  b.leaf_offs.push_back(0);
  b.group_offs.push_back(0);
  for (uint32_t q = 0; q < b.nq(); q++) {
    const uint32_t n = nl(q);
    uint32_t g = 0;
    for (uint32_t l = 0; l < n;) {
      const uint32_t len = flat ? 1 : 1 + r.below(3);
      for (uint32_t j = 0; j < len && l < n; j++, l++) b.leaf_group.push_back(g);
      const bool dm = dismax_groups && r.below(2) != 0;
      b.group_plan.push_back(dm ? D : S);
      b.group_tie.push_back(dm ? 0.5f * (float)r.below(3) : 0.0f);
      g++;
    }
    b.leaf_offs.push_back((uint32_t)b.leaf_group.size());
    b.group_offs.push_back((uint32_t)b.group_plan.size());
    b.nleaves.push_back(n);
    b.qplan.push_back(r.below(2) ? D : S);
    b.qtie.push_back(b.qplan.back() == D ? 0.3f : 0.0f);
  }
}


// ---- the cases -----------------------------------------------------------------------------------
constexpr uint32_t V = 60;  // terms of every small segment
using Edit = std::function<void(Batch &)>;

Batch flat(uint64_t seed, uint32_t n_segs, uint32_t nq, uint32_t T, uint32_t no_term = 0, int wmode = 0) {
  Rng r{seed};
  Batch b;
  b.n_segs = n_segs;
  b.random_queries(r, nq, T, V, no_term, wmode);
  return b;
}

void filters(Batch &b, int mode) {  // 1: every query filtered; 2: some
  for (uint32_t q = 0; q < b.nq(); q++) b.filt.push_back(mode == 1 ? (q % 2 ? 2 : 0) : (q % 3 == 0 ? 0 : q % 7 == 0 ? 2 : -1));
}

void cases_k_and_segments() {
  for (uint32_t n_segs = 1; n_segs <= 3; n_segs++)
    for (int champs = 0; champs <= 1; champs++) {
      const std::vector<Seg> segs = make_segs(10 + n_segs, n_segs, V, champs != 0);
      for (uint32_t k : {0u, 1u, 11u, 101u, 256u, 257u, 1024u, 1025u, (uint32_t)SLG_MAX_K})
        for (int sorted = 0; sorted <= 1; sorted++) {
          Rng r{1000 + k};
          Batch b;
          b.n_segs = n_segs;
          b.k = k;
          b.sorted = sorted != 0;
          // query 5 is empty; one id in five is SLG_NO_TERM (one-term queries: no term in any segment)
          b.random_queries(r, 24, [](uint32_t q) { return q == 5 ? 0u : 1u + q % 5; }, V, 5, 1);
          run("k segs=" + std::to_string(n_segs) + " champs=" + std::to_string(champs) + " k=" + std::to_string(k) +
                  " sorted=" + std::to_string(sorted), segs, b);
        }
    }
  const std::vector<Seg> segs = make_segs(20, 2, V, true);
  Batch none;
  none.n_segs = 2;
  run("nq=0", segs, none);
  Batch missing = flat(21, 2, 5, 3);
  std::fill(missing.tids.begin(), missing.tids.end(), SLG_NO_TERM);
  run("no term in any segment", segs, missing);
  Batch one = flat(22, 2, 1, 2);
  run("nq=1", segs, one);
  run("nq=64", segs, flat(23, 2, 64, 3, 6, 1));
}

void cases_strategy_terms_weights_filters() {
  const std::vector<Seg> segs = make_segs(30, 2, V, true);
  for (int strategy : {SLG_STRATEGY_BM25, SLG_STRATEGY_WAND, SLG_STRATEGY_BMW})
    for (uint32_t T : {1u, 4u, 5u, 8u, 9u, 13u, 32u, (uint32_t)SLG_MAX_QUERY_TERMS})
      for (uint32_t k : {11u, 300u}) {
        Batch b = flat(3000 + T, 2, 16, T, 9);
        b.strategy = strategy;
        b.k = k;
        run("strategy=" + std::to_string(strategy) + " T=" + std::to_string(T) + " k=" + std::to_string(k), segs, b);
      }
  for (int wm = 0; wm < 4; wm++) {  // positive / all zero / all negative / mixed
    Batch b = flat(3100, 2, 16, 4, 0, wm == 3 ? 1 : 0);
    for (float &x : b.w) x = wm == 1 ? 0.0f : wm == 2 ? -x : x;
    run("weights mode=" + std::to_string(wm), segs, b);
  }
  for (int fm = 0; fm < 3; fm++)
    for (uint32_t T : {3u, 6u, 12u}) {
      Batch b = flat(3200 + T, 2, 32, T);
      if (fm) filters(b, fm);
      run("filters mode=" + std::to_string(fm) + " T=" + std::to_string(T), segs, b);
    }
}

// 5-term queries: one stop word among rare terms (segments of shape 1: the classification is kept), or lists
// of similar density (shape 2: it is dropped)
Batch five_terms(uint64_t seed, uint32_t n_segs, uint32_t nq, bool stop_word) {
  Rng r{seed};
  Batch b;
  b.n_segs = n_segs;
  for (uint32_t q = 0; q < nq; q++) {
    for (uint32_t i = 0; i < 5; i++) {
      std::vector<uint32_t> row(n_segs);
      for (auto &id : row) id = stop_word && i == q % 5 ? r.below(2) : 2 + r.below(V - 2);
      b.term(row, 1.0f);
    }
    b.end_query();
  }
  return b;
}

void cases_tuning() {
  const std::vector<Seg> skewed = make_segs(40, 2, V, true, 1), even = make_segs(41, 2, V, true, 2),
                         mixed = make_segs(42, 2, V, true);
  Rng r{43};
  Batch shared = flat(44, 2, 24, 3);
  random_leaves(shared, r, [](uint32_t) { return 2u; });
  const Batch stop = five_terms(45, 2, 32, true), dense = five_terms(46, 2, 32, false), nine = flat(47, 2, 16, 9);
  struct Shape { const char *name; const std::vector<Seg> *segs; const Batch *b; };
  const Shape shapes[] = {{"stop-word", &skewed, &stop}, {"similar-density", &even, &dense},
                          {"shared-leaves", &mixed, &shared}, {"nine-terms", &skewed, &nine}};
  for (const Shape &sh : shapes) {
    for (int pruning = -1; pruning <= 1; pruning++)
      for (int block_max = 0; block_max <= 1; block_max++)
        for (int uniform_plans = 0; uniform_plans <= 1; uniform_plans++)
          for (uint32_t umt : {4u, 8u})
            for (int strategy : {SLG_STRATEGY_WAND, SLG_STRATEGY_BMW}) {
              Batch b = *sh.b;
              b.strategy = strategy;
              b.tn.pruning = pruning;
              b.tn.block_max = block_max;
              b.tn.uniform_plans = uniform_plans;
              b.tn.uniform_max_terms = umt;
              run(std::string("tuning ") + sh.name + " pruning=" + std::to_string(pruning) + " block_max=" +
                      std::to_string(block_max) + " uniform_plans=" + std::to_string(uniform_plans) +
                      " uniform_max_terms=" + std::to_string(umt) + " strategy=" + std::to_string(strategy), *sh.segs, b);
            }
    for (uint32_t rps : {0u, 1u, 4u, 40u})
      for (uint32_t max_rps : {0u, 2u, 12u})
        for (int order = 0; order <= 1; order++)
          for (uint32_t k : {11u, 101u}) {
            Batch b = *sh.b;
            b.k = k;
            b.tn.rounds_per_slice = rps;
            b.tn.max_rounds_per_slice = max_rps;
            b.tn.slice_order = order;
            run(std::string("slices ") + sh.name + " rounds_per_slice=" + std::to_string(rps) + " max=" +
                    std::to_string(max_rps) + " slice_order=" + std::to_string(order) + " k=" + std::to_string(k), *sh.segs, b);
          }
    for (int v = 0; v < 4; v++) {
      Batch b = *sh.b;
      if (v == 0) b.tn.uniform_round_target = 96;
      if (v == 1) b.tn.uniform_sigma_x100 = 100;
      if (v == 2) b.tn.multi_round_target = 100, b.tn.probe_target = 600;
      if (v == 3) b.tn.slices_per_subquery = 2;
      run(std::string("targets ") + sh.name + " variant=" + std::to_string(v), *sh.segs, b);
    }
  }
}

void cases_score_plans() {
  const std::vector<Seg> segs = make_segs(50, 2, V, true);
  Rng r{51};
  for (uint32_t T : {3u, 6u, 12u}) {
    Batch b = flat(5000 + T, 2, 24, T, 7);
    random_leaves(b, r, [T](uint32_t) { return std::max(1u, T / 2); });
    run("q_leaf shared T=" + std::to_string(T), segs, b);
    for (float tie : {0.0f, 0.3f, 1.0f})
      for (int with_nleaves = 0; with_nleaves <= 1; with_nleaves++) {
        Batch d = b;
        d.qplan.assign(d.nq(), D);
        for (uint32_t q = 0; q < d.nq(); q += 4) d.qplan[q] = S;
        d.qtie.assign(d.nq(), tie);
        if (with_nleaves) d.nleaves.assign(d.nq(), T);  // (leaves beyond T / 2 have no term)
        run("dismax T=" + std::to_string(T) + " tie=" + std::to_string(tie) + " q_nleaves=" + std::to_string(with_nleaves), segs, d);
      }
    Batch plain = flat(5100 + T, 2, 24, T, 7);
    plain.qplan.assign(plain.nq(), D);
    plain.qtie.assign(plain.nq(), 0.3f);
    run("dismax without q_leaf T=" + std::to_string(T), segs, plain);
  }
  for (uint32_t T : {2u, 4u, 8u})
    for (int with_leaves = 0; with_leaves <= 1; with_leaves++) {
      Batch b = flat(5200 + T, 2, 16, T, 9);
      if (with_leaves) random_leaves(b, r, [T](uint32_t) { return T; });
      for (uint32_t q = 0; q < b.nq(); q++) b.min_match.push_back(std::vector<uint32_t>{0, 1, 2, 255}[q % 4]);
      run("q_min_match T=" + std::to_string(T) + " q_leaf=" + std::to_string(with_leaves), segs, b);
      b.qplan.assign(b.nq(), D);
      b.qtie.assign(b.nq(), 0.5f);
      run("q_min_match dismax T=" + std::to_string(T) + " q_leaf=" + std::to_string(with_leaves), segs, b);
    }
  // two-level plans in the caller's form
  for (int form = 0; form < 4; form++)  // flat-equivalent / nested Sum groups / DisMax groups / leaves without a term
    for (uint32_t T : {4u, 9u})
      for (uint32_t k : {11u, 300u}) {
        Batch b = flat(5300 + T, 2, 16, T, 8);
        b.k = k;
        const uint32_t named = form == 0 ? T : std::max(2u, T / 2);
        random_leaves(b, r, [named](uint32_t) { return named; });
        if (form == 0)  // every leaf named, so that no term shares one either
          for (uint32_t q = 0; q < b.nq(); q++)
            for (uint32_t i = 0; i < T; i++) b.leaf[b.offs[q] + i] = i;
        two_level(b, r, [&](uint32_t q) { return form == 3 ? named + 1 + q % 3 : named; }, form == 0, form >= 2);
        if (form == 0) b.qplan.assign(b.nq(), S);
        run("two-level form=" + std::to_string(form) + " T=" + std::to_string(T) + " k=" + std::to_string(k), segs, b);
      }
  // trees node by node: depth 0 (a single leaf) .. SLG_MAX_PLAN_DEPTH, and batches that mix them
  for (uint32_t depth = 0; depth <= SLG_MAX_PLAN_DEPTH + 1; depth++)
    for (int uneven = 0; uneven <= 1; uneven++)
      for (uint32_t T : {3u, 10u})
        for (int fm : {0, 2}) {
          Batch b = flat(5400 + 10 * depth + T, 2, 20, T, 8);
          if (fm) filters(b, fm);
          random_trees(b, r, [depth](uint32_t q) { return depth > SLG_MAX_PLAN_DEPTH ? q % (SLG_MAX_PLAN_DEPTH + 1) : depth; },
                       uneven != 0);
          run("trees depth=" + (depth > SLG_MAX_PLAN_DEPTH ? std::string("mixed") : std::to_string(depth)) + " uneven=" +
                  std::to_string(uneven) + " T=" + std::to_string(T) + " filters=" + std::to_string(fm), segs, b);
        }
  {
    Batch b = flat(5500, 2, 3, 4);
    tree(b, {S, L, D, L, L, L}, {0, 0, .5f, 0, 0, 0}, {0, 0, 0, 2, 2, 0});        // depth 2: bare leaves beside a group
    tree(b, {S, S, S, L, L}, {0, 0, 0, 0, 0}, {0, 0, 0, 2, 1});                    // accepted although not in pre-order
    tree(b, {D, L, S, L, S, L, D, L, L}, {1, 0, 0, 0, 0, 0, .3f, 0, 0}, {0, 0, 0, 2, 2, 4, 4, 6, 6});  // leaves at depths 1 .. 4
    b.leaf = {0, 1, 2, 3, 0, 1, 1, 0, 0, 2, 4, 4};
    run("trees written out", segs, b);
    b.k = 0;
    run("trees written out k=0", segs, b);
  }
  for (int shape = 0; shape < 3; shape++) {  // the limits: 255 leaves under the root; 510 nodes in 255 groups; the same, deep
    Batch b = flat(5600, 2, 2, 32, 8);
    for (uint32_t q = 0; q < 2; q++) {
      std::vector<int> kind{S};
      std::vector<uint32_t> parent{0};
      if (shape == 0)
        for (uint32_t i = 0; i < 255; i++) kind.push_back(L), parent.push_back(0);
      for (uint32_t g = 0; shape != 0 && g < (shape == 1 ? 254u : 127u); g++) {
        const uint32_t at = (uint32_t)kind.size();
        kind.push_back(g % 2 ? D : S), parent.push_back(0);
        if (shape == 2) kind.push_back(S), parent.push_back(at);
        for (uint32_t l = 0; l < (shape == 1 ? 1u : 2u); l++) kind.push_back(L), parent.push_back((uint32_t)(shape == 2 ? at + 1 : at));
      }
      if (shape != 0) kind.push_back(L), parent.push_back(0);
      tree(b, kind, std::vector<float>(kind.size(), 0.25f), parent);
    }
    random_leaves(b, r, [](uint32_t) { return 255u; });
    run("trees at the limits shape=" + std::to_string(shape), segs, b);
  }
}

// >= 8192 sub-queries over 4 segments: pass 1 runs on several threads where the CPU budget gives them
Batch threaded_deep(uint64_t seed) {
  Rng r{seed};
  Batch b = flat(seed + 1, 4, 2304, 4, 6);
  filters(b, 2);
  random_trees(b, r, [](uint32_t q) { return q % (SLG_MAX_PLAN_DEPTH + 1); });
  return b;
}

void cases_threaded() {
  const std::vector<Seg> segs = make_segs(60, 4, V, true), skewed = make_segs(61, 4, V, true, 1);
  run("threaded flat", segs, flat(62, 4, 2304, 3, 6, 1));
  run("threaded deep trees and filters", segs, threaded_deep(63));
  run("threaded stop-word", skewed, five_terms(64, 4, 2560, true));
  Batch big_k = flat(65, 4, 2304, 6);
  big_k.k = 300;
  run("threaded k=300", segs, big_k);
  for (int where = 0; where < 4; where++) {  // which error a threaded batch reports
    Batch b = where < 2 ? flat(66, 4, 2304, 3) : threaded_deep(67);
    if (where == 0) b.tids[10 * 3 * 4 + 1] = V, b.tids[2300 * 3 * 4 + 2] = V + 1;  // early and late: the early one
    if (where == 1) b.tids[2300 * 3 * 4 + 2] = V;                                  // late only
    if (where == 2) b.w[2303 * 4] = INFINITY, b.filt[9] = 1;                       // early filter, late weight
    if (where == 3) b.tids[5 * 4 * 4] = V, b.node_kind.back() = 9;                 // pass 1 early, validation late
    run("threaded malformed where=" + std::to_string(where), segs, b);
  }
}

void cases_malformed() {
  const std::vector<Seg> segs = make_segs(70, 2, V, true);
  Rng r{71};
  const Batch plain = flat(72, 2, 6, 3);
  Batch trees = plain, groups = plain, leaves = plain;
  random_trees(trees, r, [](uint32_t q) { return 1 + q % 3; });
  random_leaves(groups, r, [](uint32_t) { return 3u; });
  two_level(groups, r, [](uint32_t) { return 4u; }, false, true);
  random_leaves(leaves, r, [](uint32_t) { return 2u; });
  int n = 0;
  auto bad = [&](const Batch &base, const char *what, const Edit &edit) {
    Batch b = base;
    edit(b);
    run("malformed " + std::to_string(n++) + " " + what, segs, b);
  };
  // a tree written out, as query 2 of `plain` (single leaves elsewhere; three terms name leaves 0 .. 2)
  auto bad_tree = [&](const char *what, const std::vector<int> &kind, const std::vector<float> &tie,
                      const std::vector<uint32_t> &parent, const std::vector<uint32_t> &leaf = {}) {
    Batch b = plain;
    for (uint32_t q = 0; q < b.nq(); q++) {
      if (q == 2 && kind.empty())
        b.node_offs.push_back(b.node_offs.back());
      else if (q == 2)
        tree(b, kind, tie, parent);
      else
        tree(b, {S, L, L, L}, {0, 0, 0, 0}, {0, 0, 0, 0});
    }
    if (!leaf.empty())
      for (uint32_t q = 0; q < b.nq(); q++) b.leaf.insert(b.leaf.end(), leaf.begin(), leaf.end());
    run("malformed " + std::to_string(n++) + " " + what, segs, b);
  };
  const float nan = std::numeric_limits<float>::quiet_NaN();
  // ---- validate_batch ----
  bad(plain, "q_offsets NULL", [](Batch &b) { b.null_offs = true; });
  bad(plain, "strategy", [](Batch &b) { b.strategy = 7; });
  bad(plain, "k", [](Batch &b) { b.k = SLG_MAX_K + 1; });
  bad(plain, "q_term_ids NULL", [](Batch &b) { b.null_tids = true; });
  bad(plain, "q_weights NULL", [](Batch &b) { b.null_w = true; });
  bad(plain, "q_offsets decrease", [](Batch &b) { b.offs[3] = b.offs[2] - 1; });
  bad(plain, "q_offsets beyond the total", [](Batch &b) { b.offs[1] = 1000000; });
  bad(plain, "33 terms", [](Batch &b) { b = Batch(); b.n_segs = 2; Rng r2{73}; b.random_queries(r2, 3, [](uint32_t q) { return q == 1 ? 33u : 2u; }, V); });
  bad(plain, "q_min_match 256", [](Batch &b) { b.min_match.assign(b.nq(), 1); b.min_match[3] = 256; });
  bad(trees, "node_kind NULL", [](Batch &b) { b.null_node_kind = true; });
  bad(trees, "q_node_offsets decrease", [](Batch &b) { b.node_offs[2] = b.node_offs[1] - 1; });
  bad_tree("tree without a node", {}, {}, {});
  bad_tree("511 nodes", std::vector<int>(511, L), std::vector<float>(511, 0.0f), std::vector<uint32_t>(511, 0));
  bad_tree("node kind", {S, L, 3, L}, {0, 0, 0, 0}, {0, 0, 0, 0});
  bad_tree("parent comes later", {S, L, L, L}, {0, 0, 0, 0}, {0, 2, 0, 0});
  bad_tree("parent is the node itself", {S, L, L, L}, {0, 0, 0, 0}, {0, 0, 2, 0});
  bad_tree("leaf with a child", {S, L, L, L}, {0, 0, 0, 0}, {0, 0, 1, 0});
  bad_tree("not in pre-order", {S, S, L, S, L, L}, {0, 0, 0, 0, 0, 0}, {0, 0, 1, 0, 1, 3});
  bad_tree("node tie 1.5", {S, D, L, L, L}, {0, 1.5f, 0, 0, 0}, {0, 0, 1, 1, 0});
  bad_tree("node tie NaN", {D, L, L, L}, {nan, 0, 0, 0}, {0, 0, 0, 0});
  bad_tree("node tie of a Sum is not read", {S, L, L, L}, {7, 0, 0, 0}, {0, 0, 0, 0});
  bad_tree("Sum without children", {S, L, L, L, D}, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0});
  {
    std::vector<int> kind(257, L);
    kind[0] = S;
    bad_tree("256 leaves", kind, std::vector<float>(257, 0.0f), std::vector<uint32_t>(257, 0));
  }
  bad_tree("deeper than the limit", {S, S, S, S, S, L, L, L}, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 1, 2, 3, 4, 0, 0});
  bad_tree("term position beyond the leaves", {S, L, L}, {0, 0, 0}, {0, 0, 0});
  bad_tree("q_leaf beyond the leaves", {S, L, L, L}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 3, 1});
  bad(groups, "group_plan NULL", [](Batch &b) { b.null_group_plan = true; });
  bad(groups, "q_nleaves NULL", [](Batch &b) { b.nleaves.clear(); });
  bad(groups, "q_leaf_offsets decrease", [](Batch &b) { b.leaf_offs[3] = b.leaf_offs[2] - 1; });
  bad(groups, "q_group_offsets decrease", [](Batch &b) { b.group_offs[3] = b.group_offs[2] - 1; });
  bad(groups, "q_nleaves disagrees", [](Batch &b) { b.nleaves[4] = 5; });
  bad(groups, "leaf_group out of range", [](Batch &b) { b.leaf_group[b.leaf_offs[2] + 3] = 9; });
  bad(groups, "leaf_group decreases", [](Batch &b) { b.leaf_group[b.leaf_offs[2] + 3] = 0; b.leaf_group[b.leaf_offs[2] + 2] = 1; b.leaf_group[b.leaf_offs[2] + 1] = 1; });
  bad(groups, "leaf_group starts at 1", [](Batch &b) { b.leaf_group[b.leaf_offs[1]] = 1; b.leaf_group[b.leaf_offs[1] + 1] = 1; });
  bad(groups, "group plan", [](Batch &b) { b.group_plan[b.group_offs[3]] = 7; });
  bad(groups, "group tie", [](Batch &b) { b.group_tie[b.group_offs[3]] = -0.1f; });
  {
    // written out: query 0 has 2 leaves in 3 groups (a group without a leaf); 256 leaves; 256 groups; groups 0, 0, 2, 2
    for (int v = 0; v < 4; v++) {
      Batch b = flat(74, 2, 1, 2);
      const uint32_t nl = v == 0 ? 2 : v == 3 ? 4 : 256, ng = v == 0 || v == 3 ? 3 : v == 1 ? 1 : 256;
      b.leaf_offs = {0, nl};
      b.group_offs = {0, ng};
      for (uint32_t l = 0; l < nl; l++) b.leaf_group.push_back(v == 1 ? 0 : v == 3 ? l & 2 : l);
      b.group_plan.assign(ng, S);
      b.group_tie.assign(ng, 0.0f);
      b.nleaves = {nl};
      run("malformed " + std::to_string(n++) + (v == 0 ? " group without a leaf" : v == 1 ? " 256 leaves" : v == 2 ? " 256 groups" : " leaf_group with a gap"), segs, b);
    }
  }
  // ---- pass 1 ----
  bad(plain, "filter id beyond the table", [](Batch &b) { b.filt.assign(b.nq(), -1); b.filt[2] = 3; });
  bad(plain, "filter id not registered", [](Batch &b) { b.filt.assign(b.nq(), -1); b.filt[2] = 1; });
  bad(plain, "q_plan", [](Batch &b) { b.qplan.assign(b.nq(), S); b.qplan[4] = 5; });
  bad(plain, "q_plan LEAF", [](Batch &b) { b.qplan.assign(b.nq(), D); b.qplan[4] = L; });
  bad(plain, "q_tie 1.5", [](Batch &b) { b.qtie.assign(b.nq(), 0.5f); b.qtie[1] = 1.5f; });
  bad(plain, "q_tie NaN", [&](Batch &b) { b.qtie.assign(b.nq(), 0.5f); b.qtie[1] = nan; });
  bad(leaves, "leaf index 2^31", [](Batch &b) { b.leaf[7] = 0x80000000u; });
  bad(groups, "leaf beyond q_nleaves", [](Batch &b) { b.leaf[b.offs[3] + 1] = 4; });
  bad(plain, "term id = n_terms", [](Batch &b) { b.tids[9] = V; });
  bad(plain, "weight inf", [](Batch &b) { b.w[5] = INFINITY; });
  bad(plain, "weight NaN", [&](Batch &b) { b.w[5] = nan; });
  bad(plain, "term id out of range where k = 0 (not looked at)", [](Batch &b) { b.tids[9] = V; b.k = 0; });
  bad(leaves, "leaf index 2^31 where k = 0", [](Batch &b) { b.leaf[7] = 0x80000000u; b.k = 0; });
  bad(groups, "leaf beyond q_nleaves where k = 0", [](Batch &b) { b.leaf[b.offs[3] + 1] = 4; b.k = 0; });
  bad(plain, "unregistered filter where k = 0", [](Batch &b) { b.filt.assign(b.nq(), -1); b.filt[2] = 1; b.k = 0; });
  // ---- after pass 1 ----
  bad(flat(75, 2, 4, 9), "q_min_match 2 with nine lists", [](Batch &b) { b.min_match.assign(b.nq(), 2); });
  bad(groups, "q_min_match 2 with a two-level plan", [](Batch &b) { b.min_match.assign(b.nq(), 2); });
  {
    // lists of 4e9 postings (the planner reads the offsets only): more cut points, more slice candidates, than 32 bits index
    Seg huge;
    huge.n_docs = 0xFFFFFFFFu;
    huge.n_terms = 32;
    for (uint64_t t = 0; t <= 32; t++) huge.offs.push_back(t * 4000000000ull);
    Batch b;
    for (uint32_t i = 0; i < 32; i++) b.term({i}, 1.0f);
    b.end_query();
    run("malformed " + std::to_string(n++) + " batch too large (bounds)", {huge}, b);
    Batch c;
    c.term({0}, 1.0f);
    c.end_query();
    c.k = 256;
    c.tn.rounds_per_slice = 1;
    c.tn.uniform_round_target = 48;
    run("malformed " + std::to_string(n++) + " batch too large (rounds)", {huge}, c);
  }
  // ---- two defects: which one is reported ----
  bad(plain, "pair: term id in query 1, weight in query 4", [](Batch &b) { b.tids[3 * 2] = V; b.w[12] = INFINITY; });
  bad(plain, "pair: weight in query 1, term id in query 4", [](Batch &b) { b.w[3] = INFINITY; b.tids[12 * 2] = V; });
  bad(plain, "pair: weight of term 1, id of term 0 in segment 1", [](Batch &b) { b.w[1] = INFINITY; b.tids[1] = V; });
  bad(plain, "pair: id of term 2 in segment 0, weight of term 0 in segment 1 only", [](Batch &b) { b.tids[4] = V; b.tids[0] = SLG_NO_TERM; b.w[0] = INFINITY; });
  bad(plain, "pair: filter and q_plan of query 2", [](Batch &b) { b.filt.assign(b.nq(), -1); b.filt[2] = 1; b.qplan.assign(b.nq(), S); b.qplan[2] = 5; });
  bad(leaves, "pair: q_tie and leaf index of query 2", [](Batch &b) { b.qtie.assign(b.nq(), 0.0f); b.qtie[2] = 2.0f; b.leaf[6] = 0x80000000u; });
  bad(leaves, "pair: leaf index of query 3, term id of query 0", [](Batch &b) { b.leaf[9] = 0x80000000u; b.tids[0] = V; });
  bad(plain, "pair: term id in query 0 (pass 1), q_min_match 256 in query 5 (validation)", [](Batch &b) { b.tids[0] = V; b.min_match.assign(b.nq(), 0); b.min_match[5] = 256; });
  bad(plain, "pair: q_min_match 256 in query 0, q_offsets decrease at query 4", [](Batch &b) { b.min_match.assign(b.nq(), 0); b.min_match[0] = 256; b.offs[4] = b.offs[3] - 1; });
  bad(trees, "pair: filter of query 0 (pass 1), node kind of query 5 (validation)", [](Batch &b) { b.filt.assign(b.nq(), -1); b.filt[0] = 1; b.node_kind.back() = 9; });
  bad(trees, "pair: node kind in query 1 and in query 4", [](Batch &b) { b.node_kind[b.node_offs[1]] = 8; b.node_kind[b.node_offs[4]] = 9; });
  bad(groups, "pair: group plan of query 1, leaf_group of query 0", [](Batch &b) { b.group_plan[b.group_offs[1]] = 7; b.leaf_group[b.leaf_offs[0]] = 1; });
  bad(groups, "pair: group tie and group plan of one group", [](Batch &b) { b.group_plan[b.group_offs[1]] = 7; b.group_tie[b.group_offs[1]] = 2.0f; });
  bad(plain, "pair: k and strategy", [](Batch &b) { b.k = SLG_MAX_K + 1; b.strategy = 9; });
}

// ---- --time -----------------------------------------------------------------------------------------
void time_batch(const char *name, uint32_t log2_vocab, uint32_t n_segs, uint32_t nq, uint32_t T, uint32_t k) {
  const uint32_t vocab = 1u << log2_vocab;
  std::vector<Seg> segs(n_segs);
  Rng r{90 + n_segs};
  for (Seg &s : segs) {  // Zipf-like lists over 2M docs; a champion row per term
    s.n_docs = 2000000;
    s.n_terms = vocab;
    s.offs.assign((size_t)vocab + 1, 0);
    s.champ.resize((size_t)vocab * kChamp);
    for (uint32_t t = 0; t < vocab; t++) {
      const uint32_t df = 1 + (uint32_t)(400000.0 / (1.0 + 0.05 * (double)t)) + r.below(64);
      s.offs[t + 1] = s.offs[t] + df;
      const float top = 1.0f + std::log((float)s.n_docs / (float)df);
      float *row = s.champ.data() + (size_t)t * kChamp;
      for (uint32_t i = 0; i < kChamp; i++) row[i] = i < df ? top * (1.0f - 0.004f * (float)i) : 0.0f;
    }
  }
  Batch b;
  b.n_segs = n_segs;
  b.k = k;
  b.random_queries(r, nq, T, vocab);
  const std::vector<SegView> sv = views(segs);
  const BatchIn in = view(b);
  std::vector<double> ms;
  Plan p;
  for (int i = 0; i < 3 + 21; i++) {
    const auto t0 = std::chrono::steady_clock::now();
    slgplan::plan_batch(sv, b.tn, in, p);
    const auto t1 = std::chrono::steady_clock::now();
    if (i >= 3) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
  }
  std::sort(ms.begin(), ms.end());
  std::printf("%s: median %.4f ms  min %.4f ms  (%zu calls after 3 warm-up; %zu sub-queries, %s; champion tables %.0f MB)\n",
              name, ms[ms.size() / 2], ms[0], ms.size(), p.sqs.size(), p.uniform ? "few-term kernel" : "many-term kernel",
              (double)n_segs * vocab * kChamp * 4.0 / 1e6);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "--time") == 0) {
    const uint32_t log2_vocab = argc > 2 ? (uint32_t)std::atoi(argv[2]) : 21u;
    time_batch("1024 x 3 terms, 1 segment, k=11", log2_vocab, 1, 1024, 3, 11);
    time_batch("8192 x 5 terms, 2 segments, k=101", log2_vocab, 2, 8192, 5, 101);
    return 0;
  }
  cases_k_and_segments();
  cases_strategy_terms_weights_filters();
  cases_tuning();
  cases_score_plans();
  cases_threaded();
  cases_malformed();
  return 0;
}
