// nested_filter_sanitize.cpp — a stand-alone program for the sanitizers (tests/test_nested_filter_args.py builds it
// with -fsanitize=address,undefined together with csrc/slg_plan.cpp): hand-made and pseudo-random nested filter
// trees, valid and malformed, through check_nested_filter_trees and plan_nested_filter_trees against a described
// state.  Every array is exactly sized, so that a read outside one is an error the sanitizer sees.
// usage: nested_filter_sanitize n_random seed -> "trees=N ok=N invalid=N unsupported=N"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../searchlite_amd/csrc/slg_plan.hpp"

namespace {
uint64_t state = 1;
uint32_t rnd(uint32_t n) {  // splitmix64
  uint64_t z = (state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) % n);
}

struct Tree {
  std::vector<slg_nested_scope> scopes;
  std::vector<slg_filter_node> nodes;
  std::vector<uint32_t> ords;
  slg_nested_filter_tree view() const {
    return slg_nested_filter_tree{(uint32_t)scopes.size(), scopes.empty() ? nullptr : scopes.data(), (uint32_t)nodes.size(),
                                  nodes.empty() ? nullptr : nodes.data(), (uint32_t)ords.size(),
                                  ords.empty() ? nullptr : ords.data()};
  }
};

// a well-formed program of about n leaves over the fields of `path` (-1: the doc level) that names the scopes in
// `children`; wild: some of its numbers are replaced by arbitrary ones
void program(Tree &t, int32_t path, const std::vector<uint32_t> &children, bool wild) {
  const uint32_t begin = (uint32_t)t.nodes.size();
  uint32_t depth = 0;
  auto push = [&](slg_filter_node n) {
    if (wild && rnd(12) == 0) n.kind = (int32_t)rnd(12) - 2;
    if (wild && rnd(12) == 0) n.field = (int32_t)rnd(14) - 3;
    if (wild && rnd(12) == 0) n.arity = rnd(20);
    if (wild && rnd(20) == 0) n.ord_begin = rnd(2) ? 0xFFFFFFFFu : rnd(8);
    t.nodes.push_back(n);
  };
  for (const uint32_t c : children) {
    slg_filter_node n{};
    n.kind = SLG_FILTER_NESTED;
    n.field = (int32_t)c;
    push(n);
    depth++;
  }
  const uint32_t leaves = 1 + rnd(4);
  for (uint32_t i = 0; i < leaves; i++) {
    slg_filter_node n{};
    // a leaf that fits the described state (see main): the doc level's agg fields 0 keyword, 1 f64, 2 and 3 i64 (3
    // beyond 2^53: unsupported); under path p < 3 nested field p, of kind f64 / i64 / keyword; deeper: OR of nothing
    static const int32_t doc_kind[4] = {SLG_FILTER_KEYWORD_IN, SLG_FILTER_RANGE_F64, SLG_FILTER_RANGE_I64, SLG_FILTER_RANGE_I64};
    static const int32_t obj_kind[3] = {SLG_FILTER_RANGE_F64, SLG_FILTER_RANGE_I64, SLG_FILTER_KEYWORD_IN};
    if (path < 0) {
      n.field = (int32_t)(rnd(12) == 0 ? 3 : rnd(3));
      n.kind = doc_kind[n.field];
    } else if (path < 3) {
      n.field = path;
      n.kind = obj_kind[path];
    } else {
      n.kind = SLG_FILTER_OR;
    }
    n.lo_f = (double)rnd(5) - 2.0;
    n.hi_f = wild && rnd(9) == 0 ? std::nan("") : (double)rnd(5);
    n.lo_i = rnd(4) == 0 ? INT64_MIN : -(int64_t)rnd(9);
    n.hi_i = rnd(4) == 0 ? INT64_MAX : (int64_t)rnd(9);
    if (n.kind == SLG_FILTER_KEYWORD_IN) {
      n.ord_begin = (uint32_t)t.ords.size();
      n.n_ords_in = rnd(4);
      for (uint32_t j = 0; j < n.n_ords_in; j++) t.ords.push_back(rnd(wild && rnd(6) == 0 ? 40 : 5));
    }
    push(n);
    depth++;
    if (rnd(3) == 0) {
      slg_filter_node m{};
      m.kind = SLG_FILTER_NOT;
      push(m);
    }
  }
  slg_filter_node top{};
  top.kind = rnd(2) ? SLG_FILTER_AND : SLG_FILTER_OR;
  top.arity = depth;
  push(top);
  uint32_t n_nodes = (uint32_t)t.nodes.size() - begin, first = begin;
  if (wild && rnd(15) == 0) n_nodes += rnd(3);
  if (wild && rnd(15) == 0) first = rnd(2) ? 0xFFFFFFFFu : first + 1u;
  if (wild && rnd(25) == 0) n_nodes = 0;
  t.scopes.push_back(slg_nested_scope{wild && rnd(15) == 0 ? (int32_t)rnd(12) - 3 : path, first, n_nodes});
}

// object scopes of the paths 0 <- 1 <- 2 <- 3 <- 4 below one another, some side by side, then the doc level
Tree random_tree(bool wild) {
  Tree t;
  std::vector<uint32_t> top;
  const uint32_t chains = rnd(4);
  for (uint32_t c = 0; c < chains; c++) {
    const uint32_t depth = 1 + rnd(wild ? 6 : 4);
    std::vector<uint32_t> below;
    for (uint32_t level = depth; level-- > 0;) {
      program(t, (int32_t)level, below, wild);
      below.assign(1, (uint32_t)t.scopes.size() - 1u);
    }
    top.push_back(below[0]);
  }
  program(t, -1, top, wild);
  return t;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  const uint32_t n_random = (uint32_t)std::atoi(argv[1]);
  state = (uint64_t)std::atoll(argv[2]);
  const uint32_t n_segs = 2;
  // the described state: made-up addresses, never read
  const auto addr = [](uint32_t owner, uint32_t s, uint32_t tag) {
    return reinterpret_cast<const uint32_t *>((uintptr_t)(((uint64_t)(owner + 1) << 32) | ((uint64_t)s << 8) | tag));
  };
  std::vector<slgplan::FscoreFieldView> fields(4);
  for (uint32_t f = 0; f < 4; f++) {
    fields[f].id = (int32_t)f;
    fields[f].keyword = f == 0;
    fields[f].n_ords = 5;
    fields[f].from_i64 = f >= 2;
    fields[f].any_value = true;
    fields[f].vmax = f == 3 ? 1e17 : 9.0;
    for (uint32_t s = 0; s < n_segs; s++) fields[f].per_seg.push_back(slg::ColumnDev{addr(f, s, 2u), addr(f, s, 1u)});
  }
  std::vector<slgplan::NestedPathView> paths(6);
  for (uint32_t p = 0; p < 6; p++) {
    paths[p].id = (int32_t)p;
    paths[p].parent = p == 5 ? -1 : (int32_t)p - 1;
    for (uint32_t s = 0; s < n_segs; s++)
      paths[p].per_seg.push_back(p == 5 && s == 1 ? slg::NestedPathDev{}
                                                  : slg::NestedPathDev{addr(p, s, 4u), addr(p, s, 5u), nullptr, nullptr, 7u, 0u});
  }
  std::vector<slgplan::NestedFieldView> nfields(6);
  for (uint32_t f = 0; f < 6; f++) {
    nfields[f].id = (int32_t)f;
    nfields[f].path = (int32_t)(f % 3);
    nfields[f].kind = 1 + (int)(f % 3);
    nfields[f].n_ords = 5;
    for (uint32_t s = 0; s < n_segs; s++) {
      nfields[f].per_seg.push_back(slg::NestedColDev{addr(f, s, 8u), addr(f, s, 9u), addr(f, s, 10u)});
      nfields[f].has.push_back(f == 5 && s == 1 ? 0 : 1);
    }
  }
  const std::vector<char> live = {1, 0, 1};
  std::vector<const uint32_t *> reject(live.size() * n_segs, nullptr);
  for (size_t f = 0; f < live.size(); f++)
    for (uint32_t s = 0; s < n_segs && live[f]; s++) reject[f * n_segs + s] = addr((uint32_t)f, s, 3u);

  size_t n_trees = 0, ok = 0, invalid = 0, unsupported = 0;
  for (uint32_t round = 0; round < n_random; round++) {
    // one to three trees a call, now and then 65 of them; every other call holds wild numbers
    std::vector<Tree> trees(rnd(40) == 0 ? 65u : 1u + rnd(3));
    for (Tree &t : trees) t = random_tree(round % 2 == 1);
    std::vector<slg_nested_filter_tree> views;
    for (const Tree &t : trees) views.push_back(t.view());
    n_trees += trees.size();
    try {
      slgplan::check_nested_filter_trees(views.data(), (uint32_t)views.size());
      slgplan::NestedFilterPlan plan;
      slgplan::plan_nested_filter_trees(fields, reject.data(), live.data(), live.size(), paths, nfields, n_segs, views.data(),
                                        (uint32_t)views.size(), plan);
      // the image is consistent: every scope's nodes lie inside the node table, every NESTED row names an object scope
      const uint32_t n_obj = plan.level_begin.back();
      if (plan.scopes.size() != n_obj + views.size()) return 3;
      for (const slg::NestedScopeDev &sc : plan.scopes) {
        if ((size_t)sc.node_begin + sc.n_nodes > plan.nodes.size()) return 4;
        for (uint32_t i = 0; i < sc.n_nodes; i++) {
          const slg::FilterNodeDev &nd = plan.nodes[sc.node_begin + i];
          if (nd.kind == slg::kFilterNested && nd.row >= n_obj) return 5;
          if (nd.kind == slg::kFilterKeywordIn && nd.bits >= plan.words.size()) return 6;
        }
      }
      ok++;
    } catch (const slgplan::SlgError &e) {
      if (e.code == SLG_ERR_INVALID) invalid++;
      else if (e.code == SLG_ERR_UNSUPPORTED) unsupported++;
      else return 7;
    }
  }
  // NULL arrays, alone
  const slg_nested_filter_tree none{};
  for (const slg_nested_filter_tree *p : {(const slg_nested_filter_tree *)nullptr, &none}) {
    try {
      slgplan::check_nested_filter_trees(p, 1);
      return 8;
    } catch (const slgplan::SlgError &e) {
      if (e.code != SLG_ERR_INVALID) return 9;
    }
  }
  std::printf("trees=%zu ok=%zu invalid=%zu unsupported=%zu\n", n_trees, ok, invalid, unsupported);
  return 0;
}
