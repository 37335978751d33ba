// slg_explain_host.hpp — the argument checks of slg_batch_explain (searchlite_gpu.h): plain C++ over the facts of a
// batch, so that the entry point (slg_explain.hip) and the CPU unit tests (slg_explain_capi.cpp in
// lib/libslg_plan.so, tests/test_explain_args.py) run the same code.  Every check comes before any device work.
#pragma once

#include <string>

#include "../../include/searchlite_gpu.h"
#include "slg_desc.hpp"
#include "slg_plan.hpp"

namespace slgexplain {

using slgplan::SlgError;

// what the checks read of a batch
struct BatchFacts {
  bool null_batch = false;
  bool detached = false;  // its index was destroyed
  bool launched = false;
  bool scan = false, hybrid = false, nested = false, deep = false, rescore = false;
  bool last_sharded = false;  // the batch's last run was slg_batch_run_sharded*
  uint32_t max_table = 0;     // the most term rows (all segments) of one query
};

// SLG_ERR_INVALID first, in the header's order; SLG_ERR_UNSUPPORTED (CPU scorer) behind every invalid argument
inline void check(const BatchFacts &b, uint32_t rows, const slg_explain_out *out) {
  auto invalid = [](bool ok, const char *msg) {
    if (!ok) throw SlgError(SLG_ERR_INVALID, std::string("explain: ") + msg);
  };
  auto unsupported = [](bool ok, const std::string &msg) {
    if (!ok) throw SlgError(SLG_ERR_UNSUPPORTED, "explain: " + msg + " (CPU scorer)");
  };
  invalid(!b.null_batch && !b.detached, "batch is NULL or its index was destroyed");
  invalid(out != nullptr, "out is NULL");
  invalid(rows != 0u, "rows is 0");
  invalid(out->base_score && out->final_score && out->n_functions, "base_score, final_score or n_functions is NULL");
  invalid(out->fn_type && out->fn_field && out->fn_value, "fn_type, fn_field or fn_value is NULL");
  invalid(!b.rescore || (out->rescored && out->rescore_score && out->combined_score),
          "a rescore batch needs rescored, rescore_score and combined_score");
  invalid(b.launched, "the batch has not run");
  unsupported(rows <= SLG_MAX_EXPLAIN_ROWS, "rows " + std::to_string(rows) + " is above SLG_MAX_EXPLAIN_ROWS");
  unsupported(!b.scan, "a scan batch is not explained");
  unsupported(!b.hybrid, "a hybrid batch is not explained");
  unsupported(!b.nested && !b.deep, "a batch with a two-level or deeper score plan is not explained");
  unsupported(b.max_table <= slg::kRescoreMaxTable,
              "a query has " + std::to_string(b.max_table) + " term rows over its segments, above the table of " +
                  std::to_string(slg::kRescoreMaxTable));
  unsupported(!b.last_sharded, "the batch's last run was sharded: its rows are the merged ones of every rank");
}

}  // namespace slgexplain
