// slg_explain_capi.cpp — a small C ABI over the argument checks of slg_batch_explain (slg_explain_host.hpp) for the
// CPU unit tests (tests/test_explain_args.py): the checks against hand-made batch facts.  Built into
// lib/libslg_plan.so with g++; NOT part of libsearchlite_gpu.so's exported surface.
#include <cstring>

#include "slg_explain_host.hpp"

extern "C" {

// flags: bit 0 a NULL batch, 1 detached, 2 launched, 3 scan, 4 hybrid, 5 nested, 6 deep, 7 rescore, 8 last run sharded
int slgx_explain_check(uint32_t flags, uint32_t max_table, uint32_t rows, const slg_explain_out *out, char *err, uint32_t err_len) {
  slgexplain::BatchFacts f;
  f.null_batch = flags & 1u;
  f.detached = flags & 2u;
  f.launched = flags & 4u;
  f.scan = flags & 8u;
  f.hybrid = flags & 16u;
  f.nested = flags & 32u;
  f.deep = flags & 64u;
  f.rescore = flags & 128u;
  f.last_sharded = flags & 256u;
  f.max_table = max_table;
  try {
    slgexplain::check(f, rows, out);
    return SLG_OK;
  } catch (const slgexplain::SlgError &e) {
    if (err && err_len) {
      std::strncpy(err, e.what(), err_len - 1);
      err[err_len - 1] = 0;
    }
    return e.code;
  }
}

}  // extern "C"
