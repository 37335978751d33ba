// slg_date.hpp — the bucket of a date_histogram node (query/aggs/mod.rs bucket_start, :3391-3401, and
// truncate_calendar, :3410-3429): value -> dense bucket id, the same arithmetic in the planner (the row range
// of a node's table, slg_aggs.hip) and in the kernels (agg_buckets, slg_aggs.hpp).  slgp_date_buckets
// (slg_plan_capi.cpp) sweeps it on the CPU.
//   fixed     id = ceil((val - offset) as f64 / step as f64): ONE IEEE f64 division of the two converted
//             operands, then ceil — a value on a boundary is its own bucket, any other goes to the next
//             boundary; the rounded quotient is the reference's, so no integer division, no reciprocal.
//             key = id * step + offset.
//   calendar  t = val - offset lies in a UTC proleptic-Gregorian day / ISO week (from Monday) / month / quarter /
//             year; id = that unit's index since 1970 (floor semantics: t = -1 is 1969-12-31), key = the
//             unit's start in ms + offset.  Plain integer arithmetic with floor division; the civil date is
//             the usual days-to-civil algorithm (era of 146 097 days, day of era, year of era,
//             mp = (5 * doy + 2) / 153).
// The planner keeps every operand within +-2^53 (fixed) and t within 0001-01-01 .. 9999-12-31 (calendar), where
// `as i64`, `as f64` and val - offset are exact and nothing overflows.
#pragma once

#include <math.h>
#include <stdint.h>

#include "slg_desc.hpp"

namespace slg {

constexpr uint32_t kDateFixed = 0, kDateDay = 1, kDateWeek = 2, kDateMonth = 3, kDateQuarter = 4, kDateYear = 5;
constexpr long long kDateDayMs = 86400000ll;
constexpr long long kDateMinMs = -62135596800000ll;  // 0001-01-01T00:00:00Z
constexpr long long kDateMaxMs = 253402300799999ll;  // 9999-12-31T23:59:59.999Z

SLG_HD inline long long date_floor_div(const long long a, const long long b) {  // b > 0
  const long long q = a / b;
  return q - ((a % b) < 0 ? 1 : 0);
}

// days since 1970-01-01 -> the civil date
SLG_HD inline void date_civil(const long long days, long long &y, uint32_t &m, uint32_t &d) {
  const long long z = days + 719468;  // days since 0000-03-01
  const long long era = date_floor_div(z, 146097);
  const uint32_t doe = (uint32_t)(z - era * 146097);                               // [0, 146096]
  const uint32_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;      // [0, 399]
  const uint32_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);                    // [0, 365], from 1 March
  const uint32_t mp = (5 * doy + 2) / 153;                                         // [0, 11], from March
  d = doy - (153 * mp + 2) / 5 + 1;
  m = mp < 10 ? mp + 3 : mp - 9;
  y = (long long)yoe + era * 400 + (m <= 2 ? 1 : 0);
}

SLG_HD inline long long date_bucket_id(const uint32_t unit, const long long step, const long long offset,
                                       const long long val) {
  const long long t = val - offset;
  if (unit == kDateFixed) return (long long)ceil((double)t / (double)step);
  const long long day = date_floor_div(t, kDateDayMs);
  if (unit == kDateDay) return day;
  if (unit == kDateWeek) return date_floor_div(day + 3, 7);  // (1970-01-01 was a Thursday: Monday is day 7 w - 3)
  long long y;
  uint32_t m, d;
  date_civil(day, y, m, d);
  if (unit == kDateYear) return y - 1970;
  const long long month = (y - 1970) * 12 + ((long long)m - 1);
  return unit == kDateMonth ? month : date_floor_div(month, 3);
}

}  // namespace slg
