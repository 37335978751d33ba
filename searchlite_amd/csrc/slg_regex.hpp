// slg_regex.hpp — the host compiler of a regex request of slg_expand_batch (slg_regex.cpp): pattern -> a minimised
// byte-level DFA in the form the device walks (slg_expand_regex.hpp), and the reference's literal-prefix rule.
// Pure host C++17, no HIP header: linked into libsearchlite_gpu.so and, behind the test C ABI of
// slg_expand_capi.cpp, into lib/libslg_plan.so.
//
// The pipeline: parse (the language of include/searchlite_gpu.h, "REGEX"; anything outside it is refused, never
// approximated) -> Thompson NFA over bytes (code-point ranges split into UTF-8 byte-range sequences; terms are
// valid UTF-8, so only the language on valid UTF-8 matters) -> subset construction -> Moore minimisation -> byte
// classes (bytes whose columns are equal share one).  The match is of the WHOLE term (^(?:pattern)$,
// util/regex.rs): the DFA starts at the term's first byte and its state after the last byte decides.
// Assertions: a start-assertion edge (^ \A) is followed only in the closure of the initial state, an end-assertion
// edge ($ \z) only when acceptance at the end of the input is decided; so `a^b` is the empty language and
// `a$|b` is {a, b}.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/searchlite_gpu.h"
#include "slg_plan.hpp"  // SlgError

namespace slgregex {

using slgplan::SlgError;

// state 0 is dead (every transition of it leads to it, it does not accept), state 1 is the start
struct Dfa {
  uint32_t n_states = 0, n_classes = 0;
  uint8_t class_of[256] = {};
  std::vector<uint8_t> table;   // [n_states x n_classes], state-major: table[state * n_classes + class]
  std::vector<uint8_t> accept;  // [32]: bit s of the 256-bit set = state s accepts
};

// Throws SLG_ERR_INVALID (the reference's regex compiler refuses the pattern too) or SLG_ERR_UNSUPPORTED (outside
// the supported language, or a minimised DFA above SLG_MAX_REGEX_STATES / SLG_MAX_REGEX_TABLE); the message names
// the construct and its byte offset in the pattern.  cps: the pattern's code points
Dfa compile(const std::vector<uint32_t> &cps);

// regex_literal_prefix (api/reader.rs:1285-1320) on the pattern's text -> the prefix's code points
std::vector<uint32_t> literal_prefix(const std::vector<uint32_t> &cps);

void utf8_append(std::string &out, uint32_t cp);

}  // namespace slgregex
