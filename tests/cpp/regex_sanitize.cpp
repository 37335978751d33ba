// regex_sanitize.cpp — a stand-alone program for the sanitizers (tests/test_regex_ref.py builds it with
// -fsanitize=address,undefined together with csrc/slg_regex.cpp): every pattern of a listing through the regex
// compiler, every pattern that compiles through the host build of the device's DFA walk over every term of a second
// listing, and the literal-prefix rule.  Both listings hold one hex-encoded UTF-8 string per line.
// usage: regex_sanitize patterns.hex terms.hex -> "patterns=N compiled=N invalid=N unsupported=N matches=N"
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../../searchlite_amd/csrc/slg_expand_regex.hpp"
#include "../../searchlite_amd/csrc/slg_regex.hpp"

static std::vector<std::string> read_hex(const char *path) {
  std::ifstream in(path);
  std::vector<std::string> out;
  std::string line;
  while (std::getline(in, line)) {
    std::string s;
    for (size_t i = 0; i + 1 < line.size(); i += 2) s.push_back((char)std::stoi(line.substr(i, 2), nullptr, 16));
    out.push_back(s);
  }
  return out;
}

// (the listings are valid UTF-8: the test wrote them)
static std::vector<uint32_t> code_points(const std::string &s) {
  std::vector<uint32_t> cps;
  const unsigned char *p = reinterpret_cast<const unsigned char *>(s.data());
  for (size_t i = 0; i < s.size();) {
    uint32_t len;
    cps.push_back(slg::utf8_next(p + i, len));
    i += len;
  }
  return cps;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  const std::vector<std::string> patterns = read_hex(argv[1]), terms = read_hex(argv[2]);
  size_t compiled = 0, invalid = 0, unsupported = 0, matches = 0, prefix_chars = 0;
  for (const std::string &pat : patterns) {
    const std::vector<uint32_t> cps = code_points(pat);
    prefix_chars += slgregex::literal_prefix(cps).size();
    try {
      const slgregex::Dfa d = slgregex::compile(cps);
      if (d.table.size() != (size_t)d.n_states * d.n_classes || d.accept.size() != slg::kRegexAcceptBytes) return 3;
      compiled++;
      // the table through an exactly sized copy, so that a step outside it is an error the sanitizer sees
      const std::vector<uint8_t> table(d.table.begin(), d.table.end());
      for (const std::string &t : terms)
        matches += slg::regex_walk(d.class_of, table.data(), d.accept.data(), d.n_classes,
                                   reinterpret_cast<const unsigned char *>(t.data()), (uint32_t)t.size());
    } catch (const slgregex::SlgError &e) {
      if (e.code == SLG_ERR_INVALID) invalid++;
      else if (e.code == SLG_ERR_UNSUPPORTED) unsupported++;
      else return 4;
    }
  }
  std::printf("patterns=%zu compiled=%zu invalid=%zu unsupported=%zu matches=%zu prefix_chars=%zu\n", patterns.size(),
              compiled, invalid, unsupported, matches, prefix_chars);
  return 0;
}
