// slg_regex.cpp — see slg_regex.hpp.  Pure host code: no HIP header, builds with g++.
#include "slg_regex.hpp"

#include <algorithm>
#include <map>

namespace slgregex {

void utf8_append(std::string &out, uint32_t cp) {
  if (cp < 0x80u) {
    out.push_back((char)cp);
  } else if (cp < 0x800u) {
    out.push_back((char)(0xC0u | (cp >> 6)));
    out.push_back((char)(0x80u | (cp & 0x3Fu)));
  } else if (cp < 0x10000u) {
    out.push_back((char)(0xE0u | (cp >> 12)));
    out.push_back((char)(0x80u | ((cp >> 6) & 0x3Fu)));
    out.push_back((char)(0x80u | (cp & 0x3Fu)));
  } else {
    out.push_back((char)(0xF0u | (cp >> 18)));
    out.push_back((char)(0x80u | ((cp >> 12) & 0x3Fu)));
    out.push_back((char)(0x80u | ((cp >> 6) & 0x3Fu)));
    out.push_back((char)(0x80u | (cp & 0x3Fu)));
  }
}

std::vector<uint32_t> literal_prefix(const std::vector<uint32_t> &cps) {
  std::vector<uint32_t> prefix;
  bool escaped = false;                                  // :1287
  for (const uint32_t ch : cps) {                        // :1288
    if (escaped) {
      if (ch == 'd' || ch == 'D' || ch == 'w' || ch == 'W' || ch == 's' || ch == 'S' || ch == 'b' || ch == 'B' ||
          ch == 'p' || ch == 'P')                        // :1299-1300
        break;
      prefix.push_back(ch);                              // :1291-1297, :1301-1306: the char as itself
      escaped = false;
      continue;
    }
    if (ch == '\\') {                                    // :1310
      escaped = true;
    } else if (ch == '^' && prefix.empty()) {            // :1311
      continue;
    } else if (ch == '.' || ch == '*' || ch == '+' || ch == '?' || ch == '(' || ch == ')' || ch == '[' || ch == ']' ||
               ch == '{' || ch == '}' || ch == '|' || ch == '$') {   // :1312
      break;
    } else {
      prefix.push_back(ch);                              // :1313-1316
    }
  }
  return prefix;
}

namespace {

constexpr uint32_t kInf = 0xFFFFFFFFu;
constexpr uint32_t kMaxRepeat = 1000;       // a count above it is refused before anything is built
constexpr uint32_t kMaxDepth = 32;          // nested groups
constexpr size_t kMaxNfaStates = 200000;
constexpr size_t kMaxRawDfaStates = 8192;   // subset construction, before minimisation

struct Range {
  uint32_t lo, hi;
};
enum class Op { Empty, Set, Cat, Alt, Repeat, Start, End };
struct Node {
  Op op = Op::Empty;
  std::vector<Range> set;
  std::vector<int> kids;
  uint32_t min = 0, max = 0;
};

std::string show(uint32_t cp) {
  std::string s;
  utf8_append(s, cp);
  return s;
}

bool is_ascii_alnum(uint32_t c) { return (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); }
bool is_ascii_punct(uint32_t c) { return c > 0x20u && c < 0x7Fu && !is_ascii_alnum(c); }

void normalise(std::vector<Range> &set) {
  std::sort(set.begin(), set.end(), [](const Range &a, const Range &b) { return a.lo < b.lo; });
  std::vector<Range> out;
  for (const Range &r : set) {
    if (!out.empty() && r.lo <= out.back().hi + 1u) out.back().hi = std::max(out.back().hi, r.hi);
    else out.push_back(r);
  }
  set.swap(out);
}

std::vector<Range> complement(const std::vector<Range> &set) {  // (normalised) within all scalar values
  std::vector<Range> out;
  uint32_t next = 0;
  for (const Range &r : set) {
    if (r.lo > next) out.push_back(Range{next, r.lo - 1});
    next = r.hi + 1;
  }
  if (next <= 0x10FFFFu) out.push_back(Range{next, 0x10FFFFu});
  return out;
}

struct Parser {
  const std::vector<uint32_t> &p;
  size_t i = 0;
  std::vector<size_t> byte_at;  // byte offset of code point i of the pattern
  std::vector<Node> nodes;
  std::vector<std::vector<uint32_t>> names;
  uint32_t depth = 0;

  explicit Parser(const std::vector<uint32_t> &cps) : p(cps) {
    size_t b = 0;
    for (const uint32_t c : cps) {
      byte_at.push_back(b);
      b += c < 0x80u ? 1 : c < 0x800u ? 2 : c < 0x10000u ? 3 : 4;
    }
    byte_at.push_back(b);
  }
  [[noreturn]] void fail(int code, const std::string &what, size_t at) const {
    throw SlgError(code, "regex: " + what + " at byte " + std::to_string(byte_at[std::min(at, p.size())]) +
                             (code == SLG_ERR_UNSUPPORTED ? " is not supported: CPU path" : ""));
  }
  bool more() const { return i < p.size(); }
  int add(Node n) {
    nodes.push_back(std::move(n));
    return (int)nodes.size() - 1;
  }
  int literal(uint32_t c) {
    Node n;
    n.op = Op::Set;
    n.set.push_back(Range{c, c});
    return add(std::move(n));
  }

  int parse() {
    const int top = parse_alt();
    if (more()) fail(SLG_ERR_INVALID, "unbalanced ')'", i);
    return top;
  }
  int parse_alt() {
    std::vector<int> alts{parse_cat()};
    while (more() && p[i] == '|') {
      i++;
      alts.push_back(parse_cat());
    }
    if (alts.size() == 1) return alts[0];
    Node n;
    n.op = Op::Alt;
    n.kids = std::move(alts);
    return add(std::move(n));
  }
  static bool quant_start(uint32_t c) { return c == '*' || c == '+' || c == '?' || c == '{'; }
  int parse_cat() {
    Node cat;
    cat.op = Op::Cat;
    while (more() && p[i] != '|' && p[i] != ')') {
      if (quant_start(p[i]))  // (after an atom its quantifier is taken at once: this one follows nothing, '(' or '|')
        fail(SLG_ERR_INVALID, "a quantifier '" + show(p[i]) + "' with nothing to repeat", i);
      const bool group = p[i] == '(';
      int atom = parse_atom();
      if (more() && quant_start(p[i])) {
        // (the regex crate repeats an assertion, other engines refuse to: refused here, a group around it is not)
        if (!group && (nodes[(size_t)atom].op == Op::Start || nodes[(size_t)atom].op == Op::End))
          fail(SLG_ERR_UNSUPPORTED, "a quantifier applied to an anchor", i);
        atom = parse_quant(atom);
        if (more() && p[i] == '?') i++;  // lazy: no meaning for a whole-term match
        if (more() && quant_start(p[i])) fail(SLG_ERR_UNSUPPORTED, "a quantifier applied to a quantifier", i);
      }
      cat.kids.push_back(atom);
    }
    if (cat.kids.size() == 1) return cat.kids[0];
    if (cat.kids.empty()) cat.op = Op::Empty;
    return add(std::move(cat));
  }
  bool digits(uint32_t &v) {  // at least one
    if (!more() || p[i] < '0' || p[i] > '9') return false;
    v = 0;
    while (more() && p[i] >= '0' && p[i] <= '9') {
      v = std::min<uint32_t>(v * 10u + (p[i] - '0'), 1000000u);
      i++;
    }
    return true;
  }
  int parse_quant(int atom) {
    Node n;
    n.op = Op::Repeat;
    n.kids.push_back(atom);
    const size_t at = i;
    const uint32_t q = p[i++];
    if (q == '*') {
      n.min = 0, n.max = kInf;
    } else if (q == '+') {
      n.min = 1, n.max = kInf;
    } else if (q == '?') {
      n.min = 0, n.max = 1;
    } else {
      const std::string bad = "a '{' that does not complete to {n}, {n,} or {n,m}";
      uint32_t lo = 0, hi = 0;
      if (more() && p[i] == ',') {
        i++;
        if (digits(hi) && more() && p[i] == '}') fail(SLG_ERR_UNSUPPORTED, "the counted repetition {,m}", at);
        fail(SLG_ERR_INVALID, bad, at);
      }
      if (!digits(lo)) fail(SLG_ERR_INVALID, bad, at);
      if (more() && p[i] == '}') {
        hi = lo;
      } else if (more() && p[i] == ',') {
        i++;
        if (more() && p[i] == '}') hi = kInf;
        else if (!digits(hi) || !more() || p[i] != '}') fail(SLG_ERR_INVALID, bad, at);
      } else {
        fail(SLG_ERR_INVALID, bad, at);
      }
      i++;  // '}'
      if (hi != kInf && lo > hi) fail(SLG_ERR_INVALID, "a counted repetition {n,m} with n > m", at);
      if (lo > kMaxRepeat || (hi != kInf && hi > kMaxRepeat))
        fail(SLG_ERR_UNSUPPORTED, "a repetition count above " + std::to_string(kMaxRepeat) + " (its DFA is above SLG_MAX_REGEX_STATES)", at);
      n.min = lo, n.max = hi;
    }
    return add(std::move(n));
  }
  // the char after a '\' at i - 1, as a literal; anything else is refused.  in_class: no anchors
  uint32_t escape_literal(bool &is_start, bool &is_end, bool in_class) {
    const size_t at = i - 1;
    if (!more()) fail(SLG_ERR_INVALID, "a trailing lone '\\'", at);
    const uint32_t e = p[i++];
    is_start = is_end = false;
    if (e == 'n') return 0x0Au;
    if (e == 't') return 0x09u;
    if (e == 'r') return 0x0Du;
    if (!in_class && e == 'A') {
      is_start = true;
      return 0;
    }
    if (!in_class && e == 'z') {
      is_end = true;
      return 0;
    }
    if (e == 'd' || e == 'D' || e == 'w' || e == 'W' || e == 's' || e == 'S' || e == 'p' || e == 'P' || e == 'b' || e == 'B')
      fail(SLG_ERR_UNSUPPORTED, "the escape \\" + show(e) + " (Unicode classes and word boundaries follow the regex crate's Unicode tables)", at);
    if (is_ascii_punct(e) && e != '<' && e != '>') return e;
    fail(SLG_ERR_UNSUPPORTED, "the escape \\" + show(e), at);
  }
  int parse_atom() {
    const size_t at = i;
    const uint32_t c = p[i++];
    Node n;
    if (c == '(') {
      if (++depth > kMaxDepth) fail(SLG_ERR_UNSUPPORTED, "groups nested deeper than " + std::to_string(kMaxDepth), at);
      if (more() && p[i] == '?') {
        i++;
        if (more() && p[i] == ':') {
          i++;
        } else if (more() && (p[i] == '<' || (p[i] == 'P' && i + 1 < p.size() && p[i + 1] == '<'))) {
          i += p[i] == 'P' ? 2 : 1;
          std::vector<uint32_t> name;
          while (more() && p[i] != '>') name.push_back(p[i++]);
          if (!more()) fail(SLG_ERR_INVALID, "an unclosed group name", at);
          i++;
          if (name.empty()) fail(SLG_ERR_INVALID, "an empty group name", at);
          for (size_t k = 0; k < name.size(); k++)
            if (!(name[k] == '_' || (is_ascii_alnum(name[k]) && (k > 0 || name[k] > '9'))))
              fail(SLG_ERR_UNSUPPORTED, "a group name outside [A-Za-z_][A-Za-z0-9_]* (or a look-around)", at);
          if (std::find(names.begin(), names.end(), name) != names.end()) fail(SLG_ERR_INVALID, "a duplicate group name", at);
          names.push_back(name);
        } else {
          if (!more()) fail(SLG_ERR_INVALID, "unbalanced '('", at);
          fail(SLG_ERR_UNSUPPORTED, "a flag group '(?" + show(p[i]) + "'", at);
        }
      }
      const int inner = parse_alt();
      if (!more()) fail(SLG_ERR_INVALID, "unbalanced '('", at);
      i++;  // ')'
      depth--;
      return inner;
    }
    if (c == '[') return parse_class(at);
    if (c == '.') {
      n.op = Op::Set;
      n.set = {Range{0, 0x09u}, Range{0x0Bu, 0x10FFFFu}};
      return add(std::move(n));
    }
    if (c == '^' || c == '$') {
      n.op = c == '^' ? Op::Start : Op::End;
      return add(std::move(n));
    }
    if (c == '\\') {
      bool is_start, is_end;
      const uint32_t lit = escape_literal(is_start, is_end, false);
      if (is_start || is_end) {
        n.op = is_start ? Op::Start : Op::End;
        return add(std::move(n));
      }
      return literal(lit);
    }
    return literal(c);  // (']' and '}' alone are literals, as in the regex crate)
  }
  uint32_t class_prim() {
    const uint32_t c = p[i++];
    if (c != '\\') return c;
    bool a, b;
    return escape_literal(a, b, true);
  }
  int parse_class(size_t at) {
    Node n;
    n.op = Op::Set;
    bool negate = false;
    if (more() && p[i] == '^') {
      negate = true;
      i++;
    }
    if (more() && p[i] == ']') {  // a leading ']' is a literal
      n.set.push_back(Range{']', ']'});
      i++;
      // (the regex crate takes a '-' here as a literal, other engines as a range from ']': refused)
      if (i + 1 < p.size() && p[i] == '-' && p[i + 1] != ']') fail(SLG_ERR_UNSUPPORTED, "a '-' after a leading ']' in a class", i);
    }
    for (;;) {
      if (!more()) fail(SLG_ERR_INVALID, "an unclosed '['", at);
      const uint32_t c = p[i];
      if (c == ']') {
        i++;
        break;
      }
      if (c == '[') fail(SLG_ERR_UNSUPPORTED, "a '[' inside a class (nested classes, [:alpha:])", i);
      if ((c == '&' || c == '-' || c == '~') && i + 1 < p.size() && p[i + 1] == c)
        fail(SLG_ERR_UNSUPPORTED, "'" + show(c) + show(c) + "' inside a class (set operations)", i);
      const size_t item_at = i;
      const uint32_t lo = class_prim();
      if (i + 1 < p.size() && p[i] == '-' && p[i + 1] != ']') {
        if (p[i + 1] == '-') fail(SLG_ERR_UNSUPPORTED, "'--' inside a class (set operations)", i);
        i++;
        if (p[i] == '[') fail(SLG_ERR_UNSUPPORTED, "a '[' inside a class (nested classes, [:alpha:])", i);
        const uint32_t hi = class_prim();
        if (lo > hi) fail(SLG_ERR_INVALID, "a reversed range in a class", item_at);
        n.set.push_back(Range{lo, hi});
      } else {
        n.set.push_back(Range{lo, lo});
      }
    }
    normalise(n.set);
    if (negate) n.set = complement(n.set);  // over all scalar values, U+000A included
    return add(std::move(n));
  }
};

// ---- the NFA over bytes -------------------------------------------------------------------------------------
enum : uint8_t { kEps = 0, kByte = 1, kAtStart = 2, kAtEnd = 3 };
struct Edge {
  uint8_t kind, lo, hi;
  uint32_t to;
};
struct Frag {
  uint32_t s, e;
};

struct Nfa {
  std::vector<std::vector<Edge>> st;
  uint32_t state() {
    if (st.size() >= kMaxNfaStates)
      throw SlgError(SLG_ERR_UNSUPPORTED, "regex: the pattern's automaton is too large (its DFA is above SLG_MAX_REGEX_STATES): CPU path");
    st.emplace_back();
    return (uint32_t)st.size() - 1;
  }
  void edge(uint32_t from, uint8_t kind, uint32_t to, uint8_t lo = 0, uint8_t hi = 0) { st[from].push_back(Edge{kind, lo, hi, to}); }

  // one sequence of byte ranges s -> e
  void byte_seq(uint32_t s, uint32_t e, const uint8_t *lo, const uint8_t *hi, int n) {
    uint32_t cur = s;
    for (int k = 0; k < n; k++) {
      const uint32_t nxt = k == n - 1 ? e : state();
      edge(cur, kByte, nxt, lo[k], hi[k]);
      cur = nxt;
    }
  }
  static int encode(uint32_t cp, uint8_t *b) {
    if (cp < 0x80u) {
      b[0] = (uint8_t)cp;
      return 1;
    }
    if (cp < 0x800u) {
      b[0] = (uint8_t)(0xC0u | (cp >> 6)), b[1] = (uint8_t)(0x80u | (cp & 0x3Fu));
      return 2;
    }
    if (cp < 0x10000u) {
      b[0] = (uint8_t)(0xE0u | (cp >> 12)), b[1] = (uint8_t)(0x80u | ((cp >> 6) & 0x3Fu)), b[2] = (uint8_t)(0x80u | (cp & 0x3Fu));
      return 3;
    }
    b[0] = (uint8_t)(0xF0u | (cp >> 18)), b[1] = (uint8_t)(0x80u | ((cp >> 12) & 0x3Fu));
    b[2] = (uint8_t)(0x80u | ((cp >> 6) & 0x3Fu)), b[3] = (uint8_t)(0x80u | (cp & 0x3Fu));
    return 4;
  }
  // the scalar values lo .. hi as sequences of byte ranges: split at the surrogates, at the encoded lengths, and
  // until every continuation position is either one value or the full 0x80 .. 0xBF
  void scalar_range(uint32_t s, uint32_t e, uint32_t lo, uint32_t hi) {
    if (lo > hi) return;
    if (lo <= 0xDFFFu && hi >= 0xD800u) {
      if (lo < 0xD800u) scalar_range(s, e, lo, 0xD7FFu);
      if (hi > 0xDFFFu) scalar_range(s, e, 0xE000u, hi);
      return;
    }
    for (const uint32_t max : {0x7Fu, 0x7FFu, 0xFFFFu})
      if (lo <= max && hi > max) {
        scalar_range(s, e, lo, max);
        scalar_range(s, e, max + 1, hi);
        return;
      }
    if (hi >= 0x80u)
      for (int k = 1; k < 4; k++) {
        const uint32_t m = (1u << (6 * k)) - 1u;
        if ((lo & ~m) != (hi & ~m)) {
          if ((lo & m) != 0u) {
            scalar_range(s, e, lo, lo | m);
            scalar_range(s, e, (lo | m) + 1u, hi);
            return;
          }
          if ((hi & m) != m) {
            scalar_range(s, e, lo, (hi & ~m) - 1u);
            scalar_range(s, e, hi & ~m, hi);
            return;
          }
        }
      }
    uint8_t a[4], b[4];
    const int n = encode(lo, a);
    encode(hi, b);
    byte_seq(s, e, a, b, n);
  }

  Frag build(const std::vector<Node> &nodes, int id) {
    const Node &n = nodes[(size_t)id];
    Frag f{state(), state()};
    switch (n.op) {
      case Op::Empty:
        edge(f.s, kEps, f.e);
        break;
      case Op::Start:
        edge(f.s, kAtStart, f.e);
        break;
      case Op::End:
        edge(f.s, kAtEnd, f.e);
        break;
      case Op::Set:
        for (const Range &r : n.set) scalar_range(f.s, f.e, r.lo, r.hi);
        break;
      case Op::Cat: {
        uint32_t cur = f.s;
        for (const int k : n.kids) {
          const Frag g = build(nodes, k);
          edge(cur, kEps, g.s);
          cur = g.e;
        }
        edge(cur, kEps, f.e);
        break;
      }
      case Op::Alt:
        for (const int k : n.kids) {
          const Frag g = build(nodes, k);
          edge(f.s, kEps, g.s);
          edge(g.e, kEps, f.e);
        }
        break;
      case Op::Repeat: {
        uint32_t cur = f.s;
        for (uint32_t k = 0; k < n.min; k++) {
          const Frag g = build(nodes, n.kids[0]);
          edge(cur, kEps, g.s);
          cur = g.e;
        }
        if (n.max == kInf) {
          const Frag g = build(nodes, n.kids[0]);
          const uint32_t loop = state();
          edge(cur, kEps, loop);
          edge(loop, kEps, g.s);
          edge(g.e, kEps, loop);
          cur = loop;
        } else {
          for (uint32_t k = n.min; k < n.max; k++) {
            edge(cur, kEps, f.e);
            const Frag g = build(nodes, n.kids[0]);
            edge(cur, kEps, g.s);
            cur = g.e;
          }
        }
        edge(cur, kEps, f.e);
        break;
      }
    }
    return f;
  }

  // the states reachable from `set` over empty edges, and over the assertions that hold here
  std::vector<uint32_t> closure(std::vector<uint32_t> set, bool at_start, bool at_end, std::vector<uint8_t> &mark) const {
    std::vector<uint32_t> stack = set;
    for (const uint32_t s : set) mark[s] = 1;
    while (!stack.empty()) {
      const uint32_t s = stack.back();
      stack.pop_back();
      for (const Edge &e : st[s]) {
        if (e.kind == kByte || (e.kind == kAtStart && !at_start) || (e.kind == kAtEnd && !at_end)) continue;
        if (!mark[e.to]) {
          mark[e.to] = 1;
          set.push_back(e.to);
          stack.push_back(e.to);
        }
      }
    }
    for (const uint32_t s : set) mark[s] = 0;
    std::sort(set.begin(), set.end());
    return set;
  }
};

}  // namespace

Dfa compile(const std::vector<uint32_t> &cps) {
  Parser ps(cps);
  const int top = ps.parse();
  Nfa nfa;
  const Frag whole = nfa.build(ps.nodes, top);
  const size_t nn = nfa.st.size();
  std::vector<uint8_t> mark(nn, 0);

  // provisional byte classes: the intervals between the boundaries of every byte edge
  bool cut[257] = {};
  cut[0] = true;
  for (const auto &edges : nfa.st)
    for (const Edge &e : edges)
      if (e.kind == kByte) cut[e.lo] = cut[(size_t)e.hi + 1] = true;
  uint8_t pre_of[256];
  std::vector<uint8_t> rep;  // a byte of each provisional class
  for (uint32_t b = 0; b < 256; b++) {
    if (cut[b]) rep.push_back((uint8_t)b);
    pre_of[b] = (uint8_t)(rep.size() - 1);
  }
  const size_t npre = rep.size();

  // subset construction.  State 0: the empty set (dead).  State 1: the initial closure, the only one in which the
  // start assertions hold; it is never looked up again (an equal set reached later is past the start)
  std::vector<std::vector<uint32_t>> sets{{}, nfa.closure({whole.s}, true, false, mark)};
  std::map<std::vector<uint32_t>, uint32_t> ids;
  std::vector<std::vector<uint32_t>> trans{std::vector<uint32_t>(npre, 0u)};
  for (size_t s = 1; s < sets.size(); s++) {
    trans.emplace_back(npre, 0u);
    for (size_t c = 0; c < npre; c++) {
      const uint8_t b = rep[c];
      std::vector<uint32_t> move;
      for (const uint32_t q : sets[s])
        for (const Edge &e : nfa.st[q])
          if (e.kind == kByte && e.lo <= b && b <= e.hi && !mark[e.to]) {
            mark[e.to] = 1;
            move.push_back(e.to);
          }
      for (const uint32_t q : move) mark[q] = 0;
      if (move.empty()) continue;
      std::vector<uint32_t> next = nfa.closure(std::move(move), false, false, mark);
      auto it = ids.find(next);
      if (it == ids.end()) {
        if (sets.size() >= kMaxRawDfaStates)
          throw SlgError(SLG_ERR_UNSUPPORTED, "regex: the pattern's DFA has more than " + std::to_string(kMaxRawDfaStates) +
                                                  " states before minimisation (SLG_MAX_REGEX_STATES): CPU path");
        it = ids.emplace(next, (uint32_t)sets.size()).first;
        sets.push_back(std::move(next));
      }
      trans[s][c] = it->second;
    }
  }
  const size_t nraw = sets.size();
  std::vector<uint8_t> acc(nraw, 0);
  for (size_t s = 1; s < nraw; s++) {
    const std::vector<uint32_t> end = nfa.closure(sets[s], s == 1, true, mark);
    acc[s] = std::binary_search(end.begin(), end.end(), whole.e);
  }

  // Moore: refine {accepting, not} by the blocks of the targets until nothing splits
  std::vector<uint32_t> block(nraw);
  for (size_t s = 0; s < nraw; s++) block[s] = acc[s];
  size_t n_blocks = 0;
  for (;;) {
    std::map<std::vector<uint32_t>, uint32_t> sig_id;
    std::vector<uint32_t> next(nraw), sig(npre + 1);
    for (size_t s = 0; s < nraw; s++) {
      sig[0] = block[s];
      for (size_t c = 0; c < npre; c++) sig[c + 1] = block[trans[s][c]];
      next[s] = sig_id.emplace(sig, (uint32_t)sig_id.size()).first->second;
    }
    block.swap(next);
    if (sig_id.size() == n_blocks) break;
    n_blocks = sig_id.size();
  }
  // number the blocks: the dead state's 0, the start's 1, the rest as the subset construction met them
  std::vector<uint32_t> number(n_blocks, kInf);
  std::vector<uint32_t> member;  // a raw state of each minimised state
  const bool empty_language = block[1] == block[0];
  number[block[0]] = 0;
  member.push_back(0);
  if (!empty_language) {
    number[block[1]] = 1;
    member.push_back(1);
    for (size_t s = 2; s < nraw; s++)
      if (number[block[s]] == kInf) {
        number[block[s]] = (uint32_t)member.size();
        member.push_back((uint32_t)s);
      }
  } else {
    member.push_back(0);  // (a start state of its own that only leads to the dead state)
  }
  const size_t n_states = member.size();

  // byte classes: provisional classes with equal columns over the minimised states
  std::map<std::vector<uint32_t>, uint8_t> col_id;
  std::vector<uint8_t> class_of_pre(npre);
  std::vector<std::vector<uint32_t>> cols;
  for (size_t c = 0; c < npre; c++) {
    std::vector<uint32_t> col(n_states);
    for (size_t s = 0; s < n_states; s++) col[s] = number[block[trans[member[s]][c]]];
    auto it = col_id.find(col);
    if (it == col_id.end()) {
      it = col_id.emplace(col, (uint8_t)cols.size()).first;
      cols.push_back(std::move(col));
    }
    class_of_pre[c] = it->second;
  }
  const size_t n_classes = cols.size();
  if (n_states > SLG_MAX_REGEX_STATES)
    throw SlgError(SLG_ERR_UNSUPPORTED, "regex: a minimised DFA of " + std::to_string(n_states) +
                                            " states, more than SLG_MAX_REGEX_STATES: CPU path");
  if (n_states * n_classes > SLG_MAX_REGEX_TABLE)
    throw SlgError(SLG_ERR_UNSUPPORTED, "regex: a transition table of " + std::to_string(n_states) + " states x " +
                                            std::to_string(n_classes) + " byte classes, more than SLG_MAX_REGEX_TABLE bytes: CPU path");
  Dfa d;
  d.n_states = (uint32_t)n_states;
  d.n_classes = (uint32_t)n_classes;
  for (uint32_t b = 0; b < 256; b++) d.class_of[b] = class_of_pre[pre_of[b]];
  d.table.resize(n_states * n_classes);
  for (size_t s = 0; s < n_states; s++)
    for (size_t c = 0; c < n_classes; c++) d.table[s * n_classes + c] = (uint8_t)cols[c][s];
  d.accept.assign(32, 0);
  for (size_t s = 1; s < n_states; s++)
    if (!(empty_language && s == 1) && acc[member[s]]) d.accept[s >> 3] |= (uint8_t)(1u << (s & 7));
  return d;
}

}  // namespace slgregex
