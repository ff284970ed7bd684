// regexReplaceAll: the whole of the template engine's regular expressions.
#include <cctype>
#include <cwchar>
#include <regex>

#include "cpilot/gotext.hpp"
#include "tmpl_internal.hpp"

namespace cpilot {
namespace tmpl {

// ---------- regexReplaceAll: Go's regexp on top of std::wregex ----------
//
// The pattern is checked and rewritten from RE2 syntax into the ECMAScript
// subset std::wregex shares with it; whatever cannot be honoured exactly is
// an error that names the construct. Matching runs on code points, and the
// replacement loop and the $-expansion are Go's, done by hand.

namespace {

struct GoRegex {
  std::wregex re;
  std::vector<std::string> groupNames;  // [0] unused; "" for unnamed
};

[[noreturn]] void reFail(const std::string& pattern, const std::string& why) {
  fail("regexReplaceAll: error parsing regexp `" + pattern + "`: " + why);
}

void emitLiteral(std::wstring& out, uint32_t cp) {
  if (cp >= 0x80 || isalnum((int)cp) || cp == ' ') {
    out += (wchar_t)cp;
  } else {
    wchar_t buf[8];
    swprintf(buf, 8, L"\\x%02x", (unsigned)cp);
    out += buf;
  }
}

GoRegex compileGoRegex(const std::string& pattern) {
  std::u32string pat;
  if (!gotext::decodeUtf8(pattern, &pat)) reFail(pattern, "invalid UTF-8");
  if (pat.size() > 1000) reFail(pattern, "expression too large");
  GoRegex out;
  out.groupNames.push_back("");
  std::wstring w;
  size_t i = 0;
  const size_t n = pat.size();
  bool icase = false;
  auto startsWith = [&](size_t at, const char* lit) {
    for (size_t k = 0; lit[k]; k++)
      if (at + k >= n || pat[at + k] != (uint32_t)(unsigned char)lit[k])
        return false;
    return true;
  };
  if (startsWith(0, "(?i)")) {
    icase = true;
    i = 4;
  }
  auto literal = [&](uint32_t cp) {
    if (icase && cp >= 0x80)
      reFail(pattern, "(?i) with a non-ASCII literal is not supported");
    emitLiteral(w, cp);
  };
  auto readHexEscape = [&]() -> uint32_t {
    // i stands after "\x"
    uint32_t v = 0;
    if (i < n && pat[i] == '{') {
      size_t k = i + 1, digits = 0;
      while (k < n && pat[k] != '}') {
        int d = pat[k] < 0x80 ? gotext::hexVal((char)pat[k]) : -1;
        if (d < 0 || ++digits > 6) reFail(pattern, "invalid escape sequence: `\\x{`");
        v = v * 16 + (uint32_t)d;
        k++;
      }
      if (k >= n || digits == 0 || v > 0x10FFFF || (v >= 0xD800 && v <= 0xDFFF))
        reFail(pattern, "invalid escape sequence: `\\x{`");
      i = k + 1;
      return v;
    }
    for (int k = 0; k < 2; k++) {
      int d = i < n && pat[i] < 0x80 ? gotext::hexVal((char)pat[i]) : -1;
      if (d < 0) reFail(pattern, "invalid escape sequence: `\\x`");
      v = v * 16 + (uint32_t)d;
      i++;
    }
    return v;
  };
  // i stands after the backslash
  auto escape = [&](bool inClass) {
    if (i >= n) reFail(pattern, "trailing backslash at end of expression");
    uint32_t c = pat[i++];
    std::string name = "\\";
    gotext::appendUtf8(name, c);
    switch (c) {
      case 'd': w += inClass ? L"0-9" : L"[0-9]"; return;
      case 'w': w += inClass ? L"0-9A-Za-z_" : L"[0-9A-Za-z_]"; return;
      case 's': w += inClass ? L"\\t\\n\\f\\r " : L"[\\t\\n\\f\\r ]"; return;
      case 'D':
      case 'W':
      case 'S':
        if (inClass)
          reFail(pattern, "`" + name + "` inside [...] is not supported");
        w += c == 'D' ? L"[^0-9]" : c == 'W' ? L"[^0-9A-Za-z_]"
                                             : L"[^\\t\\n\\f\\r ]";
        return;
      case 'b':
      case 'B':
        if (inClass) reFail(pattern, "invalid escape sequence: `" + name + "`");
        w += L'\\';
        w += (wchar_t)c;
        return;
      case 'n': w += L"\\n"; return;
      case 't': w += L"\\t"; return;
      case 'r': w += L"\\r"; return;
      case 'f': w += L"\\f"; return;
      case 'v': w += L"\\v"; return;
      case 'a': w += L"\\x07"; return;
      case 'x': literal(readHexEscape()); return;
      case 'p':
      case 'P':
        reFail(pattern, "Unicode class `" + name + "` is not supported");
      case 'z':
      case 'A':
      case 'Q':
      case 'E':
      case 'C':
        reFail(pattern, "`" + name + "` is not supported");
      default:
        break;
    }
    if (c >= '1' && c <= '9')
      reFail(pattern, "backreference `" + name + "` is not supported by Go");
    if (c >= 0x80 || isalnum((int)c))
      reFail(pattern, "invalid escape sequence: `" + name + "`");
    literal(c);  // escaped punctuation
  };
  int depth = 0;
  // Go refuses a repetition operator with nothing to repeat and one stacked
  // on another (a**, a+*); only a single lazy '?' may follow one
  enum class Prev { Nothing, Atom, Repeat, Lazy } prev = Prev::Nothing;
  bool sawRepeat = false, sawLazy = false;
  auto repetition = [&](const std::string& op) {
    if (prev == Prev::Nothing)
      reFail(pattern, "missing argument to repetition operator: `" + op + "`");
    if (prev == Prev::Lazy || (prev == Prev::Repeat && op != "?"))
      reFail(pattern, "invalid nested repetition operator");
    sawRepeat = true;
    sawLazy = prev == Prev::Repeat;
  };
  while (i < n) {
    uint32_t c = pat[i];
    if (c == '\\') {
      i++;
      escape(false);
    } else if (c == '[') {
      w += L'[';
      i++;
      if (i < n && pat[i] == '^') {
        w += L'^';
        i++;
      }
      bool first = true, closed = false;
      while (i < n) {
        uint32_t cc = pat[i];
        if (cc == ']' && !first) {
          closed = true;
          i++;
          break;
        }
        first = false;
        if (cc == '\\') {
          i++;
          escape(true);
        } else if (cc == '[') {
          if (startsWith(i, "[:")) {
            size_t k = i + 2;
            std::wstring cls = L"[:";
            while (k < n && pat[k] >= 'a' && pat[k] <= 'z') cls += (wchar_t)pat[k++];
            if (!startsWith(k, ":]"))
              reFail(pattern, "invalid character class range");
            w += cls + L":]";
            i = k + 2;
          } else if (startsWith(i, "[.") || startsWith(i, "[=")) {
            reFail(pattern, "collating classes are not supported");
          } else {
            literal(cc);
            i++;
          }
        } else if (cc == '-') {
          w += L'-';
          i++;
        } else {
          literal(cc);
          i++;
        }
      }
      if (!closed) reFail(pattern, "missing closing ]");
      w += L']';
    } else if (c == '(') {
      depth++;
      if (startsWith(i, "(?:")) {
        w += L"(?:";
        i += 3;
      } else if (startsWith(i, "(?P<")) {
        size_t k = i + 4;
        std::string name;
        while (k < n && pat[k] < 0x80 && isIdentChar((char)pat[k]))
          name += (char)pat[k++];
        if (name.empty() || k >= n || pat[k] != '>')
          reFail(pattern, "invalid named capture");
        for (auto& g : out.groupNames)
          if (g == name) reFail(pattern, "duplicate capture group name");
        out.groupNames.push_back(name);
        w += L'(';
        i = k + 1;
      } else if (startsWith(i, "(?=") || startsWith(i, "(?!") ||
                 startsWith(i, "(?<")) {
        reFail(pattern, "lookaround is not supported by Go");
      } else if (startsWith(i, "(?")) {
        reFail(pattern,
               "flags are only supported as (?i) at the start of the pattern");
      } else {
        out.groupNames.push_back("");
        w += L'(';
        i++;
      }
    } else if (c == ')') {
      if (--depth < 0) reFail(pattern, "unexpected )");
      w += L')';
      i++;
    } else if (c == '.') {
      w += L"[^\\n]";  // ECMAScript's dot also excludes \r and U+2028/9
      i++;
    } else if (c == '{') {
      // a well-formed {n}, {n,} or {n,m} repeats; anything else is literal
      size_t k = i + 1;
      long lo = -1, hi = -1;
      auto readNum = [&]() {
        long v = -1;
        while (k < n && pat[k] >= '0' && pat[k] <= '9') {
          v = (v < 0 ? 0 : v) * 10 + (long)(pat[k] - '0');
          if (v > 1000) reFail(pattern, "invalid repeat count");
          k++;
        }
        return v;
      };
      lo = readNum();
      bool comma = k < n && pat[k] == ',';
      if (comma) {
        k++;
        hi = readNum();
      }
      if (lo >= 0 && k < n && pat[k] == '}') {
        if (comma && hi >= 0 && hi < lo) reFail(pattern, "invalid repeat count");
        repetition("{}");
        for (size_t j = i; j <= k; j++) w += (wchar_t)pat[j];
        i = k + 1;
      } else {
        literal(c);
        i++;
      }
    } else if (c == '*' || c == '+' || c == '?') {
      repetition(std::string(1, (char)c));
      w += (wchar_t)c;
      i++;
    } else if (c == '|' || c == '^' || c == '$') {
      w += (wchar_t)c;
      i++;
    } else {
      literal(c);
      i++;
    }
    // what the next repetition operator would apply to
    if (sawRepeat) {
      prev = sawLazy ? Prev::Lazy : Prev::Repeat;
    } else {
      prev = (c == '(' || c == '|') ? Prev::Nothing : Prev::Atom;
    }
    sawRepeat = sawLazy = false;
  }
  if (depth != 0) reFail(pattern, "missing closing )");
  try {
    auto flags = std::regex::ECMAScript;
    if (icase) flags |= std::regex::icase;
    out.re = std::wregex(w, flags);
  } catch (const std::regex_error& e) {
    reFail(pattern, e.what());
  }
  return out;
}

// Regexp.Expand for one match: $$, $name, ${name}; an all-digit name is an
// index; unknown, out-of-range and unmatched groups expand to nothing; a
// malformed reference leaves the '$' as text.
void expandReplacement(const std::string& repl, const GoRegex& re,
                       const std::wsmatch& m,
                       const std::vector<std::string>& groupBytes,
                       std::string& out) {
  size_t i = 0;
  while (i < repl.size()) {
    if (repl[i] != '$') {
      out += repl[i++];
      continue;
    }
    if (i + 1 < repl.size() && repl[i + 1] == '$') {
      out += '$';
      i += 2;
      continue;
    }
    size_t k = i + 1;
    bool brace = k < repl.size() && repl[k] == '{';
    if (brace) k++;
    size_t start = k;
    while (k < repl.size() && isIdentChar(repl[k])) k++;
    if (k < repl.size() && ((unsigned char)repl[k] & 0x80))
      fail("regexReplaceAll: a non-ASCII character after a $name in the "
           "replacement is not supported");
    std::string name = repl.substr(start, k - start);
    if (name.empty() || (brace && (k >= repl.size() || repl[k] != '}'))) {
      out += '$';  // malformed
      i++;
      continue;
    }
    if (brace) k++;
    i = k;
    long num = 0;
    for (char c : name) {
      if (c < '0' || c > '9' || num >= 100000000) {
        num = -1;
        break;
      }
      num = num * 10 + (c - '0');
    }
    if (name[0] == '0' && name.size() > 1) num = -1;
    if (num < 0) {
      for (size_t g = 1; g < re.groupNames.size(); g++)
        if (re.groupNames[g] == name) {
          num = (long)g;
          break;
        }
    }
    if (num >= 0 && (size_t)num < m.size() && m[(size_t)num].matched)
      out += groupBytes[(size_t)num];
  }
}

}  // namespace

Value fnRegexReplaceAll(const std::vector<Value>& args) {
  if (args.size() != 3) fail("wrong number of args for regexReplaceAll");
  GoRegex re = compileGoRegex(wantStr(args[0], "regexReplaceAll", "the pattern"));
  const std::string& repl = wantStr(args[1], "regexReplaceAll", "the replacement");
  const std::string& src = wantStr(args[2], "regexReplaceAll", "the value");
  std::u32string cps;
  if (!gotext::decodeUtf8(src, &cps))
    fail("regexReplaceAll: the value is not valid UTF-8");
  if (cps.size() > 65536)
    fail("regexReplaceAll: the value is longer than 65536 characters");
  std::wstring subject(cps.begin(), cps.end());
  auto toBytes = [](std::wstring::const_iterator a,
                    std::wstring::const_iterator b) {
    std::string out;
    for (; a != b; ++a) gotext::appendUtf8(out, (uint32_t)*a);
    return out;
  };
  // Regexp.ReplaceAllString: leftmost matches in turn; an empty match that
  // abuts the previous match is not replaced; always advance.
  std::string out;
  size_t lastEnd = 0, searchPos = 0;
  try {
    while (searchPos <= subject.size()) {
      std::wsmatch m;
      auto flags = std::regex_constants::match_default;
      if (searchPos > 0) flags |= std::regex_constants::match_prev_avail;
      if (!std::regex_search(subject.cbegin() + (long)searchPos, subject.cend(),
                             m, re.re, flags))
        break;
      size_t a0 = (size_t)(m[0].first - subject.cbegin());
      size_t a1 = (size_t)(m[0].second - subject.cbegin());
      out += toBytes(subject.cbegin() + (long)lastEnd, m[0].first);
      if (a1 > lastEnd || a0 == 0) {
        std::vector<std::string> groups(m.size());
        for (size_t g = 0; g < m.size(); g++)
          if (m[g].matched) groups[g] = toBytes(m[g].first, m[g].second);
        expandReplacement(repl, re, m, groups, out);
      }
      lastEnd = a1;
      searchPos = a1 > searchPos ? a1 : searchPos + 1;
    }
  } catch (const std::regex_error& e) {
    fail(std::string("regexReplaceAll: ") + e.what());
  }
  if (lastEnd < subject.size())
    out += toBytes(subject.cbegin() + (long)lastEnd, subject.cend());
  return Value::str(out);
}

}  // namespace tmpl
}  // namespace cpilot
