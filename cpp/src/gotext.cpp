#include "cpilot/gotext.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <strings.h>

namespace cpilot {
namespace gotext {

// ---------- UTF-8 ----------

void appendUtf8(std::string& out, uint32_t cp) {
  if (cp < 0x80) {
    out += (char)cp;
  } else if (cp < 0x800) {
    out += (char)(0xC0 | (cp >> 6));
    out += (char)(0x80 | (cp & 0x3F));
  } else if (cp < 0x10000) {
    out += (char)(0xE0 | (cp >> 12));
    out += (char)(0x80 | ((cp >> 6) & 0x3F));
    out += (char)(0x80 | (cp & 0x3F));
  } else {
    out += (char)(0xF0 | (cp >> 18));
    out += (char)(0x80 | ((cp >> 12) & 0x3F));
    out += (char)(0x80 | ((cp >> 6) & 0x3F));
    out += (char)(0x80 | (cp & 0x3F));
  }
}

size_t utf8SeqLen(const std::string& s, size_t i, uint32_t* cpOut) {
  unsigned char c = (unsigned char)s[i];
  size_t len;
  uint32_t cp, min;
  if (c < 0x80) {
    if (cpOut) *cpOut = c;
    return 1;
  } else if ((c & 0xE0) == 0xC0) {
    len = 2; cp = c & 0x1F; min = 0x80;
  } else if ((c & 0xF0) == 0xE0) {
    len = 3; cp = c & 0x0F; min = 0x800;
  } else if ((c & 0xF8) == 0xF0) {
    len = 4; cp = c & 0x07; min = 0x10000;
  } else {
    return 0;
  }
  if (i + len > s.size()) return 0;
  for (size_t k = 1; k < len; k++) {
    unsigned char cc = (unsigned char)s[i + k];
    if ((cc & 0xC0) != 0x80) return 0;
    cp = (cp << 6) | (cc & 0x3F);
  }
  if (cp < min || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return 0;
  if (cpOut) *cpOut = cp;
  return len;
}

bool decodeUtf8(const std::string& s, std::u32string* out) {
  out->clear();
  for (size_t i = 0; i < s.size();) {
    uint32_t cp;
    size_t n = utf8SeqLen(s, i, &cp);
    if (n == 0) return false;
    out->push_back(cp);
    i += n;
  }
  return true;
}

size_t runeCount(const std::string& s) {
  size_t n = 0;
  for (size_t i = 0; i < s.size(); n++) {
    size_t len = utf8SeqLen(s, i);
    i += len ? len : 1;
  }
  return n;
}

// ---------- white space ----------

bool isSpace(uint32_t cp) {
  return (cp >= 0x09 && cp <= 0x0D) || cp == 0x20 || cp == 0x85 ||
         cp == 0xA0 || cp == 0x1680 || (cp >= 0x2000 && cp <= 0x200A) ||
         cp == 0x2028 || cp == 0x2029 || cp == 0x202F || cp == 0x205F ||
         cp == 0x3000;
}

std::string trimSpace(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a < b) {
    uint32_t cp;
    size_t n = utf8SeqLen(s, a, &cp);
    if (n == 0 || !isSpace(cp) || a + n > b) break;
    a += n;
  }
  while (b > a) {
    // step back to the lead byte of the last sequence
    size_t k = b - 1;
    while (k > a && ((unsigned char)s[k] & 0xC0) == 0x80 && b - k < 4) k--;
    uint32_t cp;
    size_t n = utf8SeqLen(s, k, &cp);
    if (n == 0 || k + n != b || !isSpace(cp)) break;
    b = k;
  }
  return s.substr(a, b - a);
}

// ---------- numbers ----------

bool atoi(const std::string& s, int64_t* out) {
  size_t i = 0;
  bool neg = false;
  if (i < s.size() && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
  if (i == s.size()) return false;
  const uint64_t two63 = (uint64_t)1 << 63;
  uint64_t v = 0;
  for (; i < s.size(); i++) {
    if (s[i] < '0' || s[i] > '9') return false;
    uint64_t d = (uint64_t)(s[i] - '0');
    if (v > (two63 - d) / 10) return false;
    v = v * 10 + d;
  }
  if (!neg && v == two63) return false;
  *out = neg ? (int64_t)(0 - v) : (int64_t)v;
  return true;
}

int hexVal(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  if (c >= 'A' && c <= 'F') return c - 'A' + 10;
  return -1;
}

bool isDecimalFloat(const std::string& s) {
  size_t i = 0;
  auto digits = [&] {
    size_t n = 0;
    while (i < s.size() && s[i] >= '0' && s[i] <= '9') i++, n++;
    return n;
  };
  size_t mantissa = digits();
  if (i < s.size() && s[i] == '.') {
    i++;
    mantissa += digits();
  }
  if (!mantissa) return false;
  if (i < s.size() && (s[i] == 'e' || s[i] == 'E')) {
    i++;
    if (i < s.size() && (s[i] == '+' || s[i] == '-')) i++;
    if (!digits()) return false;
  }
  return i == s.size();
}

bool parseFloat(const std::string& v, double* out) {
  size_t i = 0;
  bool neg = false, sign = false;
  if (i < v.size() && (v[i] == '+' || v[i] == '-')) {
    neg = v[i] == '-';
    sign = true;
    i++;
  }
  const char* rest = v.c_str() + i;
  if (v.size() - i == strlen(rest)) {  // no embedded NUL
    if (!strcasecmp(rest, "inf") || !strcasecmp(rest, "infinity")) {
      *out = neg ? -INFINITY : INFINITY;
      return true;
    }
    if (!sign && !strcasecmp(rest, "nan")) {
      *out = std::nan("");
      return true;
    }
  }
  if (!isDecimalFloat(v.substr(i))) return false;
  // the text is plain decimal now, which strtod rounds as Go does
  double val = strtod(v.c_str(), nullptr);
  if (std::isinf(val)) return false;  // Go: value out of range
  *out = val;
  return true;
}

}  // namespace gotext
}  // namespace cpilot
