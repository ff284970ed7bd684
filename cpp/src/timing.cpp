#include "cpilot/timing.hpp"

#include <cctype>
#include <cstdint>
#include <cstdlib>

#include "cpilot/gotext.hpp"

namespace cpilot {

namespace {

constexpr uint64_t kTwo63 = (uint64_t)1 << 63;

[[noreturn]] void invalidDuration(const std::string& s) {
  throw std::runtime_error("time: invalid duration " + s);
}

Duration secondsToDuration(int64_t sec) {
  constexpr int64_t kMaxSec = INT64_MAX / 1000000000;
  if (sec > kMaxSec || sec < -kMaxSec)
    throw std::runtime_error("time: duration of " + std::to_string(sec) +
                             " seconds overflows");
  return Duration(sec * 1000000000);
}

}  // namespace

Duration parseGoDuration(const std::string& orig) {
  // Go time.ParseDuration: [-+]?([0-9]*(\.[0-9]*)?[a-z]+)+ accumulated in
  // an unsigned integer; any step past 2^63 is an error, as is a positive
  // total past 2^63-1. "0" is allowed without a unit.
  size_t i = 0;
  const std::string& s = orig;
  bool neg = false;
  if (i < s.size() && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
  if (s.compare(i, std::string::npos, "0") == 0) return Duration(0);
  if (i == s.size()) invalidDuration(orig);
  uint64_t total = 0;
  while (i < s.size()) {
    if (!(s[i] == '.' || (s[i] >= '0' && s[i] <= '9'))) invalidDuration(orig);
    // [0-9]*
    uint64_t v = 0;
    size_t start = i;
    for (; i < s.size() && s[i] >= '0' && s[i] <= '9'; i++) {
      if (v > kTwo63 / 10) invalidDuration(orig);
      v = v * 10 + (uint64_t)(s[i] - '0');
      if (v > kTwo63) invalidDuration(orig);
    }
    bool pre = i != start;
    // (\.[0-9]*)? -- digits past what fits are dropped, as Go does
    uint64_t frac = 0;
    double scale = 1;
    bool post = false;
    if (i < s.size() && s[i] == '.') {
      i++;
      start = i;
      bool overflow = false;
      for (; i < s.size() && s[i] >= '0' && s[i] <= '9'; i++) {
        if (overflow) continue;
        if (frac > (kTwo63 - 1) / 10) {
          overflow = true;
          continue;
        }
        uint64_t y = frac * 10 + (uint64_t)(s[i] - '0');
        if (y > kTwo63) {
          overflow = true;
          continue;
        }
        frac = y;
        scale *= 10;
      }
      post = i != start;
    }
    if (!pre && !post) invalidDuration(orig);
    // unit: everything up to the next digit or dot
    start = i;
    while (i < s.size() && s[i] != '.' && !(s[i] >= '0' && s[i] <= '9')) i++;
    if (i == start)
      throw std::runtime_error("time: missing unit in duration " + orig);
    std::string unit = s.substr(start, i - start);
    uint64_t mult;
    if (unit == "ns") mult = 1;
    else if (unit == "us" || unit == "\xc2\xb5s" || unit == "\xce\xbcs")
      mult = 1000;
    else if (unit == "ms") mult = 1000000;
    else if (unit == "s") mult = 1000000000;
    else if (unit == "m") mult = 60000000000ULL;
    else if (unit == "h") mult = 3600000000000ULL;
    else
      throw std::runtime_error("time: unknown unit \"" + unit +
                               "\" in duration " + orig);
    if (v > kTwo63 / mult) invalidDuration(orig);
    v *= mult;
    if (frac > 0) {
      // the one float step Go takes: frac*(unit/scale) <= 3.6e12
      v += (uint64_t)((double)frac * ((double)mult / scale));
      if (v > kTwo63) invalidDuration(orig);
    }
    total += v;
    if (total > kTwo63) invalidDuration(orig);
  }
  if (neg) return Duration((int64_t)(0 - total));
  if (total > kTwo63 - 1) invalidDuration(orig);
  return Duration((int64_t)total);
}

Duration parseDuration(const Json& v) {
  if (v.isInt()) return secondsToDuration(v.asInt());
  if (v.isDouble()) {
    // the reference only accepts integer types here; a JSON5 float is an
    // error ("unexpected duration of type float64")
    throw std::runtime_error("unexpected duration of type float64");
  }
  if (v.isString()) {
    const std::string& s = v.str();
    // a string strconv.Atoi accepts = seconds, parsed as "<n>s"
    // (duration.go:53-55), so it overflows like any other duration
    int64_t sec = 0;
    if (gotext::atoi(s, &sec))
      return parseGoDuration(std::to_string(sec) + "s");
    return parseGoDuration(s);
  }
  throw std::runtime_error("unexpected duration type");
}

Duration getTimeout(const std::string& s) {
  if (s.empty()) return Duration(0);
  return parseDuration(Json(s));
}

bool parsePositiveDuration(const Json& v, Duration* out) {
  if (v.isString() &&
      (v.str().empty() || !isdigit((unsigned char)v.str()[0])))
    return false;
  if (!v.isString() && !v.isNumber()) return false;
  try {
    *out = parseDuration(v);
  } catch (const std::exception&) {
    return false;
  }
  return *out >= std::chrono::milliseconds(1);
}

std::string secondsString(int seconds) {
  return std::to_string(seconds) + "s";
}

}  // namespace cpilot
