// How template values print: %v floats, Value::print, print/println,
// printf and %q.
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cpilot/gotext.hpp"
#include "tmpl_internal.hpp"

namespace cpilot {
namespace tmpl {

// ---------- float printing (fmt's %v for float64) ----------

namespace {

// Shortest digits that round-trip; exponent form when the decimal exponent
// is below -4 or at least kExponentThreshold, with a sign and at least two
// exponent digits.
constexpr int kExponentThreshold = 21;

std::string formatFloatV(double f) {
  if (std::isnan(f)) return "NaN";
  if (std::isinf(f)) return f > 0 ? "+Inf" : "-Inf";
  char buf[64];
  auto res = std::to_chars(buf, buf + sizeof(buf), f,
                           std::chars_format::scientific);
  std::string sci(buf, res.ptr);  // [-]d[.ddd]e[+-]XX
  std::string out;
  size_t i = 0;
  if (sci[0] == '-') {
    out = "-";
    i = 1;
  }
  size_t e = sci.find('e');
  std::string digits;
  for (size_t k = i; k < e; k++)
    if (sci[k] != '.') digits += sci[k];
  int exp = atoi(sci.c_str() + e + 1);
  if (exp < -4 || exp >= kExponentThreshold) {
    out += digits[0];
    if (digits.size() > 1) out += "." + digits.substr(1);
    char ebuf[16];
    snprintf(ebuf, sizeof(ebuf), "e%c%02d", exp < 0 ? '-' : '+', abs(exp));
    return out + ebuf;
  }
  if (exp < 0) {
    out += "0." + std::string((size_t)(-exp - 1), '0') + digits;
    return out;
  }
  size_t intDigits = (size_t)exp + 1;
  if (digits.size() <= intDigits) {
    out += digits + std::string(intDigits - digits.size(), '0');
  } else {
    out += digits.substr(0, intDigits) + "." + digits.substr(intDigits);
  }
  return out;
}

}  // namespace

std::string Value::print() const {
  switch (kind) {
    case Kind::Nil: return "";
    case Kind::Str: return s;
    case Kind::Int: return std::to_string(i);
    case Kind::Float: return formatFloatV(f);
    case Kind::Bool: return b ? "true" : "false";
    case Kind::List: {
      std::string out = "[";
      bool first = true;
      for (auto& e : *list) {
        if (!first) out += " ";
        first = false;
        out += e.print();
      }
      return out + "]";
    }
    case Kind::Map: {
      // fmt's map[k:v k:v], keys sorted
      std::string out = "map[";
      bool first = true;
      for (auto& kv : *map) {
        if (!first) out += " ";
        first = false;
        out += kv.first + ":" + kv.second.print();
      }
      return out + "]";
    }
  }
  return "";
}

Value fnPrint(const std::vector<Value>& args, bool newline) {
  // fmt.Sprint semantics: spaces between operands when neither is a string
  std::string out;
  for (size_t i = 0; i < args.size(); i++) {
    if (i > 0 && args[i - 1].kind != Value::Kind::Str &&
        args[i].kind != Value::Kind::Str && !newline)
      out += " ";
    else if (i > 0 && newline)
      out += " ";  // Sprintln: always spaces
    out += args[i].print();
  }
  if (newline) out += "\n";
  return Value::str(out);
}

namespace {

// strconv.Quote. Which code points Go prints as they are depends on its
// Unicode tables; the ranges known here are exact, anything else non-ASCII
// is refused rather than guessed.
std::string goQuote(const std::string& s) {
  std::string out = "\"";
  char buf[16];
  for (size_t i = 0; i < s.size();) {
    uint32_t cp;
    size_t n = gotext::utf8SeqLen(s, i, &cp);
    if (n == 0) {
      snprintf(buf, sizeof(buf), "\\x%02x", (unsigned char)s[i]);
      out += buf;
      i++;
      continue;
    }
    if (cp == '"' || cp == '\\') {
      out += '\\';
      out += (char)cp;
    } else if (cp >= 0x20 && cp < 0x7F) {
      out += (char)cp;
    } else if (cp == '\a') out += "\\a";
    else if (cp == '\b') out += "\\b";
    else if (cp == '\f') out += "\\f";
    else if (cp == '\n') out += "\\n";
    else if (cp == '\r') out += "\\r";
    else if (cp == '\t') out += "\\t";
    else if (cp == '\v') out += "\\v";
    else if (cp < 0x20 || cp == 0x7F) {
      snprintf(buf, sizeof(buf), "\\x%02x", (unsigned)cp);
      out += buf;
    } else if ((cp >= 0x80 && cp <= 0xA0) || cp == 0xAD) {
      snprintf(buf, sizeof(buf), "\\u%04x", (unsigned)cp);
      out += buf;
    } else if ((cp >= 0xA1 && cp <= 0x36F) || (cp >= 0x400 && cp <= 0x4FF) ||
               (cp >= 0x3041 && cp <= 0x3096) ||
               (cp >= 0x30A1 && cp <= 0x30FA) ||
               (cp >= 0x4E00 && cp <= 0x9FA5)) {
      out.append(s, i, n);
    } else {
      snprintf(buf, sizeof(buf), "U+%04X", (unsigned)cp);
      fail(std::string("printf: %q of code point ") + buf +
           " is not supported");
    }
    i += n;
  }
  return out + "\"";
}

}  // namespace

// printf with the verbs %s %v %d %f %q %t %x %% and the flags '-', '0',
// width and .precision. Where fmt would print a %!verb(...) complaint, this
// is an error.
Value fnPrintf(const std::vector<Value>& args) {
  if (args.empty()) fail("printf needs a format string");
  if (args[0].kind != Value::Kind::Str) fail("printf format must be string");
  const std::string& fmt = args[0].s;
  std::string out;
  size_t argi = 1;
  for (size_t i = 0; i < fmt.size(); i++) {
    if (fmt[i] != '%') {
      out += fmt[i];
      continue;
    }
    size_t specStart = i++;
    bool minus = false, zero = false;
    for (; i < fmt.size() && (fmt[i] == '-' || fmt[i] == '0'); i++)
      (fmt[i] == '-' ? minus : zero) = true;
    long width = -1, prec = -1;
    auto readNum = [&]() {
      long v = 0;
      for (; i < fmt.size() && isdigit((unsigned char)fmt[i]); i++) {
        v = v * 10 + (fmt[i] - '0');
        if (v > 10000) fail("printf: width or precision too large");
      }
      return v;
    };
    if (i < fmt.size() && isdigit((unsigned char)fmt[i])) width = readNum();
    if (i < fmt.size() && fmt[i] == '.') {
      i++;
      prec = readNum();
    }
    if (i >= fmt.size()) fail("printf: format ends inside a verb");
    char verb = fmt[i];
    std::string spec = fmt.substr(specStart, i - specStart + 1);
    if (verb == '%') {
      if (spec != "%%") fail("printf: unsupported verb " + spec);
      out += '%';
      continue;
    }
    if (!strchr("svdfqtx", verb)) fail("printf: unsupported verb " + spec);
    if (argi >= args.size()) fail("printf: not enough args for " + spec);
    const Value& a = args[argi++];
    auto wrongType = [&]() {
      fail("printf: " + spec + " of a value of type " + a.typeName());
    };
    bool numeric = verb == 'd' || verb == 'f' ||
                   (verb == 'x' && a.kind == Value::Kind::Int);
    if (zero && !numeric) fail("printf: unsupported flag 0 in " + spec);
    if (prec >= 0 && verb != 'f' && verb != 's')
      fail("printf: unsupported precision in " + spec);
    std::string sign, body;
    switch (verb) {
      case 's':
        if (a.kind != Value::Kind::Str) wrongType();
        body = a.s;
        if (prec >= 0) {
          // at most prec code points
          size_t pos = 0;
          for (long k = 0; k < prec && pos < body.size(); k++) {
            size_t len = gotext::utf8SeqLen(body, pos);
            pos += len ? len : 1;
          }
          body.resize(pos);
        }
        break;
      case 'v':
        body = a.print();
        break;
      case 'q':
        if (a.kind != Value::Kind::Str) wrongType();
        body = goQuote(a.s);
        break;
      case 't':
        if (a.kind != Value::Kind::Bool) wrongType();
        body = a.b ? "true" : "false";
        break;
      case 'd':
      case 'x': {
        if (verb == 'x' && a.kind == Value::Kind::Str) {
          char buf[4];
          for (unsigned char c : a.s) {
            snprintf(buf, sizeof(buf), "%02x", c);
            body += buf;
          }
          break;
        }
        int64_t v = 0;
        if (a.kind == Value::Kind::Int) v = a.i;
        else if (verb == 'd' && a.kind == Value::Kind::Str && gotext::atoi(a.s, &v)) {
          // a numeric string under %d: kept from before, Go has %!d(string=7)
        } else wrongType();
        uint64_t mag = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
        if (v < 0) sign = "-";
        char buf[32];
        snprintf(buf, sizeof(buf), verb == 'd' ? "%llu" : "%llx",
                 (unsigned long long)mag);
        body = buf;
        break;
      }
      case 'f': {
        if (a.kind != Value::Kind::Float) wrongType();
        if (std::isnan(a.f) || std::isinf(a.f)) {
          body = formatFloatV(a.f);
          zero = false;
          break;
        }
        if (std::signbit(a.f)) sign = "-";
        std::vector<char> buf(400 + (size_t)(prec < 0 ? 6 : prec));
        snprintf(buf.data(), buf.size(), "%.*f", (int)(prec < 0 ? 6 : prec),
                 std::fabs(a.f));
        body = buf.data();
        break;
      }
    }
    size_t have = sign.size() + gotext::runeCount(body);
    size_t pad = width > 0 && (size_t)width > have ? (size_t)width - have : 0;
    if (minus) out += sign + body + std::string(pad, ' ');
    else if (zero) out += sign + std::string(pad, '0') + body;
    else out += std::string(pad, ' ') + sign + body;
  }
  if (argi < args.size()) fail("printf: too many args for the format");
  return Value::str(out);
}

}  // namespace tmpl
}  // namespace cpilot
