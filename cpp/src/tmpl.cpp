#include "cpilot/tmpl.hpp"

#include <cctype>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <regex>
#include <stdexcept>
#include <vector>

extern char** environ;

namespace cpilot {
namespace {

[[noreturn]] void fail(const std::string& msg) {
  throw std::runtime_error("template: " + msg);
}

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

// Length in bytes of the well-formed UTF-8 sequence at s[i], 0 if there is
// none (bad lead byte, truncation, overlong form, surrogate, > U+10FFFF).
size_t utf8SeqLen(const std::string& s, size_t i, uint32_t* cpOut = nullptr) {
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

// Strict decode; false on any malformed sequence.
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

// Code points of s for width/precision purposes; a malformed byte counts
// as one, as Go's rune iteration does.
size_t runeCount(const std::string& s) {
  size_t n = 0;
  for (size_t i = 0; i < s.size(); n++) {
    size_t len = utf8SeqLen(s, i);
    i += len ? len : 1;
  }
  return n;
}

// unicode.IsSpace
bool isGoSpace(uint32_t cp) {
  return (cp >= 0x09 && cp <= 0x0D) || cp == 0x20 || cp == 0x85 ||
         cp == 0xA0 || cp == 0x1680 || (cp >= 0x2000 && cp <= 0x200A) ||
         cp == 0x2028 || cp == 0x2029 || cp == 0x202F || cp == 0x205F ||
         cp == 0x3000;
}

// strings.TrimSpace
std::string goTrimSpace(const std::string& s) {
  size_t a = 0, b = s.size();
  while (a < b) {
    uint32_t cp;
    size_t n = utf8SeqLen(s, a, &cp);
    if (n == 0 || !isGoSpace(cp) || a + n > b) break;
    a += n;
  }
  while (b > a) {
    // step back to the lead byte of the last sequence
    size_t k = b - 1;
    while (k > a && ((unsigned char)s[k] & 0xC0) == 0x80 && b - k < 4) k--;
    uint32_t cp;
    size_t n = utf8SeqLen(s, k, &cp);
    if (n == 0 || k + n != b || !isGoSpace(cp)) break;
    b = k;
  }
  return s.substr(a, b - a);
}

// [+-]?[0-9]+ within int64: what strconv.Atoi accepts
bool strictAtoi(const std::string& s, int64_t* out) {
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

// ---------- float printing (fmt's %v for float64) ----------

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

// ---------- values ----------

struct Value;
using ValueList = std::vector<Value>;
using ValueMap = std::map<std::string, Value>;

struct Value {
  enum class Kind { Nil, Str, Int, Float, Bool, List, Map };
  Kind kind = Kind::Nil;
  std::string s;
  int64_t i = 0;
  double f = 0;
  bool b = false;
  std::shared_ptr<ValueList> list;
  std::shared_ptr<ValueMap> map;

  static Value nil() { return Value{}; }
  static Value str(std::string v) {
    Value r;
    r.kind = Kind::Str;
    r.s = std::move(v);
    return r;
  }
  static Value integer(int64_t v) {
    Value r;
    r.kind = Kind::Int;
    r.i = v;
    return r;
  }
  static Value number(double v) {
    Value r;
    r.kind = Kind::Float;
    r.f = v;
    return r;
  }
  static Value boolean(bool v) {
    Value r;
    r.kind = Kind::Bool;
    r.b = v;
    return r;
  }
  static Value mklist(ValueList v) {
    Value r;
    r.kind = Kind::List;
    r.list = std::make_shared<ValueList>(std::move(v));
    return r;
  }
  static Value mkmap(ValueMap v) {
    Value r;
    r.kind = Kind::Map;
    r.map = std::make_shared<ValueMap>(std::move(v));
    return r;
  }

  // .key on a map; a missing key is the zero value "" (missingkey=zero),
  // and so is a field of anything that is not a map
  Value field(const std::string& key) const {
    if (kind != Kind::Map) return Value::str("");
    auto it = map->find(key);
    return it == map->end() ? Value::str("") : it->second;
  }

  bool truthy() const {
    switch (kind) {
      case Kind::Nil: return false;
      case Kind::Str: return !s.empty();
      case Kind::Int: return i != 0;
      case Kind::Float: return f != 0;
      case Kind::Bool: return b;
      case Kind::List: return list && !list->empty();
      case Kind::Map: return map && !map->empty();
    }
    return false;
  }

  const char* typeName() const {
    switch (kind) {
      case Kind::Nil: return "nil";
      case Kind::Str: return "string";
      case Kind::Int: return "int";
      case Kind::Float: return "float64";
      case Kind::Bool: return "bool";
      case Kind::List: return "list";
      case Kind::Map: return "map";
    }
    return "?";
  }

  std::string print() const {
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
};

const std::string& wantStr(const Value& v, const char* fn, const char* what) {
  if (v.kind != Value::Kind::Str)
    fail(std::string(fn) + ": " + what + " must be a string, got " +
         v.typeName());
  return v.s;
}

// ---------- expression AST ----------

struct Expr;
using ExprPtr = std::shared_ptr<Expr>;

struct Expr {
  enum class Kind { Field, Var, StrLit, Lit, Call, Pipeline, Dot } kind;
  std::vector<std::string> path;  // Field: .A.B  / Var: name, then .A.B
  std::string strval;
  Value litval;                 // Lit: number or bool
  std::string fname;            // Call
  std::vector<ExprPtr> args;    // Call
  std::vector<ExprPtr> stages;  // Pipeline
};

// ---------- template AST ----------

struct Node;
using NodePtr = std::shared_ptr<Node>;

struct Node {
  enum class Kind { Text, Action, If, Range, Assign, With } kind;
  std::string text;               // Text
  ExprPtr expr;                   // Action/If/Range/With/Assign rhs
  std::vector<std::string> decl;  // variables declared by the header
  std::vector<NodePtr> body;      // If/Range/With
  std::vector<NodePtr> elseBody;  // If/Range/With
};

// ---------- lexer for actions ----------

struct ActionTok {
  enum class Kind { Ident, Field, Var, Str, Num, Bool, LParen, RParen, Pipe,
                    Declare, Comma, End } kind;
  std::string text;
  Value val;                 // Num / Bool
  bool spaceBefore = false;  // whitespace (or the delimiter) precedes it
};

bool isIdentChar(char c) { return isalnum((unsigned char)c) || c == '_'; }
bool isActionSpace(char c) {
  return c == ' ' || c == '\t' || c == '\r' || c == '\n';
}

int hexVal(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  if (c >= 'A' && c <= 'F') return c - 'A' + 10;
  return -1;
}

class ActionLexer {
 public:
  explicit ActionLexer(std::string s) : s_(std::move(s)) {}

  ActionTok next() {
    size_t before = pos_;
    while (pos_ < s_.size() && isActionSpace(s_[pos_])) pos_++;
    ActionTok t = lexOne();
    t.spaceBefore = before == 0 || pos0_ != before;
    return t;
  }

 private:
  std::string s_;
  size_t pos_ = 0;
  size_t pos0_ = 0;  // where the current token starts

  ActionTok make(ActionTok::Kind k, std::string text) {
    ActionTok t;
    t.kind = k;
    t.text = std::move(text);
    return t;
  }

  ActionTok lexOne() {
    pos0_ = pos_;
    if (pos_ >= s_.size()) return make(ActionTok::Kind::End, "");
    char c = s_[pos_];
    if (c == '(') { pos_++; return make(ActionTok::Kind::LParen, "("); }
    if (c == ')') { pos_++; return make(ActionTok::Kind::RParen, ")"); }
    if (c == '|') { pos_++; return make(ActionTok::Kind::Pipe, "|"); }
    if (c == ',') { pos_++; return make(ActionTok::Kind::Comma, ","); }
    if (c == ':' && pos_ + 1 < s_.size() && s_[pos_ + 1] == '=') {
      pos_ += 2;
      return make(ActionTok::Kind::Declare, ":=");
    }
    if (c == '"' || c == '`') return lexString(c);
    if (c == '\'') fail("character constants are not supported");
    if (c == '.' && !(pos_ + 1 < s_.size() &&
                      isdigit((unsigned char)s_[pos_ + 1]))) {
      // .A.B.C as one token; "." alone is the dot
      std::string path;
      while (pos_ < s_.size() && s_[pos_] == '.') {
        size_t start = ++pos_;
        while (pos_ < s_.size() && isIdentChar(s_[pos_])) pos_++;
        if (pos_ == start) {
          if (path.empty() && !(pos_ < s_.size() && s_[pos_] == '.'))
            return make(ActionTok::Kind::Field, "");  // the dot
          fail("unexpected '.' in action");
        }
        path += "." + s_.substr(start, pos_ - start);
      }
      return make(ActionTok::Kind::Field, path);
    }
    if (c == '$') {
      // $name, with an optional field path riding along: $v.A.B
      size_t start = ++pos_;
      while (pos_ < s_.size() && isIdentChar(s_[pos_])) pos_++;
      std::string name = s_.substr(start, pos_ - start);
      while (pos_ < s_.size() && s_[pos_] == '.') {
        size_t fstart = ++pos_;
        while (pos_ < s_.size() && isIdentChar(s_[pos_])) pos_++;
        if (pos_ == fstart) fail("unexpected '.' after variable");
        name += "." + s_.substr(fstart, pos_ - fstart);
      }
      return make(ActionTok::Kind::Var, name);
    }
    if (isdigit((unsigned char)c) || c == '-' || c == '+' || c == '.')
      return lexNumber();
    if (isalpha((unsigned char)c) || c == '_') {
      size_t start = pos_;
      while (pos_ < s_.size() && isIdentChar(s_[pos_])) pos_++;
      std::string name = s_.substr(start, pos_ - start);
      if (name == "true" || name == "false") {
        ActionTok t = make(ActionTok::Kind::Bool, name);
        t.val = Value::boolean(name == "true");
        return t;
      }
      return make(ActionTok::Kind::Ident, name);
    }
    fail(std::string("unexpected character '") + c + "' in action");
  }

  // Go number syntax: decimal, 0x hex, leading-0 octal, floats with an
  // optional exponent. A number is a float when its text has '.', 'e' or
  // 'E' (and is not hex), an int otherwise.
  ActionTok lexNumber() {
    size_t start = pos_;
    if (s_[pos_] == '+' || s_[pos_] == '-') pos_++;
    size_t body = pos_;
    bool hex = pos_ + 1 < s_.size() && s_[pos_] == '0' &&
               (s_[pos_ + 1] == 'x' || s_[pos_ + 1] == 'X');
    while (pos_ < s_.size()) {
      char c = s_[pos_];
      if (isalnum((unsigned char)c) || c == '.' || c == '_') {
        pos_++;
      } else if ((c == '+' || c == '-') && !hex && pos_ > body &&
                 (s_[pos_ - 1] == 'e' || s_[pos_ - 1] == 'E')) {
        pos_++;
      } else {
        break;
      }
    }
    std::string text = s_.substr(start, pos_ - start);
    std::string mag = s_.substr(body, pos_ - body);
    bool neg = text[0] == '-';
    ActionTok t = make(ActionTok::Kind::Num, text);
    auto bad = [&]() { fail("bad number syntax: \"" + text + "\""); };
    auto fromMagnitude = [&](uint64_t v) {
      const uint64_t two63 = (uint64_t)1 << 63;
      if (v > two63 || (!neg && v == two63))
        fail("integer constant " + text + " overflows int");
      return Value::integer(neg ? (int64_t)(0 - v) : (int64_t)v);
    };
    auto parseBase = [&](const std::string& digits, int base) {
      if (digits.empty()) bad();
      uint64_t v = 0;
      for (char c : digits) {
        int d = hexVal(c);
        if (d < 0 || d >= base) bad();
        if (v > (UINT64_MAX - (uint64_t)d) / (uint64_t)base)
          fail("integer constant " + text + " overflows int");
        v = v * (uint64_t)base + (uint64_t)d;
      }
      return v;
    };
    if (hex) {
      t.val = fromMagnitude(parseBase(mag.substr(2), 16));
      return t;
    }
    // digits* ('.' digits*)? ([eE] [+-]? digits+)?  with a mantissa digit
    size_t k = 0;
    size_t intDigits = 0, fracDigits = 0;
    bool isFloat = false;
    while (k < mag.size() && isdigit((unsigned char)mag[k])) k++, intDigits++;
    if (k < mag.size() && mag[k] == '.') {
      isFloat = true;
      k++;
      while (k < mag.size() && isdigit((unsigned char)mag[k])) k++, fracDigits++;
    }
    if (intDigits + fracDigits == 0) bad();
    if (k < mag.size() && (mag[k] == 'e' || mag[k] == 'E')) {
      isFloat = true;
      k++;
      if (k < mag.size() && (mag[k] == '+' || mag[k] == '-')) k++;
      size_t expDigits = 0;
      while (k < mag.size() && isdigit((unsigned char)mag[k])) k++, expDigits++;
      if (expDigits == 0) bad();
    }
    if (k != mag.size()) bad();
    if (isFloat) {
      double v = strtod(mag.c_str(), nullptr);
      if (std::isinf(v)) fail("number " + text + " out of range");
      t.val = Value::number(neg ? -v : v);
      return t;
    }
    bool octal = mag.size() > 1 && mag[0] == '0' &&
                 mag.find_first_of("89") == std::string::npos;
    t.val = fromMagnitude(parseBase(mag, octal ? 8 : 10));
    return t;
  }

  // "..." with Go's escapes, or a `raw` string
  ActionTok lexString(char quote) {
    pos_++;
    std::string out;
    if (quote == '`') {
      size_t end = s_.find('`', pos_);
      if (end == std::string::npos) fail("unterminated raw quoted string");
      out = s_.substr(pos_, end - pos_);
      pos_ = end + 1;
      return make(ActionTok::Kind::Str, out);
    }
    while (true) {
      if (pos_ >= s_.size() || s_[pos_] == '\n')
        fail("unterminated quoted string");
      char c = s_[pos_++];
      if (c == '"') break;
      if (c != '\\') {
        out += c;
        continue;
      }
      if (pos_ >= s_.size()) fail("unterminated quoted string");
      char e = s_[pos_++];
      switch (e) {
        case 'a': out += '\a'; break;
        case 'b': out += '\b'; break;
        case 'f': out += '\f'; break;
        case 'n': out += '\n'; break;
        case 'r': out += '\r'; break;
        case 't': out += '\t'; break;
        case 'v': out += '\v'; break;
        case '\\': out += '\\'; break;
        case '"': out += '"'; break;
        case 'x': out += (char)readHex(2, "\\x"); break;
        case 'u':
        case 'U': {
          uint32_t cp = readHex(e == 'u' ? 4 : 8, e == 'u' ? "\\u" : "\\U");
          if (cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF))
            fail("invalid Unicode code point in string escape");
          appendUtf8(out, cp);
          break;
        }
        default:
          if (e >= '0' && e <= '7') {
            // \NNN: exactly three octal digits, at most \377
            uint32_t v = (uint32_t)(e - '0');
            for (int k = 0; k < 2; k++) {
              if (pos_ >= s_.size() || s_[pos_] < '0' || s_[pos_] > '7')
                fail("invalid octal escape in string");
              v = v * 8 + (uint32_t)(s_[pos_++] - '0');
            }
            if (v > 255) fail("invalid octal escape in string");
            out += (char)v;
            break;
          }
          fail(std::string("unknown escape \\") + e + " in string");
      }
    }
    return make(ActionTok::Kind::Str, out);
  }

  uint32_t readHex(int n, const char* what) {
    uint32_t v = 0;
    for (int k = 0; k < n; k++) {
      int d = pos_ < s_.size() ? hexVal(s_[pos_]) : -1;
      if (d < 0) fail(std::string("invalid ") + what + " escape in string");
      v = v * 16 + (uint32_t)d;
      pos_++;
    }
    return v;
  }
};

// ---------- action parser ----------

std::vector<std::string> splitPath(const std::string& p) {
  std::vector<std::string> out;
  std::string cur;
  for (char c : p) {
    if (c == '.') {
      if (!cur.empty()) out.push_back(cur);
      cur.clear();
    } else {
      cur += c;
    }
  }
  if (!cur.empty()) out.push_back(cur);
  return out;
}

bool isKnownFunction(const std::string& name) {
  static const char* const names[] = {
      "default", "env", "split", "join", "replaceAll", "regexReplaceAll",
      "loop", "printf", "print", "println", "len", "index", "eq", "ne",
      "lt", "le", "gt", "ge", "and", "or", "not"};
  for (auto n : names)
    if (name == n) return true;
  return false;
}

// Variables visible at the current point of the parse. As in Go, using an
// undefined variable is a parse error, whether or not the action runs.
using VarScope = std::vector<std::string>;

class ActionParser {
 public:
  ActionParser(std::string s, VarScope* vars) : lex_(std::move(s)), vars_(vars) {
    advance();
  }

  bool atEnd() const { return tok_.kind == ActionTok::Kind::End; }
  bool atIdent(const char* name) const {
    return tok_.kind == ActionTok::Kind::Ident && tok_.text == name;
  }
  std::string identText() const {
    return tok_.kind == ActionTok::Kind::Ident ? tok_.text : "";
  }
  void skipIdent() { advance(); }

  void expectEnd(const char* context) {
    if (!atEnd())
      fail(std::string("unexpected \"") + tok_.text + "\" in " + context);
  }

  // [$a [, $b] :=] pipeline, to the end of the action. The declared names
  // are returned; the caller adds them to the scope once the pipeline (which
  // cannot see them yet) is parsed.
  ExprPtr parseHeader(const char* context, size_t maxDecl,
                      std::vector<std::string>* decl) {
    decl->clear();
    if (tok_.kind == ActionTok::Kind::Var &&
        tok_.text.find('.') == std::string::npos) {
      ActionLexer savedLex = lex_;
      ActionTok savedTok = tok_;
      std::vector<std::string> names{tok_.text};
      advance();
      if (tok_.kind == ActionTok::Kind::Comma) {
        advance();
        if (tok_.kind != ActionTok::Kind::Var ||
            tok_.text.find('.') != std::string::npos)
          fail("expected variable after ','");
        names.push_back(tok_.text);
        advance();
        if (tok_.kind != ActionTok::Kind::Declare)
          fail(std::string("expected := after variables in ") + context);
      }
      if (tok_.kind == ActionTok::Kind::Declare) {
        if (names.size() > maxDecl)
          fail(std::string("too many declarations in ") + context);
        for (auto& n : names)
          if (n.empty()) fail("cannot declare $");
        advance();
        *decl = names;
      } else {
        lex_ = savedLex;
        tok_ = savedTok;
      }
    }
    ExprPtr e = parsePipeline();
    expectEnd(context);
    return e;
  }

 private:
  ActionLexer lex_;
  ActionTok tok_;
  VarScope* vars_;
  int parenDepth_ = 0;

  void advance() { tok_ = lex_.next(); }

  ExprPtr parsePipeline() {
    auto first = parseCommand();
    if (tok_.kind != ActionTok::Kind::Pipe) return first;
    auto pipe = std::make_shared<Expr>();
    pipe->kind = Expr::Kind::Pipeline;
    pipe->stages.push_back(first);
    while (tok_.kind == ActionTok::Kind::Pipe) {
      advance();
      auto stage = parseCommand();
      if (stage->kind != Expr::Kind::Call)
        fail("non executable command in pipeline stage " +
             std::to_string(pipe->stages.size() + 1));
      pipe->stages.push_back(stage);
    }
    return pipe;
  }

  bool atCommandEnd() const {
    return tok_.kind == ActionTok::Kind::End ||
           tok_.kind == ActionTok::Kind::Pipe ||
           tok_.kind == ActionTok::Kind::RParen;
  }

  // command: function arg*  |  operand
  ExprPtr parseCommand() {
    if (atCommandEnd()) fail("missing value for command");
    ExprPtr head;
    if (tok_.kind == ActionTok::Kind::Ident) {
      head = std::make_shared<Expr>();
      head->kind = Expr::Kind::Call;
      head->fname = tok_.text;
      if (head->fname == "define" || head->fname == "template" ||
          head->fname == "block")
        fail("{{" + head->fname + "}} is not supported");
      if (!isKnownFunction(head->fname))
        fail("function \"" + head->fname + "\" not defined");
      advance();
    } else {
      head = parseOperand();
    }
    while (!atCommandEnd()) {
      // operands are separated by space; `"a""b"` or `.A(` is an error
      if (!tok_.spaceBefore)
        fail("unexpected \"" + tok_.text + "\" in operand");
      if (head->kind != Expr::Kind::Call || parenthesised(head))
        fail("unexpected \"" + tok_.text +
             "\": can't give argument to non-function");
      if (tok_.kind == ActionTok::Kind::Ident)
        fail("function \"" + tok_.text +
             "\" as an argument needs parentheses");
      head->args.push_back(parseOperand());
    }
    return head;
  }

  std::vector<const Expr*> parens_;  // calls that came out of ( ... )
  bool parenthesised(const ExprPtr& e) const {
    for (auto p : parens_)
      if (p == e.get()) return true;
    return false;
  }

  ExprPtr parseOperand() {
    auto e = std::make_shared<Expr>();
    switch (tok_.kind) {
      case ActionTok::Kind::Field:
        if (tok_.text.empty()) {
          e->kind = Expr::Kind::Dot;
        } else {
          e->kind = Expr::Kind::Field;
          e->path = splitPath(tok_.text);
        }
        advance();
        return e;
      case ActionTok::Kind::Var: {
        e->kind = Expr::Kind::Var;
        size_t dot = tok_.text.find('.');
        e->path = {tok_.text.substr(0, dot)};
        if (dot != std::string::npos)
          for (auto& f : splitPath(tok_.text.substr(dot)))
            e->path.push_back(f);
        bool known = e->path[0].empty();  // "$" is always the root
        for (auto& v : *vars_)
          if (v == e->path[0]) known = true;
        if (!known) fail("undefined variable $" + e->path[0]);
        advance();
        return e;
      }
      case ActionTok::Kind::Str:
        e->kind = Expr::Kind::StrLit;
        e->strval = tok_.text;
        advance();
        return e;
      case ActionTok::Kind::Num:
      case ActionTok::Kind::Bool:
        e->kind = Expr::Kind::Lit;
        e->litval = tok_.val;
        advance();
        return e;
      case ActionTok::Kind::LParen: {
        if (++parenDepth_ > 100) fail("parentheses nested too deep");
        advance();
        auto inner = parsePipeline();
        if (tok_.kind != ActionTok::Kind::RParen) fail("unclosed left paren");
        advance();
        parenDepth_--;
        // (pipeline).Field would be a field of the result; not supported
        if (tok_.kind == ActionTok::Kind::Field && !tok_.spaceBefore)
          fail("a field of a parenthesised pipeline is not supported");
        parens_.push_back(inner.get());
        return inner;
      }
      case ActionTok::Kind::Ident:
        fail("function \"" + tok_.text +
             "\" as an argument needs parentheses");
      case ActionTok::Kind::RParen:
        fail("unexpected right paren");
      case ActionTok::Kind::Declare:
        fail("unexpected \":=\" in operand");
      default:
        fail("unexpected \"" + tok_.text + "\" in operand");
    }
  }
};

// ---------- template parser ----------

class TemplateParser {
 public:
  explicit TemplateParser(const std::string& text) : text_(text) {}

  std::vector<NodePtr> parse() { return parseNodes(nullptr); }

 private:
  const std::string& text_;
  size_t pos_ = 0;
  bool pendingTrim_ = false;  // previous action had a right-trim marker
  int depth_ = 0;
  VarScope vars_;

  // how a node list ended: {{end}}, {{else}}, or {{else if ...}} with the
  // parser standing after the "if"
  struct Terminator {
    enum class Kind { None, End, Else, ElseIf } kind = Kind::None;
    std::shared_ptr<ActionParser> rest;
  };

  // One {{ ... }}: finds the closing delimiter without being fooled by
  // "}}" inside a quoted string or a comment. Returns false for a comment.
  bool scanAction(size_t open, std::string* body, bool* trimL, bool* trimR,
                  size_t* after) {
    const size_t n = text_.size();
    size_t p = open + 2;
    *trimL = p + 1 < n && text_[p] == '-' && isActionSpace(text_[p + 1]);
    if (*trimL) p++;
    size_t q = p;
    while (q < n && isActionSpace(text_[q])) q++;
    if (text_.compare(q, 2, "/*") == 0) {
      size_t e = text_.find("*/", q + 2);
      if (e == std::string::npos) fail("unclosed comment");
      size_t r = e + 2;
      bool space = false;
      while (r < n && isActionSpace(text_[r])) r++, space = true;
      *trimR = space && r < n && text_[r] == '-';
      if (*trimR) r++;
      if (text_.compare(r, 2, "}}") != 0)
        fail("comment ends before closing delimiter");
      *after = r + 2;
      return false;
    }
    size_t i = p;
    while (true) {
      if (i >= n) fail("unclosed action");
      char c = text_[i];
      if (c == '"' || c == '\'') {
        size_t k = i + 1;
        while (true) {
          if (k >= n || text_[k] == '\n') fail("unterminated quoted string");
          if (text_[k] == '\\') {
            k += 2;
            continue;
          }
          if (text_[k] == c) break;
          k++;
        }
        i = k + 1;
      } else if (c == '`') {
        size_t k = text_.find('`', i + 1);
        if (k == std::string::npos) fail("unterminated raw quoted string");
        i = k + 1;
      } else if (c == '}' && i + 1 < n && text_[i + 1] == '}') {
        break;
      } else {
        i++;
      }
    }
    *trimR = i >= p + 2 && text_[i - 1] == '-' && isActionSpace(text_[i - 2]);
    *body = text_.substr(p, (*trimR ? i - 1 : i) - p);
    *after = i + 2;
    return true;
  }

  std::vector<NodePtr> parseNodes(Terminator* terminator) {
    if (++depth_ > 200) fail("block nesting too deep");
    std::vector<NodePtr> nodes;
    struct DepthGuard {
      int& d;
      ~DepthGuard() { d--; }
    } guard{depth_};
    while (pos_ < text_.size()) {
      size_t open = text_.find("{{", pos_);
      std::string raw = text_.substr(
          pos_, (open == std::string::npos ? text_.size() : open) - pos_);
      if (open == std::string::npos) {
        emitText(nodes, raw, false);
        pos_ = text_.size();
        break;
      }
      std::string body;
      bool trimL = false, trimR = false;
      size_t after = 0;
      bool isAction = scanAction(open, &body, &trimL, &trimR, &after);
      emitText(nodes, raw, trimL);
      pos_ = after;
      pendingTrim_ = trimR;
      if (!isAction) continue;  // {{/* comment */}}

      auto ap = std::make_shared<ActionParser>(body, &vars_);
      std::string keyword = ap->identText();
      if (keyword == "end") {
        ap->skipIdent();
        ap->expectEnd("{{end}}");
        if (!terminator) fail("unexpected {{end}}");
        terminator->kind = Terminator::Kind::End;
        return nodes;
      }
      if (keyword == "else") {
        ap->skipIdent();
        if (!terminator) fail("unexpected {{else}}");
        if (ap->atIdent("if")) {
          ap->skipIdent();
          terminator->kind = Terminator::Kind::ElseIf;
          terminator->rest = ap;
        } else {
          ap->expectEnd("{{else}}");
          terminator->kind = Terminator::Kind::Else;
        }
        return nodes;
      }
      if (keyword == "if" || keyword == "with" || keyword == "range") {
        ap->skipIdent();
        nodes.push_back(parseControl(keyword, *ap));
        continue;
      }
      // {{ $x := pipeline }} or {{ pipeline }}
      auto node = std::make_shared<Node>();
      node->expr = ap->parseHeader("command", 1, &node->decl);
      node->kind = node->decl.empty() ? Node::Kind::Action : Node::Kind::Assign;
      for (auto& v : node->decl) vars_.push_back(v);
      nodes.push_back(node);
    }
    if (terminator) fail("unexpected EOF, expected {{end}}");
    return nodes;
  }

  // {{if}}, {{with}} or {{range}} with the parser after the keyword; reads
  // through the matching {{end}}. Variables of the header are visible in
  // the body and the else branch; what a branch declares ends with it.
  NodePtr parseControl(const std::string& keyword, ActionParser& header) {
    auto node = std::make_shared<Node>();
    node->kind = keyword == "if"     ? Node::Kind::If
                 : keyword == "with" ? Node::Kind::With
                                     : Node::Kind::Range;
    size_t outer = vars_.size();
    node->expr = header.parseHeader(keyword.c_str(), keyword == "range" ? 2 : 1,
                                    &node->decl);
    for (auto& v : node->decl) vars_.push_back(v);
    size_t inner = vars_.size();
    Terminator term;
    node->body = parseNodes(&term);
    vars_.resize(inner);
    if (term.kind == Terminator::Kind::ElseIf) {
      if (keyword != "if") fail("{{else if}} is only allowed after {{if}}");
      // nested chain shares our {{end}}
      node->elseBody.push_back(parseControl("if", *term.rest));
    } else if (term.kind == Terminator::Kind::Else) {
      Terminator term2;
      node->elseBody = parseNodes(&term2);
      if (term2.kind != Terminator::Kind::End)
        fail("expected {{end}} to close " + keyword);
    }
    vars_.resize(outer);
    return node;
  }

  // {{- and -}} trim space, tab, CR and LF, nothing else
  void emitText(std::vector<NodePtr>& nodes, std::string raw,
                bool trimRightOfText) {
    if (pendingTrim_) {
      size_t i = 0;
      while (i < raw.size() && isActionSpace(raw[i])) i++;
      raw = raw.substr(i);
      pendingTrim_ = false;
    }
    if (trimRightOfText) {
      size_t i = raw.size();
      while (i > 0 && isActionSpace(raw[i - 1])) i--;
      raw = raw.substr(0, i);
    }
    if (raw.empty()) return;
    auto node = std::make_shared<Node>();
    node->kind = Node::Kind::Text;
    node->text = std::move(raw);
    nodes.push_back(node);
  }
};

// ---------- functions (template.go:19-140) ----------

Value fnDefault(const std::vector<Value>& args) {
  if (args.size() != 2) fail("wrong number of args for default");
  const Value& defVal = args[0];
  const Value& tmplVal = args[1];
  if (tmplVal.kind == Value::Kind::Str && !tmplVal.s.empty())
    return tmplVal;
  if (defVal.kind == Value::Kind::Str) return defVal;
  return Value::str(defVal.print());
}

Value fnEnv(const std::vector<Value>& args) {
  if (args.size() != 1) fail("wrong number of args for env");
  const char* v = getenv(wantStr(args[0], "env", "the name").c_str());
  return Value::str(v ? v : "");
}

// strings.Split(s, ""): one element per UTF-8 sequence
ValueList explode(const std::string& s) {
  ValueList out;
  for (size_t i = 0; i < s.size();) {
    size_t n = utf8SeqLen(s, i);
    if (n == 0) n = 1;
    out.push_back(Value::str(s.substr(i, n)));
    i += n;
  }
  return out;
}

Value fnSplit(const std::vector<Value>& args) {
  if (args.size() != 2) fail("wrong number of args for split");
  const std::string& sep = wantStr(args[0], "split", "the separator");
  // TrimSpace first (template.go:19-25)
  std::string s = goTrimSpace(wantStr(args[1], "split", "the value"));
  ValueList out;
  if (s.empty()) return Value::mklist(out);
  if (sep.empty()) return Value::mklist(explode(s));
  size_t pos = 0;
  while (true) {
    size_t next = s.find(sep, pos);
    if (next == std::string::npos) {
      out.push_back(Value::str(s.substr(pos)));
      break;
    }
    out.push_back(Value::str(s.substr(pos, next - pos)));
    pos = next + sep.size();
  }
  return Value::mklist(out);
}

Value fnJoin(const std::vector<Value>& args) {
  if (args.size() != 2) fail("wrong number of args for join");
  const std::string& sep = wantStr(args[0], "join", "the separator");
  if (args[1].kind != Value::Kind::List) fail("join expects a list");
  std::string out;
  bool first = true;
  for (auto& e : *args[1].list) {
    if (!first) out += sep;
    first = false;
    out += wantStr(e, "join", "every element");
  }
  return Value::str(out);
}

Value fnReplaceAll(const std::vector<Value>& args) {
  if (args.size() != 3) fail("wrong number of args for replaceAll");
  const std::string& from = wantStr(args[0], "replaceAll", "the pattern");
  const std::string& to = wantStr(args[1], "replaceAll", "the replacement");
  const std::string& s = wantStr(args[2], "replaceAll", "the value");
  std::string out;
  if (from.empty()) {
    // strings.Replace: before every code point and at the end
    out = to;
    for (auto& piece : explode(s)) out += piece.s + to;
    return Value::str(out);
  }
  size_t pos = 0;
  while (true) {
    size_t next = s.find(from, pos);
    if (next == std::string::npos) {
      out += s.substr(pos);
      break;
    }
    out += s.substr(pos, next - pos);
    out += to;
    pos = next + from.size();
  }
  return Value::str(out);
}

// ---------- regexReplaceAll: Go's regexp on top of std::wregex ----------
//
// The pattern is checked and rewritten from RE2 syntax into the ECMAScript
// subset std::wregex shares with it; whatever cannot be honoured exactly is
// an error that names the construct. Matching runs on code points, and the
// replacement loop and the $-expansion are Go's, done by hand.

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
  if (!decodeUtf8(pattern, &pat)) reFail(pattern, "invalid UTF-8");
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
        int d = pat[k] < 0x80 ? hexVal((char)pat[k]) : -1;
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
      int d = i < n && pat[i] < 0x80 ? hexVal((char)pat[i]) : -1;
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
    appendUtf8(name, c);
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

Value fnRegexReplaceAll(const std::vector<Value>& args) {
  if (args.size() != 3) fail("wrong number of args for regexReplaceAll");
  GoRegex re = compileGoRegex(wantStr(args[0], "regexReplaceAll", "the pattern"));
  const std::string& repl = wantStr(args[1], "regexReplaceAll", "the replacement");
  const std::string& src = wantStr(args[2], "regexReplaceAll", "the value");
  std::u32string cps;
  if (!decodeUtf8(src, &cps))
    fail("regexReplaceAll: the value is not valid UTF-8");
  if (cps.size() > 65536)
    fail("regexReplaceAll: the value is longer than 65536 characters");
  std::wstring subject(cps.begin(), cps.end());
  auto toBytes = [](std::wstring::const_iterator a,
                    std::wstring::const_iterator b) {
    std::string out;
    for (; a != b; ++a) appendUtf8(out, (uint32_t)*a);
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

// loop's ensureInt: an int, or a string strconv.Atoi accepts
int64_t loopInt(const Value& v) {
  if (v.kind == Value::Kind::Int) return v.i;
  int64_t out = 0;
  if (v.kind == Value::Kind::Str) {
    if (strictAtoi(v.s, &out)) return out;
    fail("loop: parsing \"" + v.s + "\": invalid syntax");
  }
  fail(std::string("loop: expected an integer, got ") + v.typeName());
}

Value fnLoop(const std::vector<Value>& args) {
  int64_t start = 0, stop = 0;
  if (args.size() == 1) {
    stop = loopInt(args[0]);
  } else if (args.size() == 2) {
    start = loopInt(args[0]);
    stop = loopInt(args[1]);
  } else {
    throw std::runtime_error(
        "loop: wrong number of arguments, expected 1 or 2, but got " +
        std::to_string(args.size()));
  }
  uint64_t span = stop < start ? (uint64_t)start - (uint64_t)stop
                               : (uint64_t)stop - (uint64_t)start;
  if (span > 1000000) fail("loop: more than 1000000 elements");
  ValueList out;
  if (stop < start) {
    for (int64_t i = start; i > stop; i--) out.push_back(Value::integer(i));
  } else {
    for (int64_t i = start; i < stop; i++) out.push_back(Value::integer(i));
  }
  return Value::mklist(out);
}

// ---------- Go text/template builtins (always available in Go) ----------

bool valueEq(const Value& a, const Value& b) {
  bool aNum = a.kind == Value::Kind::Int || a.kind == Value::Kind::Float;
  bool bNum = b.kind == Value::Kind::Int || b.kind == Value::Kind::Float;
  if (aNum && bNum) {
    double av = a.kind == Value::Kind::Int ? (double)a.i : a.f;
    double bv = b.kind == Value::Kind::Int ? (double)b.i : b.f;
    return av == bv;
  }
  if (a.kind == Value::Kind::Bool || b.kind == Value::Kind::Bool)
    return a.truthy() == b.truthy();
  return a.print() == b.print();
}

int valueCmp(const Value& a, const Value& b) {
  bool aNum = a.kind == Value::Kind::Int || a.kind == Value::Kind::Float;
  bool bNum = b.kind == Value::Kind::Int || b.kind == Value::Kind::Float;
  if (aNum && bNum) {
    double av = a.kind == Value::Kind::Int ? (double)a.i : a.f;
    double bv = b.kind == Value::Kind::Int ? (double)b.i : b.f;
    return av < bv ? -1 : (av > bv ? 1 : 0);
  }
  return a.print().compare(b.print()) < 0
             ? -1
             : (a.print() == b.print() ? 0 : 1);
}

Value fnLen(const std::vector<Value>& args) {
  if (args.size() != 1) fail("wrong number of args for len");
  const Value& v = args[0];
  if (v.kind == Value::Kind::List) return Value::integer((int64_t)v.list->size());
  if (v.kind == Value::Kind::Str) return Value::integer((int64_t)v.s.size());
  if (v.kind == Value::Kind::Map) return Value::integer((int64_t)v.map->size());
  fail("len of unsupported type");
}

Value fnIndex(const std::vector<Value>& args) {
  if (args.size() != 2) fail("wrong number of args for index");
  if (args[0].kind == Value::Kind::Map) {
    if (args[1].kind != Value::Kind::Str)
      fail("index of map needs a string key");
    return args[0].field(args[1].s);
  }
  if (args[0].kind != Value::Kind::List && args[0].kind != Value::Kind::Str)
    fail("index of unsupported type");
  if (args[1].kind != Value::Kind::Int)
    fail(std::string("cannot index with type ") + args[1].typeName());
  int64_t i = args[1].i;
  if (args[0].kind == Value::Kind::List) {
    if (i < 0 || (size_t)i >= args[0].list->size())
      fail("index out of range");
    return (*args[0].list)[(size_t)i];
  }
  if (i < 0 || (size_t)i >= args[0].s.size()) fail("index out of range");
  return Value::integer((unsigned char)args[0].s[(size_t)i]);
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

// strconv.Quote. Which code points Go prints as they are depends on its
// Unicode tables; the ranges known here are exact, anything else non-ASCII
// is refused rather than guessed.
std::string goQuote(const std::string& s) {
  std::string out = "\"";
  char buf[16];
  for (size_t i = 0; i < s.size();) {
    uint32_t cp;
    size_t n = utf8SeqLen(s, i, &cp);
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
            size_t len = utf8SeqLen(body, pos);
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
        else if (verb == 'd' && a.kind == Value::Kind::Str && strictAtoi(a.s, &v)) {
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
    size_t have = sign.size() + runeCount(body);
    size_t pad = width > 0 && (size_t)width > have ? (size_t)width - have : 0;
    if (minus) out += sign + body + std::string(pad, ' ');
    else if (zero) out += sign + std::string(pad, '0') + body;
    else out += std::string(pad, ' ') + sign + body;
  }
  if (argi < args.size()) fail("printf: too many args for the format");
  return Value::str(out);
}

// ---------- evaluator ----------

class Evaluator {
 public:
  // "." and "$" start as `root`
  std::string exec(const std::vector<NodePtr>& nodes, const Value& root) {
    vars_.clear();
    vars_.emplace_back("", root);
    std::string out;
    execNodes(nodes, root, out);
    return out;
  }

 private:
  // Go's variable stack: a declaration pushes, the end of the enclosing
  // if/with/range (or of one range iteration) pops, lookups go from the top
  std::vector<std::pair<std::string, Value>> vars_;

  void execNodes(const std::vector<NodePtr>& nodes, const Value& dot,
                 std::string& out) {
    for (auto& n : nodes) {
      switch (n->kind) {
        case Node::Kind::Text:
          out += n->text;
          break;
        case Node::Kind::Action:
          out += eval(n->expr, dot).print();
          break;
        case Node::Kind::Assign:
          vars_.emplace_back(n->decl[0], eval(n->expr, dot));
          break;
        case Node::Kind::If:
        case Node::Kind::With: {
          size_t mark = vars_.size();
          Value v = eval(n->expr, dot);
          for (auto& name : n->decl) vars_.emplace_back(name, v);
          if (v.truthy())
            execNodes(n->body, n->kind == Node::Kind::With ? v : dot, out);
          else
            execNodes(n->elseBody, dot, out);
          vars_.resize(mark, {"", Value::nil()});
          break;
        }
        case Node::Kind::Range: {
          size_t mark = vars_.size();
          Value coll = eval(n->expr, dot);
          if (coll.kind != Value::Kind::List && coll.kind != Value::Kind::Nil)
            throw std::runtime_error("template: range over non-list value");
          // until an iteration sets them the variables hold the collection,
          // which is what {{else}} sees
          for (auto& name : n->decl) vars_.emplace_back(name, coll);
          size_t inner = vars_.size();
          if (coll.kind == Value::Kind::List && !coll.list->empty()) {
            int64_t idx = 0;
            for (auto& item : *coll.list) {
              if (n->decl.size() >= 1) vars_[inner - 1].second = item;
              if (n->decl.size() >= 2)
                vars_[inner - 2].second = Value::integer(idx);
              execNodes(n->body, item, out);
              vars_.resize(inner, {"", Value::nil()});
              idx++;
            }
          } else {
            execNodes(n->elseBody, dot, out);
          }
          vars_.resize(mark, {"", Value::nil()});
          break;
        }
      }
    }
  }

  Value eval(const ExprPtr& e, const Value& dot) {
    switch (e->kind) {
      case Expr::Kind::StrLit:
        return Value::str(e->strval);
      case Expr::Kind::Lit:
        return e->litval;
      case Expr::Kind::Dot:
        return dot;
      case Expr::Kind::Field: {
        // missing key, or a field of a non-map value: missingkey=zero
        Value v = dot;
        for (auto& key : e->path) v = v.field(key);
        return v;
      }
      case Expr::Kind::Var: {
        for (size_t k = vars_.size(); k-- > 0;) {
          if (vars_[k].first != e->path[0]) continue;
          Value v = vars_[k].second;
          for (size_t i = 1; i < e->path.size(); i++) v = v.field(e->path[i]);
          return v;
        }
        fail("undefined variable $" + e->path[0]);
      }
      case Expr::Kind::Call: {
        std::vector<Value> args;
        for (auto& a : e->args) args.push_back(eval(a, dot));
        return callFn(e->fname, args);
      }
      case Expr::Kind::Pipeline: {
        Value v = eval(e->stages[0], dot);
        for (size_t i = 1; i < e->stages.size(); i++) {
          auto& stage = e->stages[i];
          std::vector<Value> args;
          for (auto& a : stage->args) args.push_back(eval(a, dot));
          args.push_back(v);  // piped value becomes the last argument
          v = callFn(stage->fname, args);
        }
        return v;
      }
    }
    return Value::nil();
  }

  Value callFn(const std::string& name, const std::vector<Value>& args) {
    if (name == "default") return fnDefault(args);
    if (name == "env") return fnEnv(args);
    if (name == "split") return fnSplit(args);
    if (name == "join") return fnJoin(args);
    if (name == "replaceAll") return fnReplaceAll(args);
    if (name == "regexReplaceAll") return fnRegexReplaceAll(args);
    if (name == "loop") return fnLoop(args);
    if (name == "printf") return fnPrintf(args);
    // Go text/template builtins (template.go's FuncMap only ADDS funcs;
    // the language builtins are always available to reference configs)
    if (name == "eq") {
      if (args.size() < 2) fail("wrong number of args for eq");
      for (size_t i = 1; i < args.size(); i++)
        if (valueEq(args[0], args[i])) return Value::boolean(true);
      return Value::boolean(false);
    }
    if (name == "ne") {
      if (args.size() != 2) fail("wrong number of args for ne");
      return Value::boolean(!valueEq(args[0], args[1]));
    }
    if (name == "lt" || name == "le" || name == "gt" || name == "ge") {
      if (args.size() != 2) fail("wrong number of args for " + name);
      int c = valueCmp(args[0], args[1]);
      bool r = (name == "lt")   ? c < 0
               : (name == "le") ? c <= 0
               : (name == "gt") ? c > 0
                                : c >= 0;
      return Value::boolean(r);
    }
    if (name == "and") {
      if (args.empty()) fail("wrong number of args for and");
      for (auto& a : args)
        if (!a.truthy()) return a;
      return args.back();
    }
    if (name == "or") {
      if (args.empty()) fail("wrong number of args for or");
      for (auto& a : args)
        if (a.truthy()) return a;
      return args.back();
    }
    if (name == "not") {
      if (args.size() != 1) fail("wrong number of args for not");
      return Value::boolean(!args[0].truthy());
    }
    if (name == "len") return fnLen(args);
    if (name == "index") return fnIndex(args);
    if (name == "print") return fnPrint(args, false);
    if (name == "println") return fnPrint(args, true);
    fail("function \"" + name + "\" not defined");
  }
};

Value fromJson(const Json& j) {
  switch (j.type()) {
    case Json::Type::Null: return Value::nil();
    case Json::Type::Bool: return Value::boolean(j.boolean());
    case Json::Type::Int: return Value::integer(j.asInt());
    case Json::Type::Double: return Value::number(j.asDouble());
    case Json::Type::String: return Value::str(j.str());
    case Json::Type::Array: {
      ValueList out;
      for (auto& e : j.array()) out.push_back(fromJson(e));
      return Value::mklist(std::move(out));
    }
    case Json::Type::Object: {
      ValueMap out;
      for (auto& kv : j.object()) out[kv.first] = fromJson(kv.second);
      return Value::mkmap(std::move(out));
    }
  }
  return Value::nil();
}

// the environment as the root map: NAME -> value
Value environmentRoot() {
  ValueMap env;
  for (char** e = environ; *e; e++) {
    const char* eq = strchr(*e, '=');
    if (!eq) continue;
    env[std::string(*e, (size_t)(eq - *e))] = Value::str(std::string(eq + 1));
  }
  return Value::mkmap(std::move(env));
}

}  // namespace

struct Template::Impl {
  std::vector<NodePtr> nodes;
};

Template Template::parse(const std::string& text) {
  auto impl = std::make_shared<Impl>();
  TemplateParser parser(text);
  impl->nodes = parser.parse();
  Template t;
  t.impl_ = std::move(impl);
  return t;
}

std::string Template::render(const Json& data) const {
  if (!impl_) throw std::runtime_error("template: not parsed");
  Evaluator ev;
  return ev.exec(impl_->nodes, fromJson(data));
}

std::string renderTemplate(const std::string& text) {
  TemplateParser parser(text);
  auto nodes = parser.parse();
  Evaluator ev;
  return ev.exec(nodes, environmentRoot());
}

}  // namespace cpilot
