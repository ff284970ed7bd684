// The config functions of the template engine, all but regexReplaceAll,
// and the builtins that compare, measure and index values.
#include <cstdlib>

#include "cpilot/gotext.hpp"
#include "tmpl_internal.hpp"

namespace cpilot {
namespace tmpl {

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

namespace {

// strings.Split(s, ""): one element per UTF-8 sequence
ValueList explode(const std::string& s) {
  ValueList out;
  for (size_t i = 0; i < s.size();) {
    size_t n = gotext::utf8SeqLen(s, i);
    if (n == 0) n = 1;
    out.push_back(Value::str(s.substr(i, n)));
    i += n;
  }
  return out;
}

}  // namespace

Value fnSplit(const std::vector<Value>& args) {
  if (args.size() != 2) fail("wrong number of args for split");
  const std::string& sep = wantStr(args[0], "split", "the separator");
  // TrimSpace first (template.go:19-25)
  std::string s = gotext::trimSpace(wantStr(args[1], "split", "the value"));
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

namespace {

// loop's ensureInt: an int, or a string strconv.Atoi accepts
int64_t loopInt(const Value& v) {
  if (v.kind == Value::Kind::Int) return v.i;
  int64_t out = 0;
  if (v.kind == Value::Kind::Str) {
    if (gotext::atoi(v.s, &out)) return out;
    fail("loop: parsing \"" + v.s + "\": invalid syntax");
  }
  fail(std::string("loop: expected an integer, got ") + v.typeName());
}

}  // namespace

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

}  // namespace tmpl
}  // namespace cpilot
