// What the pieces of the template engine share: the value type, the two
// syntax trees, and each piece's entry points. Private to cpp/src; the
// public interface is cpilot/tmpl.hpp.
//
//   tmpl_parse.cpp  text -> tree: action lexer, action parser, block parser
//   tmpl_funcs.cpp  the config functions (all but the regex) and eq/len/index
//   tmpl_regex.cpp  regexReplaceAll: RE2 syntax on std::wregex, Go's expansion
//   tmpl_print.cpp  how values print: %v floats, print, printf, %q
//   tmpl.cpp        the evaluator and the public Template / renderTemplate
#pragma once

#include <cctype>
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace cpilot {
namespace tmpl {

[[noreturn]] inline void fail(const std::string& msg) {
  throw std::runtime_error("template: " + msg);
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

  std::string print() const;  // fmt's %v (tmpl_print.cpp)
};

inline const std::string& wantStr(const Value& v, const char* fn,
                                  const char* what) {
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

// ---------- tmpl_parse.cpp ----------

inline bool isIdentChar(char c) {
  return isalnum((unsigned char)c) || c == '_';
}

// Throws std::runtime_error on anything Go's parser would refuse.
std::vector<NodePtr> parseTemplate(const std::string& text);

// ---------- tmpl_funcs.cpp ----------

Value fnDefault(const std::vector<Value>& args);
Value fnEnv(const std::vector<Value>& args);
Value fnSplit(const std::vector<Value>& args);
Value fnJoin(const std::vector<Value>& args);
Value fnReplaceAll(const std::vector<Value>& args);
Value fnLoop(const std::vector<Value>& args);
bool valueEq(const Value& a, const Value& b);
int valueCmp(const Value& a, const Value& b);
Value fnLen(const std::vector<Value>& args);
Value fnIndex(const std::vector<Value>& args);

// ---------- tmpl_regex.cpp ----------

Value fnRegexReplaceAll(const std::vector<Value>& args);

// ---------- tmpl_print.cpp ----------

Value fnPrint(const std::vector<Value>& args, bool newline);
Value fnPrintf(const std::vector<Value>& args);

}  // namespace tmpl
}  // namespace cpilot
