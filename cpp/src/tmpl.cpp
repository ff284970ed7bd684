// The evaluator of the template engine and its public interface; parsing,
// functions, regexps and printing live in the tmpl_*.cpp files next to it.
#include "cpilot/tmpl.hpp"

#include <cstring>

#include "tmpl_internal.hpp"

extern char** environ;

namespace cpilot {
namespace tmpl {
namespace {

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
}  // namespace tmpl

struct Template::Impl {
  std::vector<tmpl::NodePtr> nodes;
};

Template Template::parse(const std::string& text) {
  auto impl = std::make_shared<Impl>();
  impl->nodes = tmpl::parseTemplate(text);
  Template t;
  t.impl_ = std::move(impl);
  return t;
}

std::string Template::render(const Json& data) const {
  if (!impl_) throw std::runtime_error("template: not parsed");
  tmpl::Evaluator ev;
  return ev.exec(impl_->nodes, tmpl::fromJson(data));
}

std::string renderTemplate(const std::string& text) {
  auto nodes = tmpl::parseTemplate(text);
  tmpl::Evaluator ev;
  return ev.exec(nodes, tmpl::environmentRoot());
}

}  // namespace cpilot
