// Template text to tree: the action lexer, the action parser and the block
// parser (see tmpl_internal.hpp for the pieces of the engine).
#include <cctype>
#include <cmath>
#include <cstdlib>

#include "cpilot/gotext.hpp"
#include "tmpl_internal.hpp"

namespace cpilot {
namespace tmpl {
namespace {

// ---------- lexer for actions ----------

struct ActionTok {
  enum class Kind { Ident, Field, Var, Str, Num, Bool, LParen, RParen, Pipe,
                    Declare, Comma, End } kind;
  std::string text;
  Value val;                 // Num / Bool
  bool spaceBefore = false;  // whitespace (or the delimiter) precedes it
};

bool isActionSpace(char c) {
  return c == ' ' || c == '\t' || c == '\r' || c == '\n';
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
        int d = gotext::hexVal(c);
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
    if (!gotext::isDecimalFloat(mag)) bad();
    bool isFloat = mag.find_first_of(".eE") != std::string::npos;
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
          gotext::appendUtf8(out, cp);
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
      int d = pos_ < s_.size() ? gotext::hexVal(s_[pos_]) : -1;
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

}  // namespace

std::vector<NodePtr> parseTemplate(const std::string& text) {
  return TemplateParser(text).parse();
}

}  // namespace tmpl
}  // namespace cpilot
