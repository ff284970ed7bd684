"""A plain model of the Go semantics the native engine has to match.

Written from Go's documented behaviour (text/template, fmt, strconv,
strings, regexp, time) and the rules in docs/30-configuration.md. It shares
no code with the C++ engine and never parses a template: tests build an
AST, `serialize` turns it into template text for the engine, and
`evaluate` computes what Go would print for the same AST.

Values are Python values: str, int, float, bool, list, dict and None.

Expressions (tuples):
    ("str", s) ("int", n) ("float", f) ("bool", b)
    ("dot",)                      .
    ("field", [names])            .A.B on the dot
    ("var", name, [names])        $name.A.B; name "" is the root "$"
    ("call", fname, [args])       fname a b c
    ("pipe", first, [calls])      first | f a | g; the piped value becomes
                                  the last argument of each call

Template nodes (tuples; else_ is None, a node list, or an ("if", ...) node
for {{else if}}):
    ("text", s) ("comment", s) ("action", expr) ("assign", name, expr)
    ("if", decl, expr, body, else_)      decl: None or a variable name
    ("with", decl, expr, body, else_)
    ("range", decls, expr, body, else_)  decls: [] / [v] / [i, v]
"""

import re
from decimal import Decimal

INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1
TRIM_CHARS = " \t\r\n"
# unicode.IsSpace, which strings.TrimSpace uses
GO_SPACE = ("\t\n\v\f\r \u0085\u00a0\u1680\u2000\u2001\u2002\u2003\u2004"
            "\u2005\u2006\u2007\u2008\u2009\u200a\u2028\u2029\u202f\u205f"
            "\u3000")
# exponent form when the decimal exponent is < -4 or >= this
FLOAT_EXPONENT_THRESHOLD = 21


class GoError(Exception):
    """Go would report an error (at parse or at execution) here."""


# ---------------------------------------------------------------- durations

_UNITS = {"ns": 1, "us": 10**3, "µs": 10**3, "μs": 10**3,
          "ms": 10**6, "s": 10**9, "m": 60 * 10**9, "h": 3600 * 10**9}
_ATOI = re.compile(r"[+-]?[0-9]+\Z")


def atoi(s):
    """strconv.Atoi on a 64-bit platform: the int, or None."""
    if not _ATOI.match(s):
        return None
    v = int(s)
    return v if INT64_MIN <= v <= INT64_MAX else None


def go_parse_duration(s):
    """time.ParseDuration with integers only. The fraction is computed
    exactly, which equals Go's one float step whenever unit / 10^digits is
    a whole number of nanoseconds times a power of ten that float64 holds
    exactly (ns: 0 digits, us: 3, ms: 6, s/m/h: 9)."""
    orig = s
    neg = False
    if s and s[0] in "+-":
        neg = s[0] == "-"
        s = s[1:]
    if s == "0":
        return 0
    if s == "":
        raise GoError("time: invalid duration " + orig)
    total = 0
    while s:
        if not (s[0] == "." or s[0] in "0123456789"):
            raise GoError("time: invalid duration " + orig)
        i = 0
        v = 0
        while i < len(s) and s[i] in "0123456789":
            if v > (1 << 63) // 10:
                raise GoError("time: invalid duration " + orig)
            v = v * 10 + int(s[i])
            if v > 1 << 63:
                raise GoError("time: invalid duration " + orig)
            i += 1
        pre = i > 0
        s = s[i:]
        frac, scale, post = 0, 1, False
        if s and s[0] == ".":
            s = s[1:]
            i = 0
            overflow = False
            while i < len(s) and s[i] in "0123456789":
                if not overflow:
                    if frac > INT64_MAX // 10:
                        overflow = True
                    else:
                        y = frac * 10 + int(s[i])
                        if y > 1 << 63:
                            overflow = True
                        else:
                            frac, scale = y, scale * 10
                i += 1
            post = i > 0
            s = s[i:]
        if not pre and not post:
            raise GoError("time: invalid duration " + orig)
        i = 0
        while i < len(s) and s[i] != "." and s[i] not in "0123456789":
            i += 1
        if i == 0:
            raise GoError("time: missing unit in duration " + orig)
        unit = _UNITS.get(s[:i])
        if unit is None:
            raise GoError("time: unknown unit in duration " + orig)
        s = s[i:]
        if v > (1 << 63) // unit:
            raise GoError("time: invalid duration " + orig)
        v *= unit
        if frac > 0:
            v += frac * unit // scale
            if v > 1 << 63:
                raise GoError("time: invalid duration " + orig)
        total += v
        if total > 1 << 63:
            raise GoError("time: invalid duration " + orig)
    if neg:
        return -total
    if total > INT64_MAX:
        raise GoError("time: invalid duration " + orig)
    return total


def parse_duration(value):
    """The reference's timing.ParseDuration: an int is seconds, a string
    strconv.Atoi accepts is seconds (parsed as "<n>s"), any other string is
    a Go duration. Returns nanoseconds or raises GoError. Seconds that do
    not fit a Duration are an error (Go would wrap silently)."""
    if isinstance(value, bool) or not isinstance(value, (int, str)):
        raise GoError("unexpected duration of type %s" % type(value).__name__)
    if isinstance(value, int):
        ns = value * 10**9
        if abs(ns) > INT64_MAX:
            raise GoError("duration overflows")
        return ns
    n = atoi(value)
    if n is not None:
        return go_parse_duration("%ds" % n)
    return go_parse_duration(value)


# ------------------------------------------------------------------- regexp

def _expand(repl, match, names):
    """Regexp.Expand for one match."""
    out = []
    i = 0
    ngroups = match.re.groups
    while i < len(repl):
        c = repl[i]
        if c != "$":
            out.append(c)
            i += 1
            continue
        if repl[i + 1:i + 2] == "$":
            out.append("$")
            i += 2
            continue
        k = i + 1
        brace = repl[k:k + 1] == "{"
        if brace:
            k += 1
        start = k
        while k < len(repl) and (repl[k] == "_" or repl[k].isalnum()):
            k += 1
        name = repl[start:k]
        if not name or (brace and repl[k:k + 1] != "}"):
            out.append("$")  # malformed: the '$' is text
            i += 1
            continue
        if brace:
            k += 1
        i = k
        num = -1
        if name.isascii() and name.isdigit() and int(name) < 10**8 and \
                not (name[0] == "0" and len(name) > 1):
            num = int(name)
        elif name in names:
            num = names[name]
        if 0 <= num <= ngroups and match.group(num) is not None:
            out.append(match.group(num))
    return "".join(out)


def regex_replace_all(pattern, repl, s):
    """Go's Regexp.ReplaceAllString(s, repl) for the syntax RE2 and Python
    share. Leftmost-first matches in turn; an empty match that abuts the
    previous match is not replaced; Go's own $-expansion."""
    try:
        rx = re.compile(pattern)
    except re.error as e:
        raise GoError("error parsing regexp: %s" % e)
    names = dict(rx.groupindex)
    out = []
    last_end = 0
    pos = 0
    while pos <= len(s):
        m = rx.search(s, pos)
        if m is None:
            break
        a0, a1 = m.span()
        out.append(s[last_end:a0])
        if a1 > last_end or a0 == 0:
            out.append(_expand(repl, m, names))
        last_end = a1
        pos = a1 if a1 > pos else pos + 1
    out.append(s[last_end:])
    return "".join(out)


# ----------------------------------------------------------------- printing

def format_float(f):
    """fmt's %v of a float64: shortest digits that round-trip; exponent
    form (sign and at least two exponent digits) when the decimal exponent
    is below -4 or at least FLOAT_EXPONENT_THRESHOLD."""
    if f != f:
        return "NaN"
    if f in (float("inf"), float("-inf")):
        return "+Inf" if f > 0 else "-Inf"
    sign, digs, exp = Decimal(repr(f)).as_tuple()
    digits = "".join(map(str, digs)).lstrip("0")
    if not digits:
        return "-0" if sign else "0"
    stripped = digits.rstrip("0")
    exp += len(digits) - len(stripped)
    digits = stripped
    e10 = exp + len(digits) - 1  # exponent of the first digit
    out = "-" if sign else ""
    if e10 < -4 or e10 >= FLOAT_EXPONENT_THRESHOLD:
        out += digits[0]
        if len(digits) > 1:
            out += "." + digits[1:]
        return out + "e%s%02d" % ("-" if e10 < 0 else "+", abs(e10))
    if e10 < 0:
        return out + "0." + "0" * (-e10 - 1) + digits
    if len(digits) <= e10 + 1:
        return out + digits + "0" * (e10 + 1 - len(digits))
    return out + digits[:e10 + 1] + "." + digits[e10 + 1:]


def sprint(v):
    """fmt's %v. None prints empty (the project's data-template rule)."""
    if v is None:
        return ""
    if isinstance(v, str):
        return v
    if isinstance(v, bool):
        return "true" if v else "false"
    if isinstance(v, int):
        return str(v)
    if isinstance(v, float):
        return format_float(v)
    if isinstance(v, list):
        return "[" + " ".join(sprint(e) for e in v) + "]"
    if isinstance(v, dict):
        return "map[" + " ".join(
            "%s:%s" % (k, sprint(v[k])) for k in sorted(v)) + "]"
    raise GoError("unprintable value %r" % (v,))


def go_print(args):
    """fmt.Sprint: a space between operands when neither is a string."""
    out = []
    for i, a in enumerate(args):
        if i > 0 and not isinstance(a, str) and \
                not isinstance(args[i - 1], str):
            out.append(" ")
        out.append(sprint(a))
    return "".join(out)


def go_println(args):
    """fmt.Sprintln: always spaces, and a newline."""
    return " ".join(sprint(a) for a in args) + "\n"


_QUOTE_ESC = {"\a": "\\a", "\b": "\\b", "\f": "\\f", "\n": "\\n",
              "\r": "\\r", "\t": "\\t", "\v": "\\v", '"': '\\"',
              "\\": "\\\\"}


def go_quote(s):
    """strconv.Quote."""
    out = ['"']
    for ch in s:
        cp = ord(ch)
        if ch in _QUOTE_ESC:
            out.append(_QUOTE_ESC[ch])
        elif ch == " " or ch.isprintable():
            out.append(ch)
        elif cp < 0x80:
            out.append("\\x%02x" % cp)
        elif cp < 0x10000:
            out.append("\\u%04x" % cp)
        else:
            out.append("\\U%08x" % cp)
    return "".join(out) + '"'


_VERB = re.compile(r"%([-0]*)([0-9]*)(?:\.([0-9]*))?(.)", re.S)


def go_printf(fmt, args):
    """fmt.Sprintf for %s %v %d %f %q %t %x %% with '-', '0', width and
    .precision. Everything fmt would answer with %!verb(...) is a GoError:
    the engine refuses those instead of printing fmt's complaint."""
    if not isinstance(fmt, str):
        raise GoError("printf format must be a string")
    out = []
    argi = 0
    i = 0
    while i < len(fmt):
        if fmt[i] != "%":
            out.append(fmt[i])
            i += 1
            continue
        m = _VERB.match(fmt, i)
        if not m:
            raise GoError("printf: bad verb")
        flags, width, prec, verb = m.groups()
        i = m.end()
        if verb == "%":
            if m.group(0) != "%%":
                raise GoError("printf: bad %%")
            out.append("%")
            continue
        if verb not in "svdfqtx":
            raise GoError("printf: unsupported verb %" + verb)
        if argi >= len(args):
            raise GoError("printf: missing argument")
        a = args[argi]
        argi += 1
        minus, zero = "-" in flags, "0" in flags
        is_int = isinstance(a, int) and not isinstance(a, bool)
        numeric = verb in "df" or (verb == "x" and is_int)
        if zero and not numeric:
            raise GoError("printf: flag 0 on a non-numeric verb")
        if prec is not None and verb not in "fs":
            raise GoError("printf: precision on %" + verb)
        sign = ""
        if verb == "s":
            if not isinstance(a, str):
                raise GoError("printf: %s of a non-string")
            body = a if prec is None else a[:int(prec or 0)]
        elif verb == "v":
            body = sprint(a)
        elif verb == "q":
            if not isinstance(a, str):
                raise GoError("printf: %q of a non-string")
            body = go_quote(a)
        elif verb == "t":
            if not isinstance(a, bool):
                raise GoError("printf: %t of a non-bool")
            body = "true" if a else "false"
        elif verb == "x" and isinstance(a, str):
            body = a.encode("utf-8", "surrogateescape").hex()
        elif verb in "dx":
            if verb == "d" and isinstance(a, str) and atoi(a) is not None:
                a = atoi(a)  # the engine's pinned leniency
            elif not is_int:
                raise GoError("printf: %" + verb + " of a non-integer")
            sign = "-" if a < 0 else ""
            body = ("%d" if verb == "d" else "%x") % abs(a)
        else:  # f
            if not isinstance(a, float):
                raise GoError("printf: %f of a non-float")
            sign = "-" if str(a).startswith("-") else ""
            body = "%.*f" % (6 if prec is None else int(prec or 0), abs(a))
        pad = max(0, int(width or 0) - len(sign) - len(body))
        if minus:
            out.append(sign + body + " " * pad)
        elif zero:
            out.append(sign + "0" * pad + body)
        else:
            out.append(" " * pad + sign + body)
    if argi < len(args):
        raise GoError("printf: extra arguments")
    return "".join(out)


# ---------------------------------------------------------------- functions

def _want_str(v, what):
    if not isinstance(v, str):
        raise GoError("%s: expected string" % what)
    return v


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _is_num(v):
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def truthy(v):
    """text/template's truth: the zero value of each type is false."""
    if v is None:
        return False
    if isinstance(v, (str, list, dict)):
        return len(v) > 0
    return bool(v)


def _fn_default(args):
    if len(args) != 2:
        raise GoError("default: wrong number of args")
    d, v = args
    if isinstance(v, str) and v != "":
        return v
    return d if isinstance(d, str) else sprint(d)


def _fn_split(args):
    if len(args) != 2:
        raise GoError("split: wrong number of args")
    sep, s = _want_str(args[0], "split"), _want_str(args[1], "split")
    s = s.strip(GO_SPACE)
    if s == "":
        return []
    return list(s) if sep == "" else s.split(sep)


def _fn_join(args):
    if len(args) != 2:
        raise GoError("join: wrong number of args")
    sep = _want_str(args[0], "join")
    if not isinstance(args[1], list):
        raise GoError("join: expected a list")
    return sep.join(_want_str(e, "join") for e in args[1])


def _fn_replace_all(args):
    if len(args) != 3:
        raise GoError("replaceAll: wrong number of args")
    frm, to, s = (_want_str(a, "replaceAll") for a in args)
    if frm == "":
        return to + "".join(ch + to for ch in s)
    return s.replace(frm, to)


def _fn_regex_replace_all(args):
    if len(args) != 3:
        raise GoError("regexReplaceAll: wrong number of args")
    pat, to, s = (_want_str(a, "regexReplaceAll") for a in args)
    return regex_replace_all(pat, to, s)


def _ensure_int(v):
    if _is_int(v):
        return v
    if isinstance(v, str):
        n = atoi(v)
        if n is None:
            raise GoError("loop: invalid syntax")
        return n
    raise GoError("loop: not an int")


def _fn_loop(args):
    if len(args) == 1:
        start, stop = 0, _ensure_int(args[0])
    elif len(args) == 2:
        start, stop = _ensure_int(args[0]), _ensure_int(args[1])
    else:
        raise GoError("loop: wrong number of arguments")
    if abs(stop - start) > 1000000:
        # Go has no limit; the engine refuses rather than exhaust memory
        raise GoError("loop: more than 1000000 elements")
    step = -1 if stop < start else 1
    return list(range(start, stop, step))


def _eq(a, b):
    if _is_num(a) and _is_num(b):
        return float(a) == float(b)
    if isinstance(a, bool) or isinstance(b, bool):
        return truthy(a) == truthy(b)
    return sprint(a) == sprint(b)


def _cmp(a, b):
    if _is_num(a) and _is_num(b):
        a, b = float(a), float(b)
    else:
        a, b = sprint(a).encode(), sprint(b).encode()
    return -1 if a < b else (1 if a > b else 0)


def _fn_len(args):
    if len(args) != 1:
        raise GoError("len: wrong number of args")
    v = args[0]
    if isinstance(v, str):
        return len(v.encode("utf-8", "surrogateescape"))
    if isinstance(v, (list, dict)):
        return len(v)
    raise GoError("len of unsupported type")


def _fn_index(args):
    if len(args) != 2:
        raise GoError("index: wrong number of args")
    c, k = args
    if isinstance(c, dict):
        if not isinstance(k, str):
            raise GoError("index: map key must be a string")
        return c.get(k, "")
    if not isinstance(c, (list, str)):
        raise GoError("index of unsupported type")
    if not _is_int(k):
        raise GoError("index: not an integer")
    if isinstance(c, str):
        c = list(c.encode("utf-8", "surrogateescape"))
    if k < 0 or k >= len(c):
        raise GoError("index out of range")
    return c[k]


def call_function(name, args, env):
    if name == "default":
        return _fn_default(args)
    if name == "env":
        if len(args) != 1:
            raise GoError("env: wrong number of args")
        return env.get(_want_str(args[0], "env"), "")
    if name == "split":
        return _fn_split(args)
    if name == "join":
        return _fn_join(args)
    if name == "replaceAll":
        return _fn_replace_all(args)
    if name == "regexReplaceAll":
        return _fn_regex_replace_all(args)
    if name == "loop":
        return _fn_loop(args)
    if name == "printf":
        if not args:
            raise GoError("printf: no format")
        return go_printf(args[0], args[1:])
    if name == "print":
        return go_print(args)
    if name == "println":
        return go_println(args)
    if name == "len":
        return _fn_len(args)
    if name == "index":
        return _fn_index(args)
    if name == "eq":
        if len(args) < 2:
            raise GoError("eq: wrong number of args")
        return any(_eq(args[0], b) for b in args[1:])
    if name in ("ne", "lt", "le", "gt", "ge"):
        if len(args) != 2:
            raise GoError(name + ": wrong number of args")
        if name == "ne":
            return not _eq(args[0], args[1])
        c = _cmp(args[0], args[1])
        return {"lt": c < 0, "le": c <= 0, "gt": c > 0, "ge": c >= 0}[name]
    if name == "and":
        if not args:
            raise GoError("and: wrong number of args")
        for a in args:
            if not truthy(a):
                return a
        return args[-1]
    if name == "or":
        if not args:
            raise GoError("or: wrong number of args")
        for a in args:
            if truthy(a):
                return a
        return args[-1]
    if name == "not":
        if len(args) != 1:
            raise GoError("not: wrong number of args")
        return not truthy(args[0])
    raise GoError('function "%s" not defined' % name)


# ---------------------------------------------------------------- evaluator

def _field(v, names):
    """.A.B: a missing key and a field of a non-map are both ""."""
    for n in names:
        v = v.get(n, "") if isinstance(v, dict) else ""
    return v


class _Eval:
    def __init__(self, root, env):
        self.env = env
        self.vars = [("", root)]  # Go's variable stack
        self.out = []

    def lookup(self, name):
        for n, v in reversed(self.vars):
            if n == name:
                return v
        raise GoError("undefined variable $" + name)

    def expr(self, e, dot):
        kind = e[0]
        if kind in ("str", "int", "float", "bool"):
            return e[1]
        if kind == "dot":
            return dot
        if kind == "field":
            return _field(dot, e[1])
        if kind == "var":
            return _field(self.lookup(e[1]), e[2])
        if kind == "call":
            return call_function(
                e[1], [self.expr(a, dot) for a in e[2]], self.env)
        if kind == "pipe":
            v = self.expr(e[1], dot)
            for _, fname, args in e[2]:
                v = call_function(
                    fname, [self.expr(a, dot) for a in args] + [v], self.env)
            return v
        raise GoError("unknown expression %r" % (e,))

    def nodes(self, nodes, dot):
        for n in nodes:
            kind = n[0]
            if kind == "text":
                self.out.append(n[1])
            elif kind == "comment":
                pass
            elif kind == "action":
                self.out.append(sprint(self.expr(n[1], dot)))
            elif kind == "assign":
                self.vars.append((n[1], self.expr(n[2], dot)))
            elif kind in ("if", "with"):
                self.if_or_with(n, dot)
            elif kind == "range":
                self.range(n, dot)
            else:
                raise GoError("unknown node %r" % (n,))

    def else_(self, else_, dot):
        if else_ is None:
            return
        if isinstance(else_, tuple):  # {{else if}}
            else_ = [else_]
        self.nodes(else_, dot)

    def if_or_with(self, n, dot):
        _, decl, e, body, else_ = n
        mark = len(self.vars)
        v = self.expr(e, dot)
        if decl is not None:
            self.vars.append((decl, v))
        if truthy(v):
            self.nodes(body, v if n[0] == "with" else dot)
        else:
            self.else_(else_, dot)
        del self.vars[mark:]

    def range(self, n, dot):
        _, decls, e, body, else_ = n
        mark = len(self.vars)
        coll = self.expr(e, dot)
        if coll is not None and not isinstance(coll, list):
            raise GoError("range over non-list value")
        for d in decls:
            self.vars.append((d, coll))
        inner = len(self.vars)
        if coll:
            for i, item in enumerate(coll):
                if len(decls) >= 1:
                    self.vars[inner - 1] = (decls[-1], item)
                if len(decls) >= 2:
                    self.vars[inner - 2] = (decls[0], i)
                self.nodes(body, item)
                del self.vars[inner:]
        else:
            self.else_(else_, dot)
        del self.vars[mark:]


def evaluate(nodes, root, env=None):
    """What Go prints for the AST `nodes` with "." and "$" starting as
    `root` (the environment map, or a JSON document). `env` is what the
    `env` function reads; it defaults to `root` for an environment root."""
    if env is None:
        env = root if isinstance(root, dict) else {}
    ev = _Eval(root, env)
    ev.nodes(nodes, root)
    return "".join(ev.out)


def ast_from_json(nodes):
    """The AST from its JSON form (lists instead of tuples), as the rows of
    tests/golden/template_cases.json carry it."""
    def expr(e):
        kind = e[0]
        if kind in ("str", "int", "float", "bool"):
            return (kind, e[1])
        if kind == "dot":
            return ("dot",)
        if kind == "field":
            return ("field", list(e[1]))
        if kind == "var":
            return ("var", e[1], list(e[2]))
        if kind == "call":
            return ("call", e[1], [expr(a) for a in e[2]])
        if kind == "pipe":
            return ("pipe", expr(e[1]),
                    [("call", c[1], [expr(a) for a in c[2]]) for c in e[2]])
        raise ValueError("unknown expression %r" % (e,))

    def else_(x):
        if x is None:
            return None
        if x and isinstance(x[0], str):
            return node(x)  # {{else if}}
        return [node(n) for n in x]

    def node(n):
        kind = n[0]
        if kind in ("text", "comment"):
            return (kind, n[1])
        if kind == "action":
            return ("action", expr(n[1]))
        if kind == "assign":
            return ("assign", n[1], expr(n[2]))
        if kind in ("if", "with"):
            return (kind, n[1], expr(n[2]), [node(b) for b in n[3]],
                    else_(n[4]))
        if kind == "range":
            return (kind, list(n[1]), expr(n[2]), [node(b) for b in n[3]],
                    else_(n[4]))
        raise ValueError("unknown node %r" % (n,))

    return [node(n) for n in nodes]


# --------------------------------------------------------------- serialiser

def _quote_string(s, rng):
    """A Go string literal for s: `raw` when possible and chosen, else
    "interpreted" with a seeded choice of escapes."""
    if "`" not in s and "\r" not in s and rng.random() < 0.3:
        return "`" + s + "`"
    out = ['"']
    for ch in s:
        cp = ord(ch)
        if ch == '"':
            out.append('\\"')
        elif ch == "\\":
            out.append("\\\\")
        elif ch == "\n":
            out.append("\\n")
        elif ch == "\t":
            out.append(rng.choice(["\\t", "\t"]))
        elif ch == "\r":
            out.append("\\r")
        elif cp < 0x20 or cp == 0x7f:
            out.append("\\x%02x" % cp)
        elif cp < 0x80 and rng.random() < 0.05:
            out.append("\\x%02x" % cp)
        elif 0x80 <= cp < 0x10000 and rng.random() < 0.3:
            out.append("\\u%04x" % cp)
        elif cp >= 0x10000 and rng.random() < 0.3:
            out.append("\\U%08x" % cp)
        else:
            out.append(ch)
    return "".join(out) + '"'


def _float_literal(f):
    text = repr(f)
    if text in ("inf", "-inf", "nan"):
        raise ValueError("no literal for %r" % f)
    # Go reads a constant as a float only if its text has '.', 'e' or 'E'
    return text


def _expr_text(e, rng, top=False):
    kind = e[0]
    if kind == "str":
        return _quote_string(e[1], rng)
    if kind == "int":
        if e[1] >= 0 and rng.random() < 0.15:
            return "0x%x" % e[1]
        return str(e[1])
    if kind == "float":
        return _float_literal(e[1])
    if kind == "bool":
        return "true" if e[1] else "false"
    if kind == "dot":
        return "."
    if kind == "field":
        return "".join("." + n for n in e[1])
    if kind == "var":
        return "$" + e[1] + "".join("." + n for n in e[2])
    if kind == "call":
        text = " ".join([e[1]] + [_expr_text(a, rng) for a in e[2]])
    elif kind == "pipe":
        sep = rng.choice([" | ", "|", " |  "])
        text = sep.join(
            [_expr_text(e[1], rng, top=True)] +
            [" ".join([c[1]] + [_expr_text(a, rng) for a in c[2]])
             for c in e[2]])
    else:
        raise ValueError("unknown expression %r" % (e,))
    if top and rng.random() < 0.85:
        return text
    return "(" + text + ")"


def serialize(nodes, rng):
    """Template text for the AST, and the AST as Go will see it.

    `rng` (a random.Random) picks the layout: spaces inside the delimiters,
    {{- and -}} trim markers, "..." or `...` strings and their escapes.
    Trim markers eat the adjacent text, so the second return value is the
    AST with its text nodes trimmed the same way; evaluate that one."""
    items = []  # ["text", s] or ["action", body, trim_left, trim_right]

    def action(body):
        items.append(["action", body,
                      rng.random() < 0.2, rng.random() < 0.2])

    def decl_text(decls):
        return ", ".join("$" + d for d in decls) + " := " if decls else ""

    def walk(nodes):
        out = []
        for n in nodes:
            kind = n[0]
            if kind == "text":
                item = ["text", n[1]]
                items.append(item)
                out.append(item)
            elif kind == "comment":
                items.append(["comment", "/*" + n[1] + "*/",
                              rng.random() < 0.2, rng.random() < 0.2])
                out.append(n)
            elif kind == "action":
                action(_expr_text(n[1], rng, top=True))
                out.append(n)
            elif kind == "assign":
                action("$%s := %s" % (n[1], _expr_text(n[2], rng, top=True)))
                out.append(n)
            else:
                out.append(control(n, kind))
        return out

    def control(n, keyword):
        _, decl, e, body, else_ = n
        decls = decl if keyword == "range" else ([decl] if decl else [])
        action("%s %s%s" % (keyword, decl_text(decls),
                            _expr_text(e, rng, top=True)))
        return finish(n, body, else_)

    def finish(n, body, else_):
        new_body = walk(body)
        if else_ is None:
            new_else = None
        elif isinstance(else_, tuple):
            _, decl, e, body2, else2 = else_
            action("else if %s%s" % (decl_text([decl] if decl else []),
                                     _expr_text(e, rng, top=True)))
            new_else = finish(else_, body2, else2)
            return (n[0], n[1], n[2], new_body, new_else)
        else:
            action("else")
            new_else = walk(else_)
        action("end")
        return (n[0], n[1], n[2], new_body, new_else)

    def finish_top(nodes):
        return walk(nodes)

    tree = finish_top(nodes)

    # trim markers eat the neighbouring text, across node boundaries
    for idx, item in enumerate(items):
        if item[0] == "text":
            continue
        if item[2]:
            k = idx - 1
            while k >= 0 and items[k][0] == "text":
                items[k][1] = items[k][1].rstrip(TRIM_CHARS)
                if items[k][1]:
                    break
                k -= 1
        if item[3]:
            k = idx + 1
            while k < len(items) and items[k][0] == "text":
                items[k][1] = items[k][1].lstrip(TRIM_CHARS)
                if items[k][1]:
                    break
                k += 1

    parts = []
    for item in items:
        if item[0] == "text":
            parts.append(item[1])
        elif item[0] == "comment":
            parts.append(("{{- " if item[2] else "{{") + item[1] +
                         (" -}}" if item[3] else "}}"))
        else:
            pad_l = rng.choice(["", " ", "  ", "\t"])
            pad_r = rng.choice(["", " ", "  ", "\t"])
            parts.append(("{{- " if item[2] else "{{") + pad_l + item[1] +
                         pad_r + (" -}}" if item[3] else "}}"))

    def freeze(nodes):
        out = []
        for n in nodes:
            if isinstance(n, list):  # a text item, now trimmed
                out.append(("text", n[1]))
            elif n[0] in ("if", "with", "range"):
                out.append(freeze_control(n))
            else:
                out.append(n)
        return out

    def freeze_control(n):
        else_ = n[4]
        if isinstance(else_, tuple):
            else_ = freeze_control(else_)
        elif else_ is not None:
            else_ = freeze(else_)
        return (n[0], n[1], n[2], freeze(n[3]), else_)

    return "".join(parts), freeze(tree)
