"""The template engine against a model of Go's semantics.

Two tiers. A hand-written table (tests/golden/template_cases.json) states
what Go 1.9 does for one template each, with the rule it rests on. Then
properties generate template ASTs, serialise them in varying layouts, and
compare the native engine with containerpilot_amd.gomodel evaluating the
same AST, for the environment root and for a JSON data root; likewise for
regexReplaceAll and for float printing.
"""

import json
import os
import random

import pytest
from hypothesis import given, settings, strategies as st

from containerpilot_amd import gomodel, native

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "template_cases.json"),
          encoding="utf-8") as f:
    CASES = json.load(f)

# environment names the table and the generators use; anything not set by a
# row is unset while it runs
ENV_NAMES = ["FOO", "MISSING", "TEST_NAME", "TEST_PARTS", "TEST_MISSING",
             "COUNT", "STAGE", "GM_A", "GM_B", "GM_N", "GM_MISSING"]


class _Env:
    """Sets exactly `env` among ENV_NAMES for the duration of a block."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.saved = {n: os.environ.get(n) for n in ENV_NAMES}
        for n in ENV_NAMES:
            if n in self.env:
                os.environ[n] = self.env[n]
            else:
                os.environ.pop(n, None)

    def __exit__(self, *exc):
        for n, v in self.saved.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v


def render_native(template, env, data=None):
    """("ok", text) or ("error", message) from the native engine."""
    with _Env(env):
        try:
            if data is None:
                return ("ok", native.render_template(template))
            return ("ok", native.render_data(template, json.dumps(data)))
        except ValueError as e:
            return ("error", str(e))


def _outcome(result):
    """Errors compare as errors: the engine and the model word them apart."""
    return result if result[0] == "ok" else ("error",)


def render_model(ast, env, data=None):
    try:
        root = dict(env) if data is None else data
        return ("ok", gomodel.evaluate(ast, root, env=env))
    except gomodel.GoError as e:
        return ("error", str(e))


# ------------------------------------------------------------------ the table

def _case_id(case):
    return "%s:%s" % (case["class"], case["template"][:40])


def test_table_is_well_formed():
    assert len(CASES) > 200
    for case in CASES:
        assert case["class"] in ("parity", "must-error", "leniency"), case
        assert case["rule"].strip(), case
        assert ("expect" in case) != (case.get("error") is True), case
        if case["class"] == "must-error":
            assert case.get("error") is True, case
        else:
            assert "expect" in case, case
        assert set(case["env"]) <= set(ENV_NAMES), case


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_table_row(case):
    data = case.get("data")
    got = render_native(case["template"], case["env"], data)
    print(case["rule"], "->", got)
    if case.get("error"):
        assert got[0] == "error", (case["rule"], got)
        # where the rule is "an error that names the construct"
        assert case.get("error_names", "") in got[1], (case["rule"], got)
    else:
        assert got == ("ok", case["expect"]), case["rule"]
    if data is None:
        # the environment as a data document is the same root
        again = render_native(case["template"], case["env"], case["env"])
        assert again[0] == got[0] and (got[0] == "error" or again == got), \
            (case["rule"], again)


PARITY_WITH_AST = [c for c in CASES if c["class"] == "parity" and "ast" in c]


def test_most_parity_rows_have_an_ast():
    parity = [c for c in CASES if c["class"] == "parity"]
    assert len(PARITY_WITH_AST) * 10 >= len(parity) * 8


@pytest.mark.parametrize("case", PARITY_WITH_AST, ids=_case_id)
def test_table_row_in_the_model(case):
    ast = gomodel.ast_from_json(case["ast"])
    assert render_model(ast, case["env"], case.get("data")) == \
        ("ok", case["expect"]), case["rule"]
    # and its serialisations, in a few layouts, render the same natively
    for seed in range(3):
        text, trimmed = gomodel.serialize(ast, random.Random(seed))
        want = render_model(trimmed, case["env"], case.get("data"))
        got = render_native(text, case["env"], case.get("data"))
        assert _outcome(got) == _outcome(want), (text, case["rule"])


# ------------------------------------------------------- generated templates

TEXT_ALPHABET = list("ab1,: \n\t-}\"\\`é日$")
texts = st.text(alphabet=st.sampled_from(TEXT_ALPHABET), max_size=4)
# text between actions: no '{', so that it never opens an action
plain = st.text(alphabet=st.sampled_from(list("ab \n\t\r\v }-é")),
                max_size=4)
small_ints = st.integers(min_value=-3, max_value=12)
loop_bounds = st.integers(min_value=-2, max_value=2)  # at most 4 elements
nice_floats = st.one_of(
    st.sampled_from([0.0, -0.0, 0.5, 1.5, 100.0, 1e20, 1e21, 1e-4, 1e-5,
                     3.14159265, 123456789.125, 2.5e-7]),
    st.floats(allow_nan=False, allow_infinity=False, width=64))

REGEX_ARGS = [("[ab]+", "_"), ("(a)(b)?", "<$2$1>"), ("x*", "-"),
              (".", "${0}${0}"), ("(?i)A", "$$"), ("(?P<n>[a-b])", "${n}$n!"),
              ("", "|"), ("a|ab", "$1x")]
PRINTF_FORMATS = [("%s", ["str"]), ("%v|%v", ["any", "any"]),
                  ("%d", ["int"]), ("%03d|%-4d|", ["int", "int"]),
                  ("%f", ["float"]), ("%6.2f|%-8.3f|%08.1f", ["float"] * 3),
                  ("%q", ["str"]), ("%5q|%-5s|%.2s", ["str"] * 3),
                  ("%t", ["bool"]), ("%x|%04x", ["int", "int"]),
                  ("%x", ["str"]), ("100%%", [])]

SCALARS = ["str", "int", "float", "bool"]
ELEM = {"lstr": "str", "lint": "int"}


class Ctx:
    """What an expression may refer to at one point of a template."""

    def __init__(self, root_fields):
        self.root = root_fields    # field path (tuple) -> type, via "$"
        self.fields = root_fields  # the same for the current dot
        self.dot = None            # type of the dot when it is no map
        self.vars = {}             # name -> type

    def child(self):
        c = Ctx(self.root)
        c.fields, c.dot, c.vars = self.fields, self.dot, dict(self.vars)
        return c

    def with_dot(self, dot_type):
        c = self.child()
        if isinstance(dot_type, dict):
            c.fields, c.dot = dot_type, None
        else:
            c.fields, c.dot = {}, dot_type
        return c


class Gen:
    """Draws typed expressions and node lists; only in-scope variables and
    fields are referred to, and arguments have the types functions take."""

    def __init__(self, draw):
        self.draw = draw

    def pick(self, options):
        return self.draw(st.sampled_from(options))

    def chance(self, percent):
        return self.draw(st.integers(0, 99)) < percent

    def literal(self, t):
        if t == "str":
            return ("str", self.draw(texts))
        if t == "int":
            return ("int", self.draw(small_ints))
        if t == "float":
            return ("float", self.draw(nice_floats))
        if t == "bool":
            return ("bool", self.draw(st.booleans()))
        if t == "lstr":
            return ("call", "split", [("str", ","), ("str", self.draw(texts))])
        if t == "lint":
            return ("call", "loop", [("int", self.draw(loop_bounds)),
                                     ("int", self.draw(loop_bounds))])
        raise AssertionError(t)

    def leaf(self, t, ctx):
        options = [self.literal(t)]
        if ctx.dot == t:
            options.append(("dot",))
        for path, ft in ctx.fields.items():
            if ft == t:
                options.append(("field", list(path)))
        for path, ft in ctx.root.items():
            if ft == t:
                options.append(("var", "", list(path)))
        for name, vt in ctx.vars.items():
            if vt == t:
                options.append(("var", name, []))
            elif isinstance(vt, dict):
                for path, ft in vt.items():
                    if ft == t:
                        options.append(("var", name, list(path)))
        return self.pick(options)

    def piped(self, fname, args):
        if args and self.chance(30):
            return ("pipe", args[-1], [("call", fname, args[:-1])])
        return ("call", fname, args)

    def expr(self, t, ctx, depth):
        if t == "any":
            t = self.pick(SCALARS + ["lstr", "lint"])
        if depth <= 0 or self.chance(35):
            return self.leaf(t, ctx)
        d = depth - 1
        if t == "str":
            kind = self.pick(["default", "join", "replaceAll", "regex",
                              "print", "println", "printf", "env", "or"])
            if kind == "default":
                dt = self.pick(SCALARS)
                return self.piped("default", [self.literal(dt),
                                              self.expr("str", ctx, d)])
            if kind == "join":
                return self.piped("join", [("str", self.pick([",", "", "é"])),
                                           self.expr("lstr", ctx, d)])
            if kind == "replaceAll":
                return self.piped("replaceAll", [
                    ("str", self.pick(["", "a", ",", "é", "ab"])),
                    ("str", self.draw(texts)), self.expr("str", ctx, d)])
            if kind == "regex":
                pat, repl = self.pick(REGEX_ARGS)
                return self.piped("regexReplaceAll", [
                    ("str", pat), ("str", repl), self.expr("str", ctx, d)])
            if kind in ("print", "println"):
                n = self.draw(st.integers(0, 3))
                return ("call", kind, [self.expr("any", ctx, d)
                                       for _ in range(n)])
            if kind == "printf":
                fmt, types = self.pick(PRINTF_FORMATS)
                return ("call", "printf", [("str", fmt)] + [
                    self.expr(at, ctx, d) for at in types])
            if kind == "env":
                return ("call", "env", [("str", self.pick(
                    ["GM_A", "GM_B", "GM_MISSING"]))])
            return ("call", "or", [self.expr("str", ctx, d),
                                   self.expr("str", ctx, d)])
        if t == "int":
            kind = self.pick(["len", "index", "and"])
            if kind == "len":
                return self.piped("len", [self.expr(
                    self.pick(["str", "lstr", "lint"]), ctx, d)])
            if kind == "index":
                return ("call", "index", [
                    ("call", "loop", [("int", 2), ("int", 6)]),
                    ("int", self.draw(st.integers(0, 3)))])
            return ("call", "and", [self.expr("int", ctx, d),
                                    self.expr("int", ctx, d)])
        if t == "bool":
            kind = self.pick(["cmp", "not", "and"])
            if kind == "cmp":
                at = self.pick(["str", "int"])
                return ("call", self.pick(["eq", "ne", "lt", "le", "gt", "ge"]),
                        [self.expr(at, ctx, d), self.expr(at, ctx, d)])
            if kind == "not":
                return self.piped("not", [self.expr("any", ctx, d)])
            return ("call", self.pick(["and", "or"]),
                    [self.expr("bool", ctx, d), self.expr("bool", ctx, d)])
        if t == "lstr":
            return self.piped("split", [
                ("str", self.pick([",", "", ":", "é"])),
                self.expr("str", ctx, d)])
        if t == "lint":
            if self.chance(50):
                return ("call", "loop", [self.expr("int", ctx, d)])
            return self.literal("lint")
        return self.leaf(t, ctx)

    def typed_expr(self, ctx):
        """(type, expr) of something a header or an assignment may hold."""
        options = SCALARS + ["lstr", "lint"]
        maps = [(p, ft) for p, ft in ctx.fields.items() if isinstance(ft, dict)]
        if maps and self.chance(25):
            path, ft = self.pick(maps)
            return ft, ("field", list(path))
        t = self.pick(options)
        return t, self.expr(t, ctx, 2)

    def block(self, ctx, depth):
        nodes = []
        ctx = ctx.child()
        for _ in range(self.draw(st.integers(0, max(1, 4 - depth)))):
            kind = self.pick(["text", "text", "action", "action", "assign",
                              "comment", "if", "with", "range"])
            if kind in ("if", "with", "range") and depth >= 4:
                kind = "action"
            if kind == "text":
                nodes.append(("text", self.draw(plain)))
            elif kind == "comment":
                nodes.append(("comment", self.pick(["", " c ", " }} "])))
            elif kind == "action":
                nodes.append(("action", self.expr("any", ctx, 2)))
            elif kind == "assign":
                name = self.pick(["x", "y"])
                t, e = self.typed_expr(ctx)
                nodes.append(("assign", name, e))
                ctx.vars[name] = t
            elif kind == "if":
                nodes.append(self.if_node(ctx, depth))
            elif kind == "with":
                t, e = self.typed_expr(ctx)
                decl = self.pick([None, "x", "w"])
                inner = ctx.with_dot(t)
                outer = ctx.child()
                if decl:
                    inner.vars[decl] = t
                    outer.vars[decl] = t
                nodes.append(("with", decl, e, self.block(inner, depth + 1),
                              self.else_block(outer, depth)))
            else:
                nodes.append(self.range_node(ctx, depth))
        return nodes

    def else_block(self, ctx, depth):
        return self.block(ctx, depth + 1) if self.chance(50) else None

    def if_node(self, ctx, depth):
        t, e = self.typed_expr(ctx)
        decl = self.pick([None, None, "x", "c"])
        inner = ctx.child()
        if decl:
            inner.vars[decl] = t
        body = self.block(inner, depth + 1)
        choice = self.pick(["none", "else", "elif"])
        if choice == "none":
            else_ = None
        elif choice == "else" or depth >= 3:
            else_ = self.block(inner, depth + 1)
        else:
            else_ = self.if_node(inner, depth + 1)
        return ("if", decl, e, body, else_)

    def range_node(self, ctx, depth):
        lists = [(p, ft) for p, ft in ctx.fields.items()
                 if isinstance(ft, list)]
        if lists and self.chance(40):
            path, ft = self.pick(lists)
            elem, e = ft[0], ("field", list(path))
        else:
            lt = self.pick(["lstr", "lint"])
            elem, e = ELEM[lt], self.expr(lt, ctx, 2)
        decls = self.pick([[], ["v"], ["i", "v"], ["x"]])
        inner = ctx.with_dot(elem)
        outer = ctx.child()
        if decls:
            inner.vars[decls[-1]] = elem
            if len(decls) == 2:
                inner.vars[decls[0]] = "int"
            # in {{else}} the variables hold the (empty) collection: print
            # them, do not compute with them
            for d in decls:
                outer.vars.pop(d, None)
        return ("range", decls, e, self.block(inner, depth + 1),
                self.else_block(outer, depth))


ENV_FIELDS = {("GM_A",): "str", ("GM_B",): "str", ("GM_N",): "str",
              ("GM_MISSING",): "str"}
ITEM = {("H",): "str", ("P",): "int"}
SUB = {("K",): "str", ("N",): "int"}
DATA_FIELDS = {("S",): "str", ("T",): "str", ("N",): "int", ("F",): "float",
               ("B",): "bool", ("Nope",): "str", ("M", "K"): "str",
               ("M", "N"): "int", ("M", "Nope", "X"): "str", ("S", "X"): "str",
               ("L",): "lstr", ("M",): SUB, ("LM",): [ITEM]}


@st.composite
def env_programs(draw):
    env = {"GM_A": draw(texts), "GM_B": draw(texts),
           "GM_N": str(draw(small_ints))}
    env = {k: v for k, v in env.items() if "\x00" not in v}
    nodes = Gen(draw).block(Ctx(ENV_FIELDS), 1)
    return env, nodes, draw(st.integers(0, 2**32))


@st.composite
def data_programs(draw):
    ints = st.integers(min_value=-(2**53), max_value=2**53)
    data = {
        "S": draw(texts), "T": draw(texts), "N": draw(ints),
        "F": draw(nice_floats), "B": draw(st.booleans()), "Z": None,
        "L": draw(st.lists(texts, max_size=4)),
        "M": {"K": draw(texts), "N": draw(ints)},
        "LM": draw(st.lists(st.fixed_dictionaries(
            {"H": texts, "P": small_ints}), max_size=4)),
    }
    nodes = Gen(draw).block(Ctx(DATA_FIELDS), 1)
    return data, nodes, draw(st.integers(0, 2**32))


@settings(max_examples=400, deadline=None, derandomize=True)
@given(env_programs())
def test_generated_templates_on_the_environment(program):
    env, nodes, seed = program
    text, trimmed = gomodel.serialize(nodes, random.Random(seed))
    assert _outcome(render_native(text, env)) == \
        _outcome(render_model(trimmed, env)), text


@settings(max_examples=400, deadline=None, derandomize=True)
@given(data_programs())
def test_generated_templates_on_data(program):
    data, nodes, seed = program
    env = {"GM_A": "from-env"}
    text, trimmed = gomodel.serialize(nodes, random.Random(seed))
    assert _outcome(render_native(text, env, data)) == \
        _outcome(render_model(trimmed, env, data)), (text, data)


# ------------------------------------------------------------ regexReplaceAll

@st.composite
def regexes(draw):
    """(pattern, nullable) over literals, classes, '.', * + ?, |, groups,
    named groups. A group that can match the empty string is not repeated:
    engines disagree about its captures."""
    icase = draw(st.booleans())
    literals = ["a", "b", "c", "A"] + ([] if icase else ["é", "日"])
    names = iter(["n", "m", "k2", "_g"])

    def atom(depth):
        kind = draw(st.sampled_from(
            ["lit", "lit", "class", "dot", "group", "named", "nocap"]
            if depth < 2 else ["lit", "class", "dot"]))
        if kind == "lit":
            return draw(st.sampled_from(literals)), False
        if kind == "class":
            return draw(st.sampled_from(
                ["[ab]", "[^a]", "[a-c]", "[^b-c]", "[]a]"] +
                ([] if icase else ["[é日]", "[^é]"]))), False
        if kind == "dot":
            return ".", False
        inner, nullable = alt(depth + 1)
        if kind == "named":
            name = next(names, None)
            if name is not None:
                return "(?P<%s>%s)" % (name, inner), nullable
        if kind == "nocap":
            return "(?:%s)" % inner, nullable
        return "(%s)" % inner, nullable

    def piece(depth):
        text, nullable = atom(depth)
        is_group = text.startswith("(")
        quant = draw(st.sampled_from(["", "", "*", "+", "?"]))
        if quant and is_group and nullable:
            quant = ""
        return text + quant, nullable or quant in ("*", "?")

    def concat(depth):
        parts = [piece(depth) for _ in range(draw(st.integers(0, 3)))]
        return "".join(p for p, _ in parts), all(n for _, n in parts)

    def alt(depth):
        branches = [concat(depth) for _ in range(draw(st.integers(1, 2)))]
        return "|".join(b for b, _ in branches), any(n for _, n in branches)

    pattern, _ = alt(0)
    return ("(?i)" if icase else "") + pattern


# made of '$', '{', '}', digits, letters and '&': references that hit,
# references that miss, and malformed ones
replacements = st.lists(st.sampled_from(
    ["$1", "$2", "${1}", "${2}", "$0", "${n}", "$n", "$m", "${k2}", "$_g",
     "$$", "$", "${", "}", "{", "&", "$&", "x", "a", "0", "9", "$01", "${n",
     "$1x", "${1}x", "$9", "${}", "$nm"]), max_size=5).map("".join)
subjects = st.text(alphabet=st.sampled_from(list("abcABé日 \n")), max_size=8)


def go_string(s):
    return "`" + s + "`"


@settings(max_examples=500, deadline=None, derandomize=True)
@given(regexes(), replacements, subjects)
def test_regex_replace_all_matches_the_model(pattern, repl, subject):
    template = "{{ regexReplaceAll %s %s %s }}" % (
        go_string(pattern), go_string(repl), go_string(subject))
    want = gomodel.regex_replace_all(pattern, repl, subject)
    assert render_native(template, {}) == ("ok", want), template


# ------------------------------------------------------------ float printing

@settings(max_examples=400, deadline=None, derandomize=True)
@given(st.floats(allow_nan=False, allow_infinity=False, width=64))
def test_float_printing_matches_the_model(f):
    want = gomodel.format_float(f)
    literal = repr(f)
    assert render_native("{{ %s }}" % literal, {}) == ("ok", want), literal
    assert render_native("{{ .F }}|{{ index .L 0 }}", {},
                          {"F": f, "L": [f]}) == ("ok", want + "|" + want)
    assert float(want.replace("+Inf", "inf")) == f


def test_float_printing_edges():
    for f, want in [(1e20, "100000000000000000000"), (1e21, "1e+21"),
                    (123456789.0, "123456789"), (0.0001, "0.0001"),
                    (0.00001, "1e-05"), (-0.0, "-0"), (5e-324, "5e-324"),
                    (1.7976931348623157e308, "1.7976931348623157e+308"),
                    (0.1 + 0.2, "0.30000000000000004"), (100.0, "100")]:
        assert gomodel.format_float(f) == want
        assert render_native("{{ %r }}" % f, {}) == ("ok", want)
