"""Differential test of sensor extraction: a small pure-Python model of the
documented rules against native.sensor_extract on generated bodies and
records. Equal means the same float bit for bit, or the same reason
string.

The model works on bytes. White space is the C locale's (space, \\t, \\n,
\\v, \\f, \\r); lines end at \\n and a final piece without one is a line;
a number is what strtod accepts whole (decimal, hex float, no
underscores) and must be finite. Bodies for `json` records are either
valid JSON (json.dumps of generated values) or one of two malformations
whose parser message is fixed: nothing but white space, and trailing
text after the document.
"""

import json
import math
import random
import re
import struct

import pytest

from containerpilot_amd import native

SPACE = b" \t\n\v\f\r"
DEC = re.compile(rb"[+-]?(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?\Z")
HEX = re.compile(rb"[+-]?0[xX]([0-9a-fA-F]+\.?[0-9a-fA-F]*|\.[0-9a-fA-F]+)"
                 rb"([pP][+-]?\d+)?\Z")
MAX_QUOTED = 64


class Reason(Exception):
    pass


def show(token):
    shown = token[:MAX_QUOTED].replace(b"\0", b"\\0")  # NUL shown as \0
    shown += b"..." if len(token) > MAX_QUOTED else b""
    return 'not a number: "%s"' % shown.decode(errors="replace")


def number(token):
    """The finite float of a trimmed token, or None."""
    t = token.strip(SPACE)
    try:
        if DEC.match(t):
            v = float(t)
        elif HEX.match(t):
            v = float.fromhex(t.decode())
        else:
            return None
    except (ValueError, OverflowError):
        return None
    return v if math.isfinite(v) else None


def lines_of(body):
    lines = body.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def unescape(ptr):
    return [t.replace("~1", "/").replace("~0", "~")
            for t in ptr.split("/")[1:]]


def model_json(body, ptr):
    if not body.strip(SPACE):
        raise Reason("json: unexpected end of input")
    try:
        doc = json.loads(body)
    except ValueError:
        raise Reason("json: unexpected trailing characters")
    cur = doc
    for tok in unescape(ptr):
        if isinstance(cur, dict) and tok in cur:
            cur = cur[tok]
        elif (isinstance(cur, list) and re.fullmatch(r"0|[1-9][0-9]{0,17}", tok)
              and int(tok) < len(cur)):
            cur = cur[int(tok)]
        else:
            raise Reason("json: no value at " + ptr)
    if isinstance(cur, bool):
        raise Reason(show(b"bool"))
    if isinstance(cur, (int, float)):
        return float(cur)
    if isinstance(cur, str):
        v = number(cur.encode())
        if v is None:
            raise Reason(show(cur.encode()))
        return v
    raise Reason(show({type(None): b"null", list: b"array",
                       dict: b"object"}[type(cur)]))


def model(body, rec):
    if "json" in rec:
        value = model_json(body, rec["json"])
    elif "line" in rec or "lineNumber" in rec:
        lines = lines_of(body)
        if "line" in rec:
            prefix = rec["line"].encode()
            hits = [l for l in lines if l.lstrip(SPACE).startswith(prefix)]
            if not hits:
                raise Reason('no line starts with "%s"' % rec["line"])
            line = hits[0]
        else:
            if rec["lineNumber"] > len(lines):
                raise Reason("no line %d" % rec["lineNumber"])
            line = lines[rec["lineNumber"] - 1]
        tokens = line.split()
        # bytes.split() without arguments splits on exactly SPACE
        field = rec.get("field", 1)
        if field > len(tokens):
            raise Reason("line has %d fields" % len(tokens))
        value = number(tokens[field - 1])
        if value is None:
            raise Reason(show(tokens[field - 1]))
    else:
        value = number(body)
        if value is None:
            raise Reason(show(body.strip(SPACE)))
    value *= rec.get("scale", 1)
    if not math.isfinite(value):
        raise Reason("value out of range")
    return value


# ---------------- generators ----------------

NUMBERS = [b"0", b"-0", b"7", b"+12", b"16630948", b"1.5", b".5", b"5.",
           b"-1.25e3", b"1E-3", b"0x10", b"0X1.8p3", b"-0x.8p1", b"1e308",
           b"9007199254740993", b"0.1", b"123456789012345678901234567890",
           b"4.9e-324", b"1e-400"]
JUNK = [b"kB", b"nan", b"NaN", b"inf", b"-inf", b"Infinity", b"1e999", b"12x",
        b"1_000", b"0x", b"--1", b"1,5", b"\xc3\xa9t\xc3\xa9", b"\xff\xfe",
        b"1\x002", b"e5", b".", b"+", b"0x1p", b"MemFree:", b"\xe2\x82\xac9",
        b"x" * 70]
KEYS = [b"MemTotal:", b"MemAvailable:", b"Active", b"cpu", b"key", b"k\xc3\xa9y",
        b"7", b"Reading:"]
GAPS = [b" ", b"  ", b"\t", b" \t ", b"\v", b"\f"]
EOLS = [b"\n", b"\n", b"\r\n"]
SCALES = [None, 1024, 0.5, -1, 1e-6, 1e300, 0]


def gen_token(rng):
    return rng.choice(NUMBERS if rng.random() < 0.7 else JUNK)


def gen_line(rng):
    kind = rng.random()
    if kind < 0.15:
        return rng.choice([b"", b" ", b"\t"])
    parts = []
    if kind < 0.75:
        parts.append(rng.choice(KEYS))
    for _ in range(rng.randrange(0, 4)):
        parts.append(gen_token(rng))
    line = rng.choice([b"", b"", b" ", b"\t "])
    for p in parts:
        line += p + rng.choice(GAPS)
    return line if rng.random() < 0.5 else line.rstrip(SPACE)


def gen_text_body(rng):
    if rng.random() < 0.1:
        return rng.choice([b"", b"\n", b" \r\n", b"\n\n"])
    body = b""
    n = rng.randrange(1, 7)
    for i in range(n):
        body += gen_line(rng)
        if i < n - 1 or rng.random() < 0.7:
            body += rng.choice(EOLS)
    return body


def gen_whole_body(rng):
    pad = [b"", b"", b" ", b"\n", b"\r\n", b"\t"]
    mid = gen_token(rng)
    if rng.random() < 0.1:
        mid += b" " + gen_token(rng)
    return rng.choice(pad) + mid + rng.choice(pad)


JSON_KEYS = ["depth", "a/b", "m~n", "", "0", "queue", "été", "list", "-"]


def gen_json_value(rng, depth):
    r = rng.random()
    if depth < 3 and r < 0.3:
        return {k: gen_json_value(rng, depth + 1)
                for k in rng.sample(JSON_KEYS, rng.randrange(0, 5))}
    if depth < 3 and r < 0.5:
        return [gen_json_value(rng, depth + 1)
                for _ in range(rng.randrange(0, 4))]
    return rng.choice([0, 7, -3, 2 ** 53 + 1, 1.5, -2.5e-7, 1e300, True,
                       False, None, "42", " 1.5 ", "0x10", "app", "", "nan",
                       "12 kB", "été"])


def gen_pointer(rng, doc):
    """Mostly a path that exists in doc, sometimes mangled."""
    toks, cur = [], doc
    while isinstance(cur, (dict, list)) and cur and rng.random() < 0.85:
        if isinstance(cur, dict):
            k = rng.choice(list(cur))
            toks.append(k)
            cur = cur[k]
        else:
            i = rng.randrange(len(cur))
            toks.append(str(i))
            cur = cur[i]
    r = rng.random()
    if r < 0.1:
        toks.append(rng.choice(["missing", "0", "-", "01", ""]))
    elif r < 0.15 and toks:
        toks[-1] = rng.choice(["99", "00", "1e0", "+1", "x"])
    return "".join("/" + t.replace("~", "~0").replace("/", "~1") for t in toks)


def gen_case(rng):
    rec = {"metric": "m"}
    scale = rng.choice(SCALES)
    if scale is not None:
        rec["scale"] = scale
    kind = rng.random()
    if kind < 0.2:
        return gen_whole_body(rng), rec
    if kind < 0.65:
        body = gen_text_body(rng)
        if rng.random() < 0.5:
            rec["line"] = rng.choice(KEYS + [b"Mem", b"nope"]).decode()
        else:
            rec["lineNumber"] = rng.randrange(1, 8)
        if rng.random() < 0.8:
            rec["field"] = rng.randrange(1, 5)
        return body, rec
    doc = gen_json_value(rng, 0)
    text = json.dumps(doc, ensure_ascii=rng.random() < 0.5,
                      indent=rng.choice([None, None, 2]))
    body = text.encode()
    r = rng.random()
    if r < 0.05:
        body = rng.choice([b"", b" \n"])
    elif r < 0.1:
        body += b" x"
    elif r < 0.3:
        body = b"\r\n " + body + b"\r\n"
    rec["json"] = gen_pointer(rng, doc)
    return body, rec


def bits(x):
    return struct.pack("<d", x)


def run_native(body, rec):
    try:
        return native.sensor_extract(body, json.dumps(rec))
    except ValueError as e:
        return str(e)


def run_model(body, rec):
    try:
        return model(body, rec)
    except Reason as e:
        return str(e)


CASES = [gen_case(random.Random(20250 + i)) for i in range(600)]


def test_generated_cases_agree_with_the_model():
    values = reasons = 0
    kinds = set()
    for body, rec in CASES:
        want = run_model(body, rec)
        got = run_native(body, rec)
        if isinstance(want, float):
            assert isinstance(got, float), (body, rec, want, got)
            assert bits(got) == bits(want), (body, rec, want, got)
            values += 1
        else:
            assert got == want, (body, rec, want, got)
            reasons += 1
            kinds.add(re.sub(r'[0-9]+|".*"|/.*', "", want))
    # the generator reaches both outcomes and every family of reason
    assert values > 150 and reasons > 150, (values, reasons)
    for kind in ["no line starts with ", "no line ", "line has  fields",
                 "not a number: ", "json: no value at ",
                 "json: unexpected end of input",
                 "json: unexpected trailing characters",
                 "value out of range"]:
        assert kind in kinds, (kind, sorted(kinds))


@pytest.mark.parametrize("body,rec,want", [
    (b"MemAvailable:   200000000 kB\n",
     {"metric": "m", "line": "MemAvailable:", "field": 2, "scale": 1024},
     204800000000.0),
    (b"Active connections: 291 \r\nserver accepts handled requests\r\n"
     b" 16630948 16630948 31070465 \r\n",
     {"metric": "m", "lineNumber": 3, "field": 1}, 16630948.0),
    (b'{"queue": {"depth": 7}}', {"metric": "m", "json": "/queue/depth"}, 7.0),
    (b"12345\n", {"metric": "m"}, 12345.0),
])
def test_documented_examples(body, rec, want):
    assert run_model(body, rec) == want
    assert native.sensor_extract(body, json.dumps(rec)) == want


def test_str_bodies_and_bad_records():
    assert native.sensor_extract("7\n", '{metric: "m", scale: 2}') == 14.0
    with pytest.raises(ValueError, match="record.json"):
        native.sensor_extract("7", '{metric: "m", json: "/a", line: "x"}')
    with pytest.raises(ValueError, match='not a number: "x"'):
        native.sensor_extract("x", '{metric: "m"}')
