"""Duration parsing against a model of Go's time.ParseDuration and of the
reference's ParseDuration wrapper (an int or an integer string is seconds).

The native entry point takes the JSON5 text of the value, as a config file
holds it: `"1m30s"` with its quotes, or a bare int.
"""

import json

import pytest
from hypothesis import given, settings, strategies as st

from containerpilot_amd import gomodel, native

INT64_MAX = 2**63 - 1
INT64_MIN = -(2**63)
ERROR = "error"


def native_duration(value):
    """ns, or ERROR. `value` is a str or an int."""
    try:
        return native.parse_duration(json.dumps(value, ensure_ascii=False))
    except ValueError:
        return ERROR


def model_duration(value):
    try:
        return gomodel.parse_duration(value)
    except gomodel.GoError:
        return ERROR


# what Go answers, stated by hand
TABLE = [
    # the reference's own rules
    (60, 60 * 10**9), ("60", 60 * 10**9), ("1m", 60 * 10**9),
    ("1m30s", 90 * 10**9), ("500ms", 500 * 10**6), ("1.5h", 5400 * 10**9),
    ("100us", 100000), ("100µs", 100000), ("100μs", 100000),
    ("0", 0), ("+0", 0), ("-0", 0), ("-5", -5 * 10**9), ("+5", 5 * 10**9),
    ("-1.5s", -1500000000), ("+1h", 3600 * 10**9), ("1h1m1s1ms1us1ns",
                                                    3661001001001),
    ("1.s", 10**9), (".5s", 5 * 10**8), ("0.000000001s", 1), ("1ns", 1),
    ("0s", 0), ("007s", 7 * 10**9), ("1s1s", 2 * 10**9),
    # integer accumulation: no float rounding of the whole number
    ("1.001s", 1001000000), ("0.3s", 300000000), ("1.1h", 3960 * 10**9),
    ("9007199254740993ns", 9007199254740993),
    # digit rules
    ("1.2.3s", ERROR), (".s", ERROR), (" 5", ERROR), ("5 ", ERROR),
    ("", ERROR), ("+", ERROR), ("-", ERROR), ("s", ERROR), (".", ERROR),
    ("1.5", ERROR), ("1.0", ERROR), ("1 s", ERROR), ("1s ", ERROR),
    (" 1s", ERROR), ("1S", ERROR), ("1d", ERROR), ("1sec", ERROR),
    ("--1s", ERROR), ("1s-", ERROR), ("1e3s", ERROR), ("0x10s", ERROR),
    ("1_000s", ERROR), ("١s", ERROR), ("xx", ERROR),
    # overflow is an error, both bounds are reachable
    ("9223372037s", ERROR), ("9223372036s", 9223372036 * 10**9),
    ("100000000000000000000ns", ERROR), ("100000000000000000000", ERROR),
    ("9223372036854775807ns", INT64_MAX), ("9223372036854775808ns", ERROR),
    ("-9223372036854775808ns", INT64_MIN), ("-9223372036854775809ns", ERROR),
    ("2562047h47m16.854775807s", INT64_MAX),
    ("2562047h47m16.854775808s", ERROR),
    ("-2562047h47m16.854775808s", INT64_MIN),
    ("-2562047h47m16.854775809s", ERROR),
    ("2562048h", ERROR), ("9223372036854775807", ERROR),
    ("4611686018427387904ns4611686018427387904ns", ERROR),
    # bare ints past what a Duration holds are refused (Go would wrap)
    (9223372036, 9223372036 * 10**9), (9223372037, ERROR),
    (-9223372036, -9223372036 * 10**9), (-9223372037, ERROR), (0, 0), (-1,
                                                                      -10**9),
]


@pytest.mark.parametrize("value,want", TABLE, ids=[repr(v) for v, _ in TABLE])
def test_duration_table(value, want):
    assert model_duration(value) == want
    got = native_duration(value)
    print(repr(value), "->", got)
    assert got == want


def test_old_entry_point_is_unchanged():
    assert native.parse_duration_ns('"1m30s"') == 90_000_000_000
    with pytest.raises(ValueError):
        native.parse_duration_ns('"xx"')
    # ... and still cannot tell a negative duration from an error
    with pytest.raises(ValueError):
        native.parse_duration_ns('"-1s"')
    assert native.parse_duration('"-1s"') == -10**9


def test_floats_and_other_types_are_refused():
    for text in ("1.5", "true", "null", "[1]", "{}", "1e3"):
        with pytest.raises(ValueError):
            native.parse_duration(text)


# fractional digits at which unit / 10^digits is exact in float64, so that
# Go's one float step adds exactly frac * unit / 10^digits
FRACTION_DIGITS = {"ns": 0, "us": 3, "µs": 3, "μs": 3, "ms": 6, "s": 9,
                   "m": 9, "h": 9}
UNIT_NS = {"ns": 1, "us": 10**3, "µs": 10**3, "μs": 10**3, "ms": 10**6,
           "s": 10**9, "m": 60 * 10**9, "h": 3600 * 10**9}


@st.composite
def terms(draw):
    """One `number unit` term: mostly small, sometimes within a few ns of
    2^63 ns or past it."""
    unit = draw(st.sampled_from(sorted(UNIT_NS)))
    mode = draw(st.sampled_from(["small", "small", "small", "edge", "huge"]))
    if mode == "small":
        whole = draw(st.integers(0, 5000))
    elif mode == "edge":
        whole = (2**63 + draw(st.integers(-3, 3))) // UNIT_NS[unit] + \
            draw(st.integers(-1, 1))
    else:
        whole = draw(st.integers(2**62, 2**66))
    digits = draw(st.integers(0, FRACTION_DIGITS[unit]))
    text = "" if (whole == 0 and digits > 0 and draw(st.booleans())) \
        else ("0" * draw(st.integers(0, 2)) + str(max(whole, 0)))
    if digits > 0 or draw(st.integers(0, 9)) == 0:
        text += "." + "".join(
            draw(st.sampled_from("0123456789")) for _ in range(digits))
    if text == ".":
        text = "0."
    return text + unit


DEFECTS = ["none", "none", "none", "second-dot", "missing-unit",
           "whitespace", "unknown-unit", "uppercase-unit"]


@st.composite
def duration_strings(draw):
    parts = [draw(terms()) for _ in range(draw(st.integers(1, 3)))]
    defect = draw(st.sampled_from(DEFECTS))
    k = draw(st.integers(0, len(parts) - 1))
    term = parts[k]
    number = term.rstrip("nsuµμmh")
    unit = term[len(number):]
    if defect == "second-dot":
        cut = draw(st.integers(0, len(number)))
        dotted = number if "." in number else number + "."
        parts[k] = dotted[:cut] + "." + dotted[cut:] + unit
    elif defect == "missing-unit":
        parts[k] = number
    elif defect == "whitespace":
        where = draw(st.sampled_from(["before", "inside", "after"]))
        space = draw(st.sampled_from([" ", "\t", "\n"]))
        parts[k] = {"before": space + term, "inside": number + space + unit,
                    "after": term + space}[where]
    elif defect == "unknown-unit":
        parts[k] = number + draw(st.sampled_from(
            ["d", "sec", "mss", "hs", "nm", "µ", "y", "min"]))
    elif defect == "uppercase-unit":
        parts[k] = number + unit.upper().replace("µ", "U").replace("Μ", "U")
    sign = draw(st.sampled_from(["", "", "+", "-"]))
    return sign + "".join(parts)


@settings(max_examples=600, deadline=None, derandomize=True)
@given(duration_strings())
def test_duration_strings_match_the_model(text):
    assert native_duration(text) == model_duration(text), text


@settings(max_examples=300, deadline=None, derandomize=True)
@given(st.one_of(st.integers(-20000, 20000),
                 st.integers(-(2**63) - 5, 2**63 + 5),
                 st.integers(9223372030, 9223372040),
                 st.integers(-9223372040, -9223372030)),
       st.sampled_from(["", "+", "-"]),
       st.sampled_from(["", " ", "\t", "\n"]),
       st.sampled_from(["", " ", "\t", "\n"]))
def test_integers_and_integer_strings_are_seconds(n, sign, lead, trail):
    # a bare int in the config text; white space around it is JSON5's affair
    if INT64_MIN <= n <= INT64_MAX:
        want = model_duration(n)
        try:
            got = native.parse_duration(lead + str(n) + trail)
        except ValueError:
            got = ERROR
        assert got == want, n
    # the same digits as a string: Atoi is strict, so any space is an error
    text = lead + sign + str(abs(n)) + trail
    assert native_duration(text) == model_duration(text), repr(text)
    if lead or trail:
        assert native_duration(text) == ERROR, repr(text)
