"""The Prometheus metrics path against a model.

native.metrics_replay runs a script through the daemon's own code: the
`telemetry.metrics` decoder, Metric::onEvent (the "name|value" split and the
value parser), the collectors and Registry::expose. The exposition is parsed
by containerpilot_amd.prommodel's strict parser and every sample compared,
as float64 and exactly, with the model's collectors fed the same script.

Two tiers, as for templates: a hand-written table
(tests/golden/metrics_cases.json, every row names its rule and is `parity`,
`must-error` or `deviation`) and properties over generated values,
operation sequences and value strings.
"""

import json
import math
import os
import re
import struct
import sys

import pytest
from hypothesis import given, settings, strategies as st

from containerpilot_amd import native, prommodel as pm

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "metrics_cases.json"),
          encoding="utf-8") as f:
    CASES = json.load(f)

DBL_MAX = sys.float_info.max
PLAIN_DIGITS = re.compile(r"-?[0-9]+\Z")


# ------------------------------------------------------------ model of a script

class FamilyModel:
    """One `families` entry: children by label values, shared bounds."""

    def __init__(self, decl):
        self.name = decl["name"]
        self.type = decl["type"]
        self.label_names = decl.get("labels", [])
        self.bounds = decl.get("buckets") or pm.DEFAULT_BOUNDS
        self.children = {}

    def child(self, label_values):
        key = tuple(label_values)
        if key not in self.children:
            c = pm.COLLECTORS[self.type]()
            if self.type == "histogram":
                c.set_bounds(self.bounds)
            self.children[key] = c
        return self.children[key]

    def apply(self, op):
        kind = op["op"]
        if kind == "setBuckets":
            self.bounds = op["bounds"]
            for c in self.children.values():
                c.set_bounds(self.bounds)
            return
        c = self.child(op.get("labels", []))
        v = float(op.get("value", 0))
        if kind == "inc" and self.type == "gauge":
            c.add(v)
        else:
            c.record(v)

    def items(self):
        children = self.children
        if not children and not self.label_names:
            # an unlabelled family exposes a zero child before any value
            zero = pm.COLLECTORS[self.type]()
            if self.type == "histogram":
                zero.set_bounds(self.bounds)
            children = {(): zero}
        for values, c in children.items():
            yield tuple(zip(self.label_names, values)), c


def model_of(script):
    """(expected {(sample name, labels): float}, [(name, labels, Summary)])
    for a replay script."""
    expected = {}
    summaries = []
    user = pm.UserMetrics(script.get("metrics") or [])
    for source in script.get("events") or []:
        user.event(source)
    for _, name, kind, collector in user.metrics:
        expected.update(collector.samples(name))
        if kind == "summary":
            summaries.append((name, (), collector))
    families = {d["name"]: FamilyModel(d) for d in script.get("families") or []}
    for op in script.get("ops") or []:
        families[op["family"]].apply(op)
    for fam in families.values():
        for labels, c in fam.items():
            expected.update(c.samples(fam.name, labels))
            if fam.type == "summary":
                summaries.append((fam.name, labels, c))
    return expected, summaries


def check_against_model(text, script):
    """Parse strictly and compare every sample with the model. Returns the
    parsed families."""
    families = pm.parse_exposition(text)
    got = pm.sample_map(families)
    expected, summaries = model_of(script)
    for key, want in expected.items():
        # the key holds le as a float: float(le) is the bound exactly
        assert key in got, (key, text)
        s = got[key]
        assert pm.same_float(s.value, want), (key, s.text, want)
        # spelling condition: a whole value below 1e15 is plain digits
        if math.isfinite(want) and want == math.floor(want) \
                and abs(want) < 1e15:
            assert PLAIN_DIGITS.match(s.text), (key, s.text)
    quantile_keys = set()
    for name, labels, summary in summaries:
        for q in pm.QUANTILES:
            key = (name, labels + (("quantile", float(q)),))
            assert key in got, (key, text)
            assert summary.quantile_admissible(q, got[key].value), \
                (key, got[key].text, len(summary.window))
            quantile_keys.add(key)
    assert set(got) == set(expected) | quantile_keys, \
        set(got) ^ (set(expected) | quantile_keys)
    for fam in families:
        if fam.type == "histogram":
            assert pm.histogram_violations(fam) == [], text
    return families


def replay(script):
    return native.metrics_replay(json.dumps(script))


# ------------------------------------------------------------ the table

def _case_id(case):
    return "%s:%s" % (case["class"], case["rule"][:60])


def _script_of(case):
    if "post" in case:
        post = case["post"]
        value = native.metric_value_string(post["json"])
        return {"metrics": [post["metric"]],
                "events": [post["key"] + "|" + value]}
    return case["script"]


def test_table_is_well_formed():
    assert len(CASES) >= 60
    rules = [c["rule"] for c in CASES]
    assert len(set(rules)) == len(rules)
    for case in CASES:
        assert case["class"] in ("parity", "must-error", "deviation"), case
        assert case["rule"].strip(), case
        assert ("script" in case) != ("post" in case), case
        assert ("expect" in case) != (case.get("error") is True), case
        if case["class"] == "must-error":
            assert case.get("error") or case.get("refused") \
                or case.get("refused_all"), case


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_table_row(case):
    script = _script_of(case)
    if case.get("error"):
        with pytest.raises(ValueError) as e:
            replay(script)
        print(case["rule"], "->", e.value)
        assert "configuration error" in str(e.value), e.value
        assert case.get("error_names", "") in str(e.value), e.value
        return
    text = replay(script)
    print(case["rule"], "->\n" + text)
    families = check_against_model(text, script)
    lines = text.split("\n")
    for line in case["expect"]:
        assert line in lines, (case["rule"], line)
    refused = script["events"] if case.get("refused_all") \
        else case.get("refused", [])
    if refused:
        without = dict(script)
        without["events"] = [e for e in script["events"] if e not in refused]
        assert replay(without) == text, case["rule"]
        # and each one alone changes nothing
        for event in refused:
            alone = dict(without)
            alone["events"] = without["events"] + [event]
            assert replay(alone) == text, (case["rule"], event)
    for name, want in case.get("help", {}).items():
        fam = [f for f in families if f.name == name][0]
        assert fam.help == want, (fam.help, want)


# ------------------------------------------------------------ the parser

GOOD_EXPOSITION = (
    "# HELP a a\\\\b\\nc\n# TYPE a counter\na{x=\"1\\\"\\\\\\n\"} 1\na 2 1700\n"
    "\n# just a comment\n"
    "# TYPE h histogram\nh_bucket{le=\"1\"} 0\nh_bucket{le=\"+Inf\"} 1\n"
    "h_sum 2.5\nh_count 1\n"
    "# TYPE s summary\n# HELP s \ns{quantile=\"0.5\"} NaN\ns_sum 0\n"
    "s_count 0\nbare -Inf\n")


def test_parser_reads_a_good_exposition():
    fams = pm.parse_exposition(GOOD_EXPOSITION)
    assert [(f.name, f.type) for f in fams] == [
        ("a", "counter"), ("h", "histogram"), ("s", "summary"),
        ("bare", "untyped")]
    assert fams[0].help == "a\\b\nc"
    assert fams[0].samples[0].labels == (("x", "1\"\\\n"),)
    assert fams[2].help == ""
    assert math.isnan(fams[2].samples[0].value)
    assert fams[3].samples[0].value == -math.inf
    assert pm.parse_exposition("") == []


@pytest.mark.parametrize("bad", [
    "a 1",                                         # no final newline
    "# TYPE a counter\n# TYPE a counter\na 1\n",   # TYPE twice
    "# HELP a x\n# HELP a x\na 1\n",               # HELP twice
    "a 1\n# TYPE a counter\n",                     # TYPE after samples
    "a 1\n# HELP a x\n",                           # HELP after samples
    "# HELP a one\ntwo\n",                         # what a raw newline does
    "# HELP a x\\y\na 1\n",                        # unknown HELP escape
    "a{x=\"\\t\"} 1\n",                            # unknown label escape
    "a{x=\"1} 1\n",                                # label value not closed
    "a{x=1} 1\n",                                  # label value not quoted
    "a{x-y=\"1\"} 1\n",                            # bad label name
    "a{x=\"1\",x=\"2\"} 1\n",                      # label twice
    "a b 1\n",                                     # space in the name
    "x-y 1\n",                                     # dash in the name
    "9a 1\n",                                      # digit first
    "a nan\na{x=\"1\"} inf\nb 0x10\n",             # hex value
    "a 1_0\n",                                     # underscore
    "a\n",                                         # no value
    "a 1 2 3\n",                                   # too many fields
    "a 1 1.5\n",                                   # float timestamp
    "a 1\na 2\n",                                  # series twice
    "a{x=\"1\",y=\"2\"} 1\na{y=\"2\",x=\"1\"} 2\n",  # series twice, reordered
    "# TYPE a counter\na 1\n# TYPE b counter\nb 1\na{x=\"1\"} 2\n",  # split
    "# TYPE a counter\na_sum 1\na_total 2\n# TYPE a_total counter\n",
    "# TYPE a counter\na_bucket{le=\"1\"} 1\n# TYPE a_bucket gauge\n"
    "a_bucket{le=\"1\"} 1\n",                      # the name is taken
    "# TYPE h histogram\nh 1\n",                   # bare name in a histogram
    "# TYPE h histogram\nh_bucket 1\n",            # bucket without le
    "# TYPE h histogram\nh_bucket{le=\"x\"} 1\n",  # le is no float
    "# TYPE s summary\ns_bucket{le=\"1\"} 1\n# TYPE s_bucket summary\n"
    "s_bucket 1\ns_bucket 2\n",
    "# TYPE a widget\na 1\n",                      # unknown type
    "# TYPE a\na 1\n",                             # TYPE without a type
    "a 1\r\n",                                     # CRLF
], ids=lambda s: repr(s)[:40])
def test_parser_refuses(bad):
    with pytest.raises(pm.ExpositionError):
        pm.parse_exposition(bad)


def test_parser_agrees_with_prometheus_client():
    parser = pytest.importorskip("prometheus_client.parser")
    script = {"metrics": [
        {"name": "c", "type": "counter", "help": "a\\b\nc"},
        {"name": "g", "type": "gauge", "help": "g"},
        {"name": "h", "type": "histogram", "help": "h"},
        {"name": "s", "type": "summary", "help": "s"}],
        "events": ["__c|1.5", "__g|-0.30000000000000004", "__h|0.02",
                   "__h|3", "__s|1", "__s|2"],
        "families": [{"name": "l", "help": "l", "type": "counter",
                      "labels": ["k"]}],
        "ops": [{"family": "l", "op": "inc", "labels": ["a\\\"\n"],
                 "value": 2}]}
    text = replay(script)
    ours = {}
    for fam in pm.parse_exposition(text):
        for s in fam.samples:
            ours[(s.name, tuple(sorted(s.labels)))] = s.value
    theirs = {}
    helps = {}
    for fam in parser.text_string_to_metric_families(text):
        helps[fam.name] = fam.documentation
        for s in fam.samples:
            # that parser renames a counter's sample, as OpenMetrics does
            name = fam.name if fam.type == "counter" else s.name
            theirs[(name, tuple(sorted(s.labels.items())))] = s.value
    assert ours.keys() == theirs.keys()
    for k in ours:
        assert pm.same_float(ours[k], theirs[k]), k
    assert helps["c"] == "a\\b\nc"


# ------------------------------------------------------------ values

def _neighbours(v):
    out = [v]
    if math.isfinite(v):
        out += [math.nextafter(v, math.inf), math.nextafter(v, -math.inf)]
    return [x for x in out if math.isfinite(x)]


SPECIAL = []
for _e in range(-30, 31):
    SPECIAL += _neighbours(10.0 ** _e)
for _v in (2.0 ** 53, 1e15, 1e15 - 0.5, 1e15 + 0.5, 999999999999999.0,
           5e-324, 2.2250738585072014e-308, 2.225073858507201e-308,
           DBL_MAX, 0.1 + 0.2, 1 / 3, 2 / 3, 1234567890.5, 1700000000.5,
           0.1, 0.005, 1e-5, 2.5, 123456789012345.67, 9.007199254740993e15):
    SPECIAL += _neighbours(_v)
SPECIAL += [-v for v in SPECIAL] + [0.0, -0.0]

values = st.one_of(
    st.sampled_from(SPECIAL),
    st.floats(allow_nan=False, allow_infinity=False, width=64),
    st.integers(-10**6, 10**6).map(float),
    st.integers(0, 2**64 - 1).map(
        lambda b: struct.unpack("<d", struct.pack("<Q", b))[0]).filter(
            math.isfinite))

FOUR_METRICS = [{"name": "c", "type": "counter", "help": "c"},
                {"name": "g", "type": "gauge", "help": "g"},
                {"name": "h", "type": "histogram", "help": "h"},
                {"name": "s", "type": "summary", "help": "s"}]


@settings(max_examples=400, deadline=None)
@given(st.lists(st.tuples(values, st.booleans()), max_size=12))
def test_values_reach_the_exposition_exactly(recorded):
    """Any finite doubles recorded into each collector type come out of the
    exposition as the model's float64, bit for bit; written as Python's
    shortest text, or as POST /v3/metric spells the JSON number."""
    events = []
    for v, via_post in recorded:
        text = native.metric_value_string(json.dumps(v)) if via_post \
            else repr(v)
        assert pm.parse_float_go19(text) == v, (v, text)
        for key in ("__c", "__g", "__h", "__s"):
            events.append(key + "|" + text)
    script = {"metrics": FOUR_METRICS, "events": events}
    check_against_model(replay(script), script)


@settings(max_examples=400, deadline=None)
@given(st.one_of(values, st.integers(-2**63, 2**63 - 1)))
def test_posted_json_number_loses_no_bit(v):
    text = native.metric_value_string(json.dumps(v))
    assert pm.parse_float_go19(text) == float(v), (v, text)
    if isinstance(v, float) and v == math.floor(v) and abs(v) < 1e15:
        assert PLAIN_DIGITS.match(text), text


def test_existing_label_spellings_stay():
    """bench.py and the gpu-box tests scrape these with fixed patterns."""
    text = replay({"families": [
        {"name": "d", "help": "d", "type": "histogram",
         "buckets": pm.DISPATCH_BOUNDS},
        {"name": "h", "help": "h", "type": "histogram"},
        {"name": "s", "help": "s", "type": "summary"}], "ops": []})
    for label in ('d_bucket{le="1e-05"}', 'd_bucket{le="0.0001"}',
                  'd_bucket{le="0.1"}', 'h_bucket{le="0.005"}',
                  'h_bucket{le="0.025"}', 'h_bucket{le="2.5"}',
                  'h_bucket{le="10"}', 's{quantile="0.5"}',
                  's{quantile="0.9"}', 's{quantile="0.99"}'):
        assert "\n" + label + " " in text, label


# ------------------------------------------------------------ histograms

bounds_lists = st.lists(values, min_size=1, max_size=6, unique=True).map(sorted)


@st.composite
def histogram_scripts(draw):
    first = draw(bounds_lists)
    other = draw(bounds_lists)
    ops = []
    for _ in range(draw(st.integers(0, 14))):
        kind = draw(st.sampled_from(["observe"] * 4 + ["same", "other",
                                                       "first"]))
        if kind == "observe":
            pick = draw(st.one_of(values, st.sampled_from(first + other)))
            ops.append({"family": "h", "op": "observe",
                        "labels": [draw(st.sampled_from(["a", "b"]))],
                        "value": pick})
        else:
            ops.append({"family": "h", "op": "setBuckets", "bounds":
                        {"same": None, "other": other, "first": first}[kind]})
    # "same" repeats whatever bounds are current: the reload case
    current = first
    for op in ops:
        if op["op"] == "setBuckets":
            if op["bounds"] is None:
                op["bounds"] = current
            current = op["bounds"]
    return {"families": [{"name": "h", "help": "h", "type": "histogram",
                          "labels": ["k"], "buckets": first}], "ops": ops}


@settings(max_examples=300, deadline=None)
@given(histogram_scripts())
def test_histogram_invariants_after_any_sequence(script):
    """Buckets non-decreasing, +Inf == _count, every bucket the model's
    count, float(le) the bound exactly: after any mix of observations and
    setBuckets calls, the repeated one with unchanged bounds included."""
    text = replay(script)
    families = check_against_model(text, script)
    for fam in families:
        les = {float(s.label("le")) for s in fam.samples
               if s.label("le") is not None}
        if fam.samples:
            final = [op["bounds"] for op in script["ops"]
                     if op["op"] == "setBuckets"]
            bounds = final[-1] if final else script["families"][0]["buckets"]
            assert les == set(bounds) | {math.inf}


def test_reload_keeps_the_dispatch_histogram_consistent():
    """The bus registers its histogram again on every config generation
    and sets the same bounds."""
    observe = [{"family": "d", "op": "observe", "value": v}
               for v in (3e-6, 1.5e-5, 7e-4, 0.2)]
    again = {"family": "d", "op": "setBuckets", "bounds": pm.DISPATCH_BOUNDS}
    script = {"families": [{"name": "d", "help": "d", "type": "histogram",
                            "buckets": pm.DISPATCH_BOUNDS}],
              "ops": observe + [again] + observe + [again, again]}
    text = replay(script)
    check_against_model(text, script)
    assert 'd_bucket{le="1e-05"} 2\n' in text
    assert 'd_bucket{le="0.1"} 6\n' in text
    assert 'd_bucket{le="+Inf"} 8\n' in text


# ------------------------------------------------------------ summaries

def _summary_script(stream):
    return {"metrics": [{"name": "s", "type": "summary", "help": "s"}],
            "events": ["__s|%r" % float(v) for v in stream]}


@pytest.mark.parametrize("n", [1, 2, 3, 10, 100, 8191, 8192, 8193])
def test_summary_quantiles_are_nearest_rank(n):
    """Each exposed quantile x is a member of the window of the last
    min(n, 8192) observations with #{w < x} <= q*m <= #{w <= x}; the
    stream increases strictly, so an evicted sample would show."""
    stream = [i + 0.5 for i in range(n)]
    script = _summary_script(stream)
    text = replay(script)
    check_against_model(text, script)
    got = pm.sample_map(pm.parse_exposition(text))
    m = min(n, pm.SUMMARY_WINDOW)
    window = stream[-m:]
    for q in pm.QUANTILES:
        x = got[("s", (("quantile", float(q)),))].value
        assert x in window, (q, x)
        assert x >= window[0]
        rank = window.index(x) + 1     # 1-based, the stream has no ties
        assert rank - 1 <= q * m <= rank, (q, x, rank, m)
    assert got[("s_count", ())].value == n
    assert got[("s_sum", ())].value == math.fsum(stream)  # exact: halves


@settings(max_examples=300, deadline=None)
@given(st.lists(st.one_of(st.integers(-3, 3).map(float),
                          st.sampled_from([math.inf, -math.inf, 0.5, -0.0])),
                min_size=1, max_size=30))
def test_summary_quantiles_with_ties(stream):
    script = _summary_script(stream)
    check_against_model(replay(script), script)


# ------------------------------------------------------------ value strings

WHITE = ["", " ", "\t", "\n", "\r\n", "\v\f", "\u0085", "\u00a0", "\u1680",
         "\u2000", "\u200a", "\u2028", "\u2029", "\u202f", "\u205f",
         "\u3000", "\u200b", "\ufeff", "\x1f", "\u180e"]

number_strings = st.one_of(
    st.builds(
        lambda sign, prefix, whole, point, frac, exp: sign + prefix + whole
        + point + frac + exp,
        st.sampled_from(["", "", "+", "-", "--", "+-", "-+"]),
        st.sampled_from(["", "", "", "0x", "0X", "0b", "0o"]),
        st.sampled_from(["", "0", "1", "12", "007", "1_000", "9" * 25,
                         "1f", "٣"]),
        st.sampled_from(["", ".", ".", ".."]),
        st.sampled_from(["", "0", "5", "25", "000001", "2_5"]),
        st.sampled_from(["", "", "e5", "E-3", "e+2", "e", "e+", "E-",
                         "e999", "e-999", "e308", "e309", "e-324", "e1.5",
                         "p3", "e_1"])),
    st.sampled_from(["nan", "NaN", "NAN", "nan(x)", "nan()", "+nan", "-nan",
                     "inf", "Inf", "+inf", "-INF", "infinity", "+Infinity",
                     "-infinity", "infinit", "in", "infinityy", "++inf",
                     "1e999", "-1e999", "1e-999", "0x1p3", "0x10", "1_0",
                     ".", "-", "+", "e", "", "1.7976931348623157e308",
                     "1.7976931348623159e308", "2e308", "4.9e-324", "2e-324",
                     "true", "null"]))

value_strings = st.builds(
    lambda lead, body, trail, more: lead + body + trail + more,
    st.sampled_from(WHITE), number_strings, st.sampled_from(WHITE),
    st.sampled_from(["", "", "", "|2", "|", "|x|y", " |5"]))

GAUGE = [{"name": "g", "type": "gauge", "help": "g"}]


@settings(max_examples=1000, deadline=None)
@given(value_strings)
def test_value_strings_are_recorded_or_refused_as_go_does(text):
    """After a 1 that every run records, the string is recorded or refused
    exactly as parse_float_go19 says; a refused one leaves the exposition
    as it was."""
    before = {"metrics": GAUGE, "events": ["__g|1"]}
    script = {"metrics": GAUGE, "events": ["__g|1", "__g|" + text]}
    out = replay(script)
    check_against_model(out, script)
    try:
        pm.parse_float_go19(text.split("|")[0])
    except ValueError:
        assert out == replay(before), text


def test_value_string_defects_are_all_generated():
    """Every defect the property is meant to inject is in its alphabet."""
    refused = ["0x1p3", "1_0", "nan(x)", "+nan", "--1", ".", "1e", "1e999",
               "\u200b1", "1e1.5", ""]
    for s in refused:
        with pytest.raises(ValueError):
            pm.parse_float_go19(s)
    for s, want in [("1e-999", 0.0), (" \u30001\u0085", 1.0), (".5", 0.5),
                    ("5.", 5.0), ("+Infinity", math.inf), ("-inf", -math.inf),
                    ("1.7976931348623157e308", DBL_MAX), ("4.9e-324", 5e-324),
                    ("2e-324", 0.0)]:
        assert pm.parse_float_go19(s) == want, s
    assert math.isnan(pm.parse_float_go19("NaN"))
    assert pm.split_event("k|1|2") == ("k", "1")
    assert pm.split_event("k") is None


# ------------------------------------------------------------ config rows

def validate(metrics):
    cfg = {"consul": "localhost:8500",
           "telemetry": {"port": 9090, "interfaces": ["static:127.0.0.1"],
                         "metrics": metrics}}
    return native.validate_config(json.dumps(cfg))


@pytest.mark.parametrize("metric, names", [
    ({"name": "a b", "type": "gauge", "help": "h"}, "a b"),
    ({"namespace": "x-y", "name": "n", "type": "gauge", "help": "h"}, "x-y_n"),
    ({"namespace": "app", "subsystem": "é", "name": "n", "type": "gauge",
      "help": "h"}, "not a valid metric name"),
    ({"name": "1st", "type": "counter", "help": "h"}, "1st"),
    ({"name": "new\nline", "type": "counter", "help": "h"},
     "not a valid metric name"),
    ({"namespace": "containerpilot", "name": "events", "type": "counter",
      "help": "h"}, "containerpilot_events"),
    ({"namespace": "containerpilot", "subsystem": "watch",
      "name": "instances", "type": "gauge", "help": "h"},
     "containerpilot_watch_instances"),
], ids=lambda v: v if isinstance(v, str) else None)
def test_config_refuses_metric_names(metric, names):
    err = validate([metric])
    assert err is not None and "MetricConfig configuration error" in err, err
    assert names in err, err


@pytest.mark.parametrize("name", pm.INTERNAL_FAMILIES)
def test_config_refuses_every_internal_family_name(name):
    err = validate([{"name": name, "type": "counter", "help": "h"}])
    assert err is not None and name in err, err


def test_config_accepts_what_prometheus_accepts():
    assert validate([
        {"namespace": "app", "subsystem": "worker", "name": "jobs_done",
         "type": "counter", "help": "done"},
        {"namespace": "job:rate", "name": "_x9", "type": "gauge", "help": "h"},
        # deviation: the reference refuses a metric without help
        {"namespace": "app", "name": "no_help", "type": "gauge"},
        {"name": "escaped", "type": "gauge", "help": "a\\b\nc"},
        # its own prefix is not reserved, only the internal names are
        {"namespace": "containerpilot", "name": "mine", "type": "gauge",
         "help": "h"},
    ]) is None
