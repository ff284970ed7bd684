"""A model of the Prometheus side of the daemon, for tests.

Plain Python written from the text exposition format 0.0.4 description and
from the documentation of Go's strconv and of prometheus/client_golang. It
shares no code with the C++ under cpp/: a strict parser of the exposition,
float64 models of the four collector types, the float a recorded value
string stands for in the reference (Go 1.9's strconv.ParseFloat after
strings.TrimSpace) and the "name|value" event rule.
"""

import math
import re
from fractions import Fraction

METRIC_NAME_RE = re.compile(r"[a-zA-Z_:][a-zA-Z0-9_:]*\Z")
LABEL_NAME_RE = re.compile(r"[a-zA-Z_][a-zA-Z0-9_]*\Z")
TYPES = ("counter", "gauge", "histogram", "summary", "untyped")

# client_golang's DefBuckets, and the bounds the event bus gives
# containerpilot_event_dispatch_seconds
DEFAULT_BOUNDS = [.005, .01, .025, .05, .1, .25, .5, 1, 2.5, 5, 10]
DISPATCH_BOUNDS = [1e-5, 2e-5, 5e-5, 1e-4, 2.5e-4, 5e-4, 1e-3, 2.5e-3, 5e-3,
                   1e-2, 5e-2, 0.1]
# client_golang's default objectives, as the exact fractions they stand for
QUANTILES = (Fraction(1, 2), Fraction(9, 10), Fraction(99, 100))
SUMMARY_WINDOW = 8192
# the daemon's own families: a user metric may not take one of these names
INTERNAL_FAMILIES = (
    "containerpilot_events", "containerpilot_event_dispatch_seconds",
    "containerpilot_event_deliveries",
    "containerpilot_control_http_requests",
    "containerpilot_watch_instances", "containerpilot_sensor_samples")


# ------------------------------------------------------------ value strings

# unicode.IsSpace: what strings.TrimSpace removes
GO_SPACE = ("\t\n\v\f\r \u0085\u00a0\u1680"
            "\u2000\u2001\u2002\u2003\u2004\u2005\u2006\u2007\u2008\u2009"
            "\u200a\u2028\u2029\u202f\u205f\u3000")

_DECIMAL_RE = re.compile(
    r"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?\Z")
_INF_RE = re.compile(r"([+-]?)(?:inf|infinity)\Z", re.I)
_NAN_RE = re.compile(r"nan\Z", re.I)


def parse_float_go19(s):
    """The float64 that strconv.ParseFloat(strings.TrimSpace(s), 64) of Go
    1.9 returns; ValueError where it returns an error. A decimal mantissa
    with at least one digit, an optional exponent and an optional sign; or
    inf / infinity / nan in any case, the sign on inf only. No hex floats
    and no underscores (both came with Go 1.13). A value that overflows is
    a range error, one that underflows is 0."""
    s = s.strip(GO_SPACE)
    m = _INF_RE.match(s)
    if m:
        return -math.inf if m.group(1) == "-" else math.inf
    if _NAN_RE.match(s):
        return math.nan
    if not _DECIMAL_RE.match(s):
        raise ValueError("invalid syntax: %r" % s)
    v = float(s)  # correctly rounded, as Go's is
    if math.isinf(v):
        raise ValueError("value out of range: %r" % s)
    return v


def split_event(source):
    """(key, value text) of a Metric event's "name|value", or None when it
    has no "|": the reference takes strings.Split(source, "|")[0] and
    [1], so a third segment is ignored."""
    parts = source.split("|")
    if len(parts) < 2:
        return None
    return parts[0], parts[1]


def full_name(namespace, subsystem, name):
    """The key events carry: all three parts joined, empty ones included."""
    return "%s_%s_%s" % (namespace, subsystem, name)


def fq_name(namespace, subsystem, name):
    """prometheus.BuildFQName: the exposed name skips empty parts."""
    return "_".join(p for p in (namespace, subsystem, name) if p)


def same_float(a, b):
    """Equal as float64 values, NaN matching NaN."""
    return a == b or (math.isnan(a) and math.isnan(b))


# ------------------------------------------------------------ collectors
# Python floats are float64; adding in the same order gives the same bits.

class Counter:
    def __init__(self):
        self.value = 0.0

    def record(self, v):
        """False when refused: a negative or NaN increment."""
        if math.isnan(v) or v < 0:
            return False
        self.value += v
        return True

    def samples(self, name, labels=()):
        return {(name, labels): self.value}


class Gauge:
    def __init__(self):
        self.value = 0.0

    def record(self, v):
        self.value = v
        return True

    def add(self, v):
        self.value += v
        return True

    def samples(self, name, labels=()):
        return {(name, labels): self.value}


class Histogram:
    def __init__(self, bounds=None):
        self.set_bounds(DEFAULT_BOUNDS if bounds is None else bounds)

    def set_bounds(self, bounds):
        """The same bounds again keep the state; others start it over."""
        bounds = [float(b) for b in bounds]
        if getattr(self, "bounds", None) == bounds:
            return
        self.bounds = bounds
        self.observations = []
        self.sum = 0.0

    def record(self, v):
        """False when refused: NaN."""
        if math.isnan(v):
            return False
        self.observations.append(v)
        self.sum += v
        return True

    def samples(self, name, labels=()):
        out = {}
        for b in self.bounds:
            out[(name + "_bucket", labels + (("le", b),))] = float(
                sum(1 for v in self.observations if v <= b))
        n = float(len(self.observations))
        out[(name + "_bucket", labels + (("le", math.inf),))] = n
        out[(name + "_sum", labels)] = self.sum
        out[(name + "_count", labels)] = n
        return out


class Summary:
    def __init__(self):
        self.count = 0
        self.sum = 0.0
        self.window = []

    def record(self, v):
        """False when refused: NaN."""
        if math.isnan(v):
            return False
        self.count += 1
        self.sum += v
        self.window.append(v)
        del self.window[:-SUMMARY_WINDOW]
        return True

    def samples(self, name, labels=()):
        """Without the quantiles: see quantile_admissible."""
        return {(name + "_sum", labels): self.sum,
                (name + "_count", labels): float(self.count)}

    def quantile_admissible(self, q, x):
        """Whether x is a correct nearest-rank q-quantile of the window:
        a member with #{w < x} <= q*m <= #{w <= x}. NaN for no sample."""
        if not self.window:
            return math.isnan(x)
        m = len(self.window)
        return (x in self.window
                and sum(1 for w in self.window if w < x) <= q * m
                and sum(1 for w in self.window if w <= x) >= q * m)


COLLECTORS = {"counter": Counter, "gauge": Gauge, "histogram": Histogram,
              "summary": Summary}


class UserMetrics:
    """`telemetry.metrics` entries fed by Metric events."""

    def __init__(self, configs):
        self.metrics = []  # (key, exposed name, type, collector)
        for c in configs:
            parts = (c.get("namespace", ""), c.get("subsystem", ""),
                     c.get("name", ""))
            self.metrics.append((full_name(*parts), fq_name(*parts),
                                 c["type"], COLLECTORS[c["type"]]()))

    def event(self, source):
        """Offer one event to every metric. True when some metric recorded
        it."""
        kv = split_event(source)
        if kv is None:
            return False
        recorded = False
        for key, _, _, collector in self.metrics:
            if key != kv[0]:
                continue
            try:
                v = parse_float_go19(kv[1])
            except ValueError:
                continue
            recorded = collector.record(v) or recorded
        return recorded

    def samples(self):
        out = {}
        for _, name, _, collector in self.metrics:
            out.update(collector.samples(name))
        return out


# ------------------------------------------------------------ exposition

class ExpositionError(ValueError):
    pass


class Sample:
    def __init__(self, name, labels, value, text):
        self.name = name
        self.labels = labels  # tuple of (name, value) in exposed order
        self.value = value
        self.text = text      # the value as spelled

    def label(self, name):
        return dict(self.labels).get(name)

    def __repr__(self):
        return "Sample(%r, %r, %r)" % (self.name, self.labels, self.text)


class Family:
    def __init__(self, name):
        self.name = name
        self.help = None
        self.type = "untyped"
        self.typed = False
        self.samples = []

    def sample_names(self):
        if self.type == "histogram":
            return [self.name + s for s in ("_bucket", "_sum", "_count")]
        if self.type == "summary":
            return [self.name, self.name + "_sum", self.name + "_count"]
        return [self.name]


def _unescape(text, escapes, what):
    out = []
    i = 0
    while i < len(text):
        c = text[i]
        if c == "\\":
            pair = text[i:i + 2]
            if pair not in escapes:
                raise ExpositionError("bad escape %r in %s" % (pair, what))
            out.append(escapes[pair])
            i += 2
        else:
            out.append(c)
            i += 1
    return "".join(out)


_HELP_ESCAPES = {"\\\\": "\\", "\\n": "\n"}
_LABEL_ESCAPES = {"\\\\": "\\", "\\\"": "\"", "\\n": "\n"}


def _parse_value(token):
    if token != token.strip(GO_SPACE) or not token:
        raise ExpositionError("bad value %r" % token)
    try:
        return parse_float_go19(token)
    except ValueError:
        raise ExpositionError("bad value %r" % token)


def _parse_labels(text, line):
    """`text` is what stands between the braces."""
    labels = []
    i = 0
    n = len(text)
    while i < n:
        eq = text.find("=", i)
        if eq < 0:
            raise ExpositionError("label without '=': %r" % line)
        name = text[i:eq].strip(" \t")
        if not LABEL_NAME_RE.match(name):
            raise ExpositionError("bad label name %r: %r" % (name, line))
        j = eq + 1
        while j < n and text[j] in " \t":
            j += 1
        if j >= n or text[j] != '"':
            raise ExpositionError("label value not quoted: %r" % line)
        j += 1
        start = j
        while j < n and text[j] != '"':
            j += 2 if text[j] == "\\" else 1
        if j >= n:
            raise ExpositionError("label value not closed: %r" % line)
        value = _unescape(text[start:j], _LABEL_ESCAPES, "label value")
        if name in dict(labels):
            raise ExpositionError("label %r twice: %r" % (name, line))
        labels.append((name, value))
        j += 1
        while j < n and text[j] in " \t":
            j += 1
        if j < n:
            if text[j] != ",":
                raise ExpositionError("junk after label value: %r" % line)
            j += 1
        i = j
    return tuple(labels)


def _closing_brace(line, start):
    """Index of the '}' that closes the label set opened before `start`."""
    in_quotes = False
    i = start
    while i < len(line):
        c = line[i]
        if in_quotes:
            if c == "\\":
                i += 1
            elif c == '"':
                in_quotes = False
        elif c == '"':
            in_quotes = True
        elif c == "}":
            return i
        i += 1
    raise ExpositionError("label set not closed: %r" % line)


def parse_exposition(text):
    """Families (in order) of a text-format 0.0.4 exposition. Raises
    ExpositionError on anything the format does not allow."""
    if text and not text.endswith("\n"):
        raise ExpositionError("last line does not end in a newline")
    families = []
    by_name = {}
    series = set()
    current = None

    def family(name):
        nonlocal current
        if current is not None and current.name == name:
            return current
        if name in by_name:
            raise ExpositionError("family %r appears twice" % name)
        if not METRIC_NAME_RE.match(name):
            raise ExpositionError("bad metric name %r" % name)
        current = Family(name)
        by_name[name] = current
        families.append(current)
        return current

    for line in text.split("\n")[:-1] if text else []:
        if "\r" in line:
            raise ExpositionError("carriage return in %r" % line)
        stripped = line.strip(" \t")
        if not stripped:
            continue
        if stripped.startswith("#"):
            m = re.match(r"#[ \t]+(HELP|TYPE)[ \t]+([^ \t]+)(?:[ \t]+(.*))?\Z",
                         stripped, re.S)
            if not m:
                if re.match(r"#[ \t]+(HELP|TYPE)\b", stripped):
                    raise ExpositionError("malformed %r" % line)
                continue  # a plain comment
            kind, name, rest = m.group(1), m.group(2), m.group(3) or ""
            fam = family(name)
            if fam.samples:
                raise ExpositionError("%s after samples: %r" % (kind, line))
            if kind == "HELP":
                if fam.help is not None:
                    raise ExpositionError("second HELP: %r" % line)
                fam.help = _unescape(rest, _HELP_ESCAPES, "help")
            else:
                if fam.typed:
                    raise ExpositionError("second TYPE: %r" % line)
                if rest not in TYPES:
                    raise ExpositionError("unknown type: %r" % line)
                fam.type = rest
                fam.typed = True
            continue

        m = re.match(r"[^ \t{]+", stripped)
        if not m:
            raise ExpositionError("no metric name: %r" % line)
        name = m.group(0)
        if not METRIC_NAME_RE.match(name):
            raise ExpositionError("bad metric name %r: %r" % (name, line))
        rest = stripped[m.end():]
        labels = ()
        if rest.startswith("{"):
            close = _closing_brace(rest, 1)
            labels = _parse_labels(rest[1:close], line)
            rest = rest[close + 1:]
        tokens = rest.split()
        if len(tokens) not in (1, 2) or rest[:1] not in (" ", "\t"):
            raise ExpositionError("want a value and at most a timestamp: %r"
                                  % line)
        value = _parse_value(tokens[0])
        if len(tokens) == 2 and not re.match(r"-?[0-9]+\Z", tokens[1]):
            raise ExpositionError("bad timestamp: %r" % line)

        if current is not None and name in current.sample_names():
            fam = current
        else:
            for other in families:
                if other is not current and name in other.sample_names():
                    raise ExpositionError(
                        "sample of %r outside its family: %r"
                        % (other.name, line))
            fam = family(name)  # a new untyped family, or the current one
            if name not in fam.sample_names():
                raise ExpositionError("sample %r does not fit type %s: %r"
                                      % (name, fam.type, line))
        if fam.type == "histogram" and name.endswith("_bucket") \
                and "le" not in dict(labels):
            raise ExpositionError("bucket without le: %r" % line)
        if "le" in dict(labels) and fam.type == "histogram":
            _parse_value(dict(labels)["le"])
        if "quantile" in dict(labels) and fam.type == "summary":
            _parse_value(dict(labels)["quantile"])
        key = (name, tuple(sorted(labels)))
        if key in series:
            raise ExpositionError("series appears twice: %r" % line)
        series.add(key)
        fam.samples.append(Sample(name, labels, value, tokens[0]))
    return families


def sample_map(families):
    """{(sample name, labels with le/quantile as floats): Sample}."""
    out = {}
    for fam in families:
        for s in fam.samples:
            labels = tuple(
                (k, parse_float_go19(v)) if k in ("le", "quantile") else (k, v)
                for k, v in s.labels)
            out[(s.name, labels)] = s
    return out


def histogram_violations(fam):
    """What breaks the histogram invariants in one parsed family, per label
    set: buckets non-decreasing in le, a +Inf bucket that is not below the
    last finite one and equals _count."""
    problems = []
    groups = {}
    for s in fam.samples:
        rest = tuple(kv for kv in s.labels if kv[0] != "le")
        groups.setdefault(rest, []).append(s)
    for rest, samples in groups.items():
        buckets = sorted((parse_float_go19(s.label("le")), s.value)
                         for s in samples if s.name == fam.name + "_bucket")
        counts = [s.value for s in samples if s.name == fam.name + "_count"]
        if not buckets or buckets[-1][0] != math.inf:
            problems.append("%r: no +Inf bucket" % (rest,))
            continue
        for (le0, c0), (le1, c1) in zip(buckets, buckets[1:]):
            if c1 < c0:
                problems.append("%r: le=%r has %r after le=%r with %r"
                                % (rest, le1, c1, le0, c0))
        if counts != [buckets[-1][1]]:
            problems.append("%r: +Inf %r but _count %r"
                            % (rest, buckets[-1][1], counts))
    return problems
