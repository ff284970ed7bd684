// Tests for the Prometheus client (cpilot/metrics.hpp) and the value rule
// of user metrics (parseMetricValue in cpilot/telemetry.hpp, which trims
// and then applies gotext::parseFloat): the float printer, name rules,
// nearest-rank quantiles, bucket state across setBuckets, the refusals,
// and, given the path of
// tests/golden/metrics_cases.json, a replay of every row of that table
// through the same hooks the Python harness calls.
// Run via `bin/cpilot_metricstests [table.json]`; exits non-zero if any
// check failed. Host code only, so it is also the program to build with
// -fsanitize=address,undefined: the casts and the sort that once were
// undefined for NaN are on its path.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>
#include <vector>

#include "cpilot/json.hpp"
#include "cpilot/log.hpp"
#include "cpilot/metrics.hpp"
#include "cpilot/telemetry.hpp"

using namespace cpilot;

extern "C" {
char* cp_metrics_replay(const char* scriptJson, char** errOut);
char* cp_metric_value_string(const char* jsonText, char** errOut);
void cp_free(char* p);
}

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                         \
    }                                                                     \
  } while (0)
#define CHECK_EQ(a, b)                                                    \
  do {                                                                    \
    auto va = (a);                                                        \
    auto vb = (b);                                                        \
    if (!(va == vb)) {                                                    \
      fprintf(stderr, "FAIL %s:%d: %s != %s\n", __FILE__, __LINE__, #a,   \
              #b);                                                        \
      failures++;                                                         \
    }                                                                     \
  } while (0)

namespace {

const double kInf = std::numeric_limits<double>::infinity();
const double kNaN = std::numeric_limits<double>::quiet_NaN();

void testFormatValue() {
  using prom::formatValue;
  CHECK_EQ(formatValue(0), std::string("0"));
  CHECK_EQ(formatValue(5), std::string("5"));
  CHECK_EQ(formatValue(12.5), std::string("12.5"));
  CHECK_EQ(formatValue(1234567890.5), std::string("1234567890.5"));
  CHECK_EQ(formatValue(0.1 + 0.2), std::string("0.30000000000000004"));
  CHECK_EQ(formatValue(9007199254740992.0), std::string("9007199254740992"));
  CHECK_EQ(formatValue(999999999999999.5), std::string("999999999999999.5"));
  CHECK_EQ(formatValue(999999999999999.0), std::string("999999999999999"));
  CHECK_EQ(formatValue(1e15), std::string("1e+15"));
  CHECK_EQ(formatValue(1e-5), std::string("1e-05"));
  CHECK_EQ(formatValue(0.005), std::string("0.005"));
  CHECK_EQ(formatValue(0.99), std::string("0.99"));
  CHECK_EQ(formatValue(5e-324), std::string("5e-324"));
  CHECK_EQ(formatValue(std::numeric_limits<double>::max()),
           std::string("1.7976931348623157e+308"));
  CHECK_EQ(formatValue(kNaN), std::string("NaN"));
  CHECK_EQ(formatValue(-kNaN), std::string("NaN"));
  CHECK_EQ(formatValue(kInf), std::string("+Inf"));
  CHECK_EQ(formatValue(-kInf), std::string("-Inf"));
}

void testNames() {
  CHECK(prom::validMetricName("a"));
  CHECK(prom::validMetricName("_a:b_9"));
  CHECK(!prom::validMetricName(""));
  CHECK(!prom::validMetricName("9a"));
  CHECK(!prom::validMetricName("a b"));
  CHECK(!prom::validMetricName("x-y"));
  CHECK(!prom::validMetricName("a\n"));
  CHECK(!prom::validMetricName("\xc3\xa9"));
  CHECK(prom::isInternalName("containerpilot_events"));
  CHECK(!prom::isInternalName("containerpilot_mine"));
}

void expectValue(const char* text, double want, int line) {
  double got = 0;
  bool ok = parseMetricValue(text, &got);
  bool same = std::isnan(want) ? std::isnan(got)
                               : (got == want && std::signbit(got) ==
                                                     std::signbit(want));
  if (!ok || !same) {
    fprintf(stderr, "FAIL %s:%d: \"%s\" -> %s%.17g, want %.17g\n", __FILE__,
            line, text, ok ? "" : "refused ", got, want);
    failures++;
  }
}
void expectRefused(const char* text, int line) {
  double got = 0;
  if (parseMetricValue(text, &got)) {
    fprintf(stderr, "FAIL %s:%d: \"%s\" -> %.17g, want a refusal\n", __FILE__,
            line, text, got);
    failures++;
  }
}
#define VALUE(text, want) expectValue(text, want, __LINE__)
#define REFUSED(text) expectRefused(text, __LINE__)

// TrimSpace, then ParseFloat: the float rules have their rows in
// unittests.cpp's testGoText; these show that the wrapper trims Go's white
// space, and nothing else, before it applies them
void testParseMetricValue() {
  VALUE("1", 1);
  VALUE(" \t7.5\r\n", 7.5);
  VALUE("\xc2\xa0\xe3\x80\x80" "7.5" "\xc2\x85\xe2\x80\x83", 7.5);
  VALUE(" -INF\n", -kInf);
  VALUE("\tNaN ", kNaN);
  REFUSED("");
  REFUSED(" ");
  REFUSED("1 2");
  REFUSED(" 1e999 ");
  REFUSED("\xe2\x80\x8b" "7");  // U+200B is no white space
  REFUSED("\x85" "7");          // nor is a lone continuation byte
  double got = 0;
  CHECK(!parseMetricValue(std::string(" 1\0" "2 ", 5), &got));
}

void testSummary() {
  prom::SummaryData s;
  CHECK(std::isnan(s.quantile(1, 2)));
  for (int i = 1; i <= 10; i++) s.observe(i);
  CHECK_EQ(s.quantile(1, 2), 5.0);
  CHECK_EQ(s.quantile(9, 10), 9.0);
  CHECK_EQ(s.quantile(99, 100), 10.0);
  prom::SummaryData one;
  one.observe(4.5);
  CHECK_EQ(one.quantile(1, 2), 4.5);
  CHECK_EQ(one.quantile(99, 100), 4.5);
  // the window drops the oldest sample
  prom::SummaryData w;
  for (int i = 0; i < 8193; i++) w.observe(i);
  CHECK_EQ(w.window.size(), (size_t)8192);
  CHECK_EQ(w.count, (uint64_t)8193);
  CHECK_EQ(w.quantile(1, 2), 4096.0);    // rank 4096 of 1..8192
  CHECK_EQ(w.quantile(99, 100), 8111.0);  // rank ceil(8110.08) = 8111
  prom::SummaryData inf;
  inf.observe(kInf);
  inf.observe(-kInf);
  inf.observe(0);
  CHECK_EQ(inf.quantile(1, 2), 0.0);
  CHECK_EQ(inf.quantile(99, 100), kInf);
}

void testFamily() {
  prom::Family counter("c", "c", prom::MetricType::Counter);
  CHECK(counter.inc({}, 2));
  CHECK(!counter.inc({}, -1));
  CHECK(!counter.inc({}, kNaN));
  CHECK(counter.inc({}, 0));
  std::string out;
  counter.expose(out);
  CHECK(out.find("\nc 2\n") != std::string::npos);

  prom::Family gauge("g", "g", prom::MetricType::Gauge);
  CHECK(gauge.inc({}, -1));
  gauge.set(kNaN);
  out.clear();
  gauge.expose(out);
  CHECK(out.find("\ng NaN\n") != std::string::npos);

  for (auto type : {prom::MetricType::Histogram, prom::MetricType::Summary}) {
    prom::Family f("f", "f", type);
    CHECK(!f.observe(kNaN));
    CHECK(f.observe(kInf));
    CHECK(f.observe(-kInf));
    CHECK(f.observe(1));
    out.clear();
    f.expose(out);
    CHECK(out.find("f_count 3\n") != std::string::npos);
    CHECK(out.find("f_sum NaN\n") != std::string::npos);
  }

  // a reload sets the same bounds again; other bounds start over
  prom::Family hist("h", "line one\nC:\\path", prom::MetricType::Histogram);
  hist.setBuckets({1, 2, 5});
  for (double v : {0.5, 1.5, 3.0, 7.0}) hist.observe(v);
  hist.setBuckets({1, 2, 5});
  out.clear();
  hist.expose(out);
  CHECK(out.find("# HELP h line one\\nC:\\\\path\n") != std::string::npos);
  CHECK(out.find("h_bucket{le=\"2\"} 2\n") != std::string::npos);
  CHECK(out.find("h_bucket{le=\"+Inf\"} 4\n") != std::string::npos);
  CHECK(out.find("h_sum 12\n") != std::string::npos);
  hist.setBuckets({1, 10});
  out.clear();
  hist.expose(out);
  CHECK(out.find("h_bucket{le=\"10\"} 0\n") != std::string::npos);
  CHECK(out.find("h_bucket{le=\"+Inf\"} 0\n") != std::string::npos);
  CHECK(out.find("h_sum 0\nh_count 0\n") != std::string::npos);
}

// ---------------- the table ----------------

std::string take(char* p) {
  std::string s = p ? p : "";
  cp_free(p);
  return s;
}

bool hasLine(const std::string& text, const std::string& line) {
  std::string hay = "\n" + text;
  return hay.find("\n" + line + "\n") != std::string::npos;
}

int replayTable(const char* path) {
  std::ifstream in(path);
  if (!in) {
    fprintf(stderr, "cannot read %s\n", path);
    failures++;
    return 0;
  }
  std::stringstream buf;
  buf << in.rdbuf();
  Json table = parseJson5(buf.str());
  int rows = 0;
  for (auto& row : table.array()) {
    rows++;
    const std::string rule = row.find("rule")->str();
    Json script = row.find("script") ? *row.find("script") : Json();
    if (const Json* post = row.find("post")) {
      char* err = nullptr;
      std::string value =
          take(cp_metric_value_string(post->find("json")->str().c_str(), &err));
      cp_free(err);
      JsonObject obj;
      JsonArray metrics, events;
      metrics.push_back(*post->find("metric"));
      events.push_back(Json(post->find("key")->str() + "|" + value));
      obj.emplace_back("metrics", Json(std::move(metrics)));
      obj.emplace_back("events", Json(std::move(events)));
      script = Json(std::move(obj));
    }
    char* err = nullptr;
    char* out = cp_metrics_replay(script.dump().c_str(), &err);
    std::string error = take(err);
    const Json* wantError = row.find("error");
    if (wantError && wantError->boolean()) {
      if (out || error.find("configuration error") == std::string::npos) {
        fprintf(stderr, "FAIL row \"%s\": want a config error, got %s\n",
                rule.c_str(), out ? out : error.c_str());
        failures++;
      }
      cp_free(out);
      continue;
    }
    if (!out) {
      fprintf(stderr, "FAIL row \"%s\": %s\n", rule.c_str(), error.c_str());
      failures++;
      continue;
    }
    std::string text = take(out);
    for (auto& line : row.find("expect")->array()) {
      if (!hasLine(text, line.str())) {
        fprintf(stderr, "FAIL row \"%s\": no line \"%s\" in\n%s\n",
                rule.c_str(), line.str().c_str(), text.c_str());
        failures++;
      }
    }
  }
  return rows;
}

}  // namespace

int main(int argc, char** argv) {
  // every refused value is logged as an error by design
  logging::setLevel(logging::Level::Fatal);
  testFormatValue();
  testNames();
  testParseMetricValue();
  testSummary();
  testFamily();
  int rows = 0;
  if (argc > 1) rows = replayTable(argv[1]);
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("all metrics tests passed (%d table rows)\n", rows);
  return 0;
}
