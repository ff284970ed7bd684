// Assert-style unit tests for the pure components (config pipeline,
// template engine, durations, event model, IP specs, arg parsing).
// Test coverage mirrors the reference's package unit tests
// (config/*_test.go, commands/commands_test.go, events/events_test.go).
// Run via `bin/cpilot_unittests`; exits non-zero on first failure.
#include <arpa/inet.h>
#include <netinet/in.h>

#include <poll.h>

#include <atomic>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <limits>
#include <thread>
#include <vector>
#include <cstdlib>
#include <cstring>
#include <string>

#include <signal.h>
#include <sys/epoll.h>
#include <sys/signalfd.h>
#include <sys/socket.h>
#include <sys/un.h>
#include <unistd.h>

#include "cpilot/command.hpp"
#include "cpilot/config.hpp"
#include "cpilot/jobs.hpp"
#include "cpilot/decode.hpp"
#include "cpilot/events.hpp"
#include "cpilot/gotext.hpp"
#include "cpilot/http.hpp"
#include "cpilot/ips.hpp"
#include "cpilot/json.hpp"
#include "cpilot/timing.hpp"
#include "cpilot/tmpl.hpp"

using namespace cpilot;

static int failures = 0;
static std::atomic<int> checks{0};  // CHECKs run on helper threads too
#define CHECK(cond)                                                       \
  do {                                                                    \
    checks++;                                                             \
    if (!(cond)) {                                                        \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                         \
    }                                                                     \
  } while (0)
#define CHECK_EQ(a, b)                                                    \
  do {                                                                    \
    auto va = (a);                                                        \
    auto vb = (b);                                                        \
    checks++;                                                             \
    if (!(va == vb)) {                                                    \
      fprintf(stderr, "FAIL %s:%d: %s != %s\n", __FILE__, __LINE__, #a,   \
              #b);                                                        \
      failures++;                                                         \
    }                                                                     \
  } while (0)

static void testJson5() {
  // comments, unquoted keys, trailing commas, single quotes
  Json v = parseJson5(R"({
    // line comment
    unquoted: 'single',
    "trailing": [1, 2, 3,],
    /* block comment */
    hex: 0xFF,
    float: 1.5e2,
    nested: {a: true, b: null},
  })");
  CHECK(v.isObject());
  CHECK_EQ(v.find("unquoted")->str(), std::string("single"));
  CHECK_EQ(v.find("trailing")->array().size(), (size_t)3);
  CHECK_EQ(v.find("hex")->asInt(), (int64_t)255);
  CHECK_EQ(v.find("float")->asDouble(), 150.0);
  CHECK(v.find("nested")->find("b")->isNull());

  // int vs double distinction (restarts truncation semantics)
  Json n = parseJson5("{a: 3, b: 1.2}");
  CHECK(n.find("a")->isInt());
  CHECK(n.find("b")->isDouble());

  // parse errors report offsets
  bool threw = false;
  try {
    parseJson5("{a: }");
  } catch (const JsonParseError& e) {
    threw = true;
    std::string msg = formatParseError("{a: }", e);
    CHECK(msg.find("parse error at line:col") == 0);
  }
  CHECK(threw);

  // serializer round-trip
  CHECK_EQ(parseJson5("{\"a\":[1,\"x\"],\"b\":true}").dump(),
           std::string("{\"a\":[1,\"x\"],\"b\":true}"));

  // duplicate keys: last wins (Go map unmarshal semantics)
  CHECK_EQ(parseJson5("{a: 1, a: 2}").find("a")->asInt(), (int64_t)2);

  // JSON5 numeric edge forms
  CHECK_EQ(parseJson5("[+5, .5, 5., -0x10]").array().size(), (size_t)4);
  CHECK(parseJson5("Infinity").isDouble());
  CHECK(parseJson5("[-Infinity]").array()[0].asDouble() < 0);
  CHECK_EQ(parseJson5("\"\\u00e9\"").str(), std::string("\xc3\xa9"));

  // pathological nesting is rejected, not a stack overflow
  std::string deep(100000, '[');
  bool threwDeep = false;
  try {
    parseJson5(deep);
  } catch (const JsonParseError&) {
    threwDeep = true;
  }
  CHECK(threwDeep);
}

static void testDurations() {
  // bare ints are seconds (timing/duration.go:33-51)
  CHECK(parseDuration(Json((int64_t)60)) == std::chrono::seconds(60));
  // numeric strings are seconds (duration.go:53-55)
  CHECK(parseDuration(Json("60")) == std::chrono::seconds(60));
  // unit strings use Go grammar
  CHECK(parseDuration(Json("1m")) == std::chrono::minutes(1));
  CHECK(parseDuration(Json("1m30s")) == std::chrono::seconds(90));
  CHECK(parseDuration(Json("500ms")) == std::chrono::milliseconds(500));
  CHECK(parseDuration(Json("1.5h")) == std::chrono::minutes(90));
  CHECK(parseGoDuration("100us") == std::chrono::microseconds(100));
  bool threw = false;
  try {
    parseDuration(Json("xx"));
  } catch (...) {
    threw = true;
  }
  CHECK(threw);
  // floats are an error (unexpected duration of type float64)
  threw = false;
  try {
    parseDuration(Json(1.5));
  } catch (...) {
    threw = true;
  }
  CHECK(threw);

  // Go's ParseDuration accumulates integers: no float rounding, the digit
  // rules, overflow is an error and both int64 bounds are reachable
  auto ns = [](const char* s) { return parseDuration(Json(s)).count(); };
  auto bad = [](const char* s) {
    try {
      parseDuration(Json(s));
    } catch (const std::exception&) {
      return true;
    }
    return false;
  };
  CHECK_EQ(ns("1.001s"), (int64_t)1001000000);
  CHECK_EQ(ns("-5"), (int64_t)-5000000000LL);
  CHECK_EQ(ns(".5s"), (int64_t)500000000);
  CHECK_EQ(ns("1.s"), (int64_t)1000000000);
  CHECK_EQ(ns("100\xc2\xb5s"), (int64_t)100000);
  CHECK_EQ(ns("2562047h47m16.854775807s"), INT64_MAX);
  CHECK_EQ(ns("-2562047h47m16.854775808s"), INT64_MIN);
  CHECK_EQ(ns("9223372036854775807ns"), INT64_MAX);
  CHECK(bad("1.2.3s"));
  CHECK(bad(".s"));
  CHECK(bad(" 5"));
  CHECK(bad("5 "));
  CHECK(bad("1S"));
  CHECK(bad("1d"));
  CHECK(bad("1.5"));
  CHECK(bad("9223372037s"));
  CHECK(bad("9223372037"));
  CHECK(bad("100000000000000000000ns"));
  CHECK(bad("9223372036854775808ns"));
  CHECK(bad("2562047h47m16.854775808s"));
  CHECK(bad("-9223372036854775809ns"));
  threw = false;
  try {
    parseDuration(Json((int64_t)9223372037LL));
  } catch (...) {
    threw = true;
  }
  CHECK(threw);
}

static void testTemplate() {
  setenv("TEST_NAME", "eleven", 1);
  setenv("TEST_PARTS", "a:b:c", 1);
  unsetenv("TEST_MISSING");

  CHECK_EQ(renderTemplate("Hello, {{.TEST_NAME}}!"),
           std::string("Hello, eleven!"));
  // missingkey=zero
  CHECK_EQ(renderTemplate("[{{.TEST_MISSING}}]"), std::string("[]"));
  // default (template.go:129-140)
  CHECK_EQ(renderTemplate("{{.TEST_MISSING | default \"World\"}}"),
           std::string("World"));
  CHECK_EQ(renderTemplate("{{.TEST_NAME | default \"World\"}}"),
           std::string("eleven"));
  CHECK_EQ(renderTemplate("{{.TEST_MISSING | default 100}}"),
           std::string("100"));
  CHECK_EQ(renderTemplate("{{.TEST_MISSING | default 10.1}}"),
           std::string("10.1"));
  // env func
  CHECK_EQ(renderTemplate("{{ env \"TEST_NAME\" }}"), std::string("eleven"));
  // split | join
  CHECK_EQ(renderTemplate("{{.TEST_PARTS | split \":\" | join \".\"}}"),
           std::string("a.b.c"));
  // replaceAll / regexReplaceAll
  CHECK_EQ(renderTemplate("{{.TEST_NAME | replaceAll \"e\" \"_\"}}"),
           std::string("_l_v_n"));
  CHECK_EQ(
      renderTemplate("{{.TEST_NAME | regexReplaceAll \"[el]+\" \"_\"}}"),
      std::string("_v_n"));
  // loop + range
  CHECK_EQ(renderTemplate("{{ range loop 3 }}x{{ end }}"), std::string("xxx"));
  CHECK_EQ(renderTemplate("{{ range $i := loop 2 5 }}{{ $i }}{{ end }}"),
           std::string("234"));
  CHECK_EQ(renderTemplate("{{ range $i := loop 5 1 }}{{ $i }}{{ end }}"),
           std::string("5432"));
  // trim markers
  CHECK_EQ(renderTemplate("a {{- \"b\" -}} c"), std::string("abc"));
  // printf + nested calls
  CHECK_EQ(renderTemplate("{{ env (printf \"TEST_%s\" \"NAME\") }}"),
           std::string("eleven"));
  // if/else
  CHECK_EQ(renderTemplate("{{ if .TEST_NAME }}y{{ else }}n{{ end }}"),
           std::string("y"));
  CHECK_EQ(renderTemplate("{{ if .TEST_MISSING }}y{{ else }}n{{ end }}"),
           std::string("n"));

  // exact expectations from the reference's template_test.go:50-70
  setenv("COUNT", "3", 1);
  CHECK_EQ(renderTemplate("{{ loop 2 5 }}"), std::string("[2 3 4]"));
  CHECK_EQ(renderTemplate("{{ loop 10 1 }}"),
           std::string("[10 9 8 7 6 5 4 3 2]"));
  CHECK_EQ(renderTemplate("{{ loop 5 }}"), std::string("[0 1 2 3 4]"));
  CHECK_EQ(renderTemplate("{{ loop .COUNT }}"), std::string("[0 1 2]"));
  CHECK_EQ(renderTemplate("{{ loop 1 .COUNT }}"), std::string("[1 2]"));
  CHECK_EQ(renderTemplate("{{ range $i := loop 2 5 -}}i={{$i}},{{ end }}"),
           std::string("i=2,i=3,i=4,"));
  unsetenv("COUNT");

  // Go template builtins are available to reference configs
  setenv("STAGE", "prod", 1);
  CHECK_EQ(renderTemplate("{{ if eq .STAGE \"prod\" }}P{{ else }}D{{ end }}"),
           std::string("P"));
  CHECK_EQ(renderTemplate("{{ if ne .STAGE \"dev\" }}y{{ end }}"),
           std::string("y"));
  CHECK_EQ(renderTemplate("{{ if and .STAGE .TEST_NAME }}both{{ end }}"),
           std::string("both"));
  CHECK_EQ(renderTemplate("{{ or .TEST_MISSING \"fallback\" }}"),
           std::string("fallback"));
  CHECK_EQ(renderTemplate("{{ if not .TEST_MISSING }}empty{{ end }}"),
           std::string("empty"));
  CHECK_EQ(renderTemplate("{{ len \"abcd\" }}"), std::string("4"));
  CHECK_EQ(renderTemplate("{{ len (loop 3) }}"), std::string("3"));
  CHECK_EQ(renderTemplate("{{ index (loop 5 8) 1 }}"), std::string("6"));
  CHECK_EQ(renderTemplate("{{ if lt 1 2 }}y{{ end }}"), std::string("y"));
  CHECK_EQ(renderTemplate("{{ print \"a\" 1 2 }}"), std::string("a1 2"));

  // comments, assignment, with, else-if, two-var range
  CHECK_EQ(renderTemplate("a{{/* ignore me */}}b"), std::string("ab"));
  CHECK_EQ(renderTemplate("{{ $x := \"v\" }}{{ $x }}{{ $x }}"),
           std::string("vv"));
  CHECK_EQ(renderTemplate("{{ with .STAGE }}got-{{ . }}{{ end }}"),
           std::string("got-prod"));
  CHECK_EQ(renderTemplate("{{ with .TEST_MISSING }}y{{ else }}n{{ end }}"),
           std::string("n"));
  CHECK_EQ(renderTemplate(
               "{{ if eq .STAGE \"dev\" }}d{{ else if eq .STAGE \"prod\" "
               "}}p{{ else }}o{{ end }}"),
           std::string("p"));
  CHECK_EQ(renderTemplate(
               "{{ range $i, $v := loop 5 8 }}{{ $i }}:{{ $v }} {{ end }}"),
           std::string("0:5 1:6 2:7 "));
  unsetenv("STAGE");

  // Go 1.9 semantics the engine has to match (the same rows, and many
  // more, are in tests/golden/template_cases.json)
  auto fails = [](const char* t) {
    try {
      renderTemplate(t);
    } catch (const std::exception&) {
      return true;
    }
    return false;
  };
  setenv("FOO", "abc", 1);
  unsetenv("MISSING");
  CHECK_EQ(renderTemplate(
               "{{ range split \",\" .MISSING }}x{{ else }}none{{ end }}"),
           std::string("none"));
  CHECK_EQ(renderTemplate("{{ $x := \"a\" }}{{ if \"y\" }}{{ $x := \"b\" }}"
                          "{{ end }}{{ $x }}"),
           std::string("a"));
  CHECK(fails("{{ if \"y\" }}{{ $z := 1 }}{{ end }}{{ $z }}"));
  CHECK_EQ(renderTemplate("{{ if true }}y{{ end }}{{ false }}"),
           std::string("yfalse"));
  CHECK(fails("{{ .FOO bar }}"));
  CHECK(fails("{{ .FOO \"x\" }}"));
  CHECK(fails("{{ (.FOO).X }}"));
  CHECK(fails("{{ end x }}"));
  CHECK_EQ(renderTemplate("{{ 0x10 }} {{ 010 }} {{ 1e3 }}"),
           std::string("16 8 1000"));
  CHECK_EQ(renderTemplate("{{ with $x := .FOO }}{{ $x }}{{ end }}"
                          "{{ if $y := .FOO }}{{ $y }}{{ end }}"),
           std::string("abcabc"));
  CHECK_EQ(renderTemplate("{{ \"a}}b\" }}{{/* }} */}}"), std::string("a}}b"));
  CHECK_EQ(renderTemplate("{{ \"\\x41\\u00e9\\\\\" }}"),
           std::string("A\xc3\xa9\\"));
  CHECK(fails("{{ \"\\q\" }}"));
  CHECK_EQ(renderTemplate("{{ regexReplaceAll \"(a)\" \"${1}x\" \"a\" }}"),
           std::string("ax"));
  CHECK_EQ(renderTemplate("{{ regexReplaceAll \"(a)\" \"$1x\" \"a\" }}"),
           std::string(""));
  CHECK_EQ(renderTemplate("{{ regexReplaceAll \"a\" \"[$&]\" \"a\" }}"),
           std::string("[$&]"));
  CHECK_EQ(renderTemplate("{{ regexReplaceAll \"x*\" \"-\" \"abxd\" }}"),
           std::string("-a-b-d-"));
  CHECK_EQ(renderTemplate("{{ regexReplaceAll \".\" \"x\" \"\xc3\xa9\" }}"),
           std::string("x"));
  CHECK_EQ(renderTemplate("{{ regexReplaceAll \"(?i)A\" \"b\" \"aA\" }}"),
           std::string("bb"));
  CHECK_EQ(renderTemplate(
               "{{ regexReplaceAll \"(?P<n>a)\" \"${n}$n\" \"a\" }}"),
           std::string("aa"));
  CHECK(fails("{{ regexReplaceAll `\\pL` \"x\" \"a\" }}"));
  CHECK(fails("{{ regexReplaceAll `a\\z` \"x\" \"a\" }}"));
  CHECK(fails("{{ regexReplaceAll `a(?i)b` \"x\" \"ab\" }}"));
  CHECK(fails("{{ regexReplaceAll `(a)\\1` \"x\" \"aa\" }}"));
  CHECK(fails("{{ regexReplaceAll `a(?=b)` \"x\" \"ab\" }}"));
  CHECK(fails("{{ regexReplaceAll \"a\" \"x\" \"\\xff\" }}"));
  CHECK_EQ(renderTemplate("{{ \"a\" | replaceAll \"\" \"-\" }}"),
           std::string("-a-"));
  CHECK_EQ(renderTemplate("{{ split \"\" \"a\xc3\xa9\" | join \",\" }}"),
           std::string("a,\xc3\xa9"));
  CHECK_EQ(renderTemplate("{{ 3.14159265 }} {{ .MISSING | default "
                          "10.123456789 }} {{ 100000000000000000000.0 }} "
                          "{{ 1e21 }} {{ 0.00001 }} {{ -0.0 }}"),
           std::string("3.14159265 10.123456789 100000000000000000000 "
                       "1e+21 1e-05 -0"));
  CHECK_EQ(renderTemplate("{{ printf \"%q|%03d|%5.2f|%-4s|%x|%t|%v|%%\" "
                          "\"a\\\"b\" 7 3.14159 \"ab\" 255 true 1.5 }}"),
           std::string("\"a\\\"b\"|007| 3.14|ab  |ff|true|1.5|%"));
  CHECK(fails("{{ printf \"%e\" 1.5 }}"));
  CHECK(fails("{{ printf \"%d\" 1 2 }}"));
  CHECK(fails("{{ loop 1.5 }}"));
  CHECK(fails("{{ loop \" 3\" }}"));
  CHECK(fails("{{ if true }}x"));
  // deliberate leniencies, pinned
  CHECK_EQ(renderTemplate("{{ eq 1 \"1\" }}[{{ .FOO.BAR }}]"
                          "{{ index \"abc\" 1 }}{{ printf \"%d\" \"7\" }}"),
           std::string("true[]987"));
  unsetenv("FOO");
}

static void testEvents() {
  EventCode code;
  CHECK(eventCodeFromString("exitSuccess", &code) &&
        code == EventCode::ExitSuccess);
  CHECK(eventCodeFromString("healthy", &code) &&
        code == EventCode::StatusHealthy);
  CHECK(eventCodeFromString("SIGHUP", &code) && code == EventCode::Signal);
  CHECK(!eventCodeFromString("bogus", &code));
  CHECK_EQ(std::string(eventCodeString(EventCode::StatusChanged)),
           std::string("StatusChanged"));
  Event a{EventCode::Startup, "global"};
  CHECK(a == GlobalStartup);
  CHECK(a != GlobalShutdown);
}

static void testParseArgs() {
  std::string exec, err;
  std::vector<std::string> args;
  CHECK(parseArgs(Json("/bin/to run"), &exec, &args, &err));
  CHECK_EQ(exec, std::string("/bin/to"));
  CHECK_EQ(args.size(), (size_t)1);
  CHECK(parseArgs(Json(JsonArray{Json("/bin/to"), Json("-a"), Json("-b")}),
                  &exec, &args, &err));
  CHECK_EQ(args.size(), (size_t)2);
  CHECK(!parseArgs(Json(""), &exec, &args, &err));
  CHECK_EQ(err, std::string("received zero-length argument"));

  // envName (commands/commands_test.go semantics)
  Command c1("/bin/to-run.sh", {}, Duration(0), false, "");
  CHECK_EQ(c1.envName(), std::string("TO_RUN"));
  Command c2("myjob", {}, Duration(0), false, "");
  CHECK_EQ(c2.envName(), std::string("MYJOB"));
}

static void testIps() {
  std::vector<InterfaceIP> ifaces;
  auto mk = [](const char* name, const char* ip) {
    InterfaceIP i;
    i.name = name;
    i.ip = ip;
    // fill bytes via getIP parse path helper: reuse static parse by spec
    struct in_addr a4;
    if (inet_pton(AF_INET, ip, &a4) == 1) {
      memset(i.bytes, 0, 16);
      i.bytes[10] = 0xff;
      i.bytes[11] = 0xff;
      memcpy(i.bytes + 12, &a4, 4);
      i.ipv6 = false;
    } else {
      struct in6_addr a6;
      inet_pton(AF_INET6, ip, &a6);
      memcpy(i.bytes, &a6, 16);
      i.ipv6 = true;
    }
    return i;
  };
  ifaces.push_back(mk("eth0", "10.2.0.5"));
  ifaces.push_back(mk("eth1", "192.168.1.10"));
  ifaces.push_back(mk("eth1", "192.168.1.11"));
  ifaces.push_back(mk("lo", "127.0.0.1"));

  std::string out, err;
  CHECK(getIP({"eth0"}, ifaces, &out, &err) && out == "10.2.0.5");
  CHECK(getIP({"eth1[1]"}, ifaces, &out, &err) && out == "192.168.1.11");
  CHECK(getIP({"192.168.1.0/24"}, ifaces, &out, &err) &&
        out == "192.168.1.10");
  CHECK(getIP({"inet"}, ifaces, &out, &err) && out == "10.2.0.5");
  CHECK(getIP({"static:192.168.1.100"}, ifaces, &out, &err) &&
        out == "192.168.1.100");
  CHECK(getIP({"bogus0"}, ifaces, &out, &err) == false);
  // default spec list: eth0:inet then inet
  CHECK(getIP({}, ifaces, &out, &err) && out == "10.2.0.5");

  // IPv6 specs
  ifaces.push_back(mk("eth2", "fe80::1234"));
  ifaces.push_back(mk("lo", "::1"));
  std::stable_sort(ifaces.begin(), ifaces.end(),
                   [](const InterfaceIP& a, const InterfaceIP& b) {
                     if (a.name != b.name) return a.name < b.name;
                     return memcmp(a.bytes, b.bytes, 16) < 0;
                   });
  CHECK(getIP({"eth2:inet6"}, ifaces, &out, &err) && out == "fe80::1234");
  CHECK(getIP({"inet6"}, ifaces, &out, &err) && out == "fe80::1234");
  // inet6 wildcard skips ::1 loopback; eth0 has no v6 address
  CHECK(getIP({"eth0:inet6"}, ifaces, &out, &err) == false);

  CHECK(validateServiceName("my-service", &err));
  CHECK(!validateServiceName("", &err));
  CHECK(!validateServiceName("-bad", &err));
  CHECK(!validateServiceName("Bad", &err));
}

static void testConfig() {
  std::string err;
  // minimal valid config
  auto cfg = newConfig(R"({"consul": "localhost:8500",
    jobs: [{name: "hello", exec: "echo hello"}]})", &err);
  CHECK(cfg != nullptr);
  if (cfg) {
    CHECK_EQ(cfg->jobs.size(), (size_t)1);
    CHECK_EQ(cfg->jobs[0]->name, std::string("hello"));
    CHECK_EQ(cfg->stopTimeout, 5);
  }

  // unknown top-level key
  CHECK(newConfig(R"({"consul": "x:8500", "bogus": 1})", &err) == nullptr);
  CHECK(err.find("unknown config keys") != std::string::npos);

  // missing consul
  CHECK(newConfig(R"({jobs: []})", &err) == nullptr);
  CHECK(err.find("no discovery backend defined") != std::string::npos);

  // job validation: port without health
  CHECK(newConfig(R"({"consul": "x:8500",
    jobs: [{name: "svc-a", port: 80}]})", &err) == nullptr);
  CHECK(err.find("health must be set if 'port' is set") != std::string::npos);

  // health requires interval + ttl
  CHECK(newConfig(R"({"consul": "x:8500",
    jobs: [{name: "svc-a", port: 80, health: {ttl: 10}}]})",
                  &err) == nullptr);
  CHECK(err.find("health.interval must be > 0") != std::string::npos);

  // when exclusivity
  CHECK(newConfig(R"({"consul": "x:8500",
    jobs: [{name: "j", exec: "x", when: {once: "startup", each: "changed"}}]})",
                  &err) == nullptr);
  CHECK(err.find("only one of") != std::string::npos);

  // restarts: unlimited with each forbidden
  CHECK(newConfig(R"({"consul": "x:8500",
    jobs: [{name: "j", exec: "x", restarts: "unlimited",
            when: {source: "watch.w", each: "changed"}}]})",
                  &err) == nullptr);
  CHECK(err.find("infinite processes") != std::string::npos);

  // restarts float truncation (jobs/config.go:375-389)
  auto cfg2 = newConfig(R"({"consul": "x:8500",
    jobs: [{name: "j", exec: "x", restarts: 1.2}]})", &err);
  CHECK(cfg2 != nullptr);
  if (cfg2) CHECK_EQ(cfg2->jobs[0]->restartLimit, 1);

  // restarts "never"
  auto cfg3 = newConfig(R"({"consul": "x:8500",
    jobs: [{name: "j", exec: "x", restarts: "never"}]})", &err);
  CHECK(cfg3 && cfg3->jobs[0]->restartLimit == 0);

  // interval job gets unlimited restarts by default + timeout=interval
  auto cfg4 = newConfig(R"({"consul": "x:8500",
    jobs: [{name: "p", exec: "x", when: {interval: "500ms"}}]})", &err);
  CHECK(cfg4 != nullptr);
  if (cfg4) {
    CHECK_EQ(cfg4->jobs[0]->restartLimit, kUnlimited);
    CHECK(cfg4->jobs[0]->freqInterval == std::chrono::milliseconds(500));
    CHECK(cfg4->jobs[0]->execTimeout == std::chrono::milliseconds(500));
  }

  // interval below 1ms rejected
  CHECK(newConfig(R"({"consul": "x:8500",
    jobs: [{name: "p", exec: "x", when: {interval: "100us"}}]})",
                  &err) == nullptr);

  // unnamed jobs are rejected (jobs/config_test.go:243-256)
  CHECK(newConfig(R"({"consul": "x:8500",
    jobs: [{exec: "/bin/echo hi"}]})", &err) == nullptr);
  CHECK(err.find("'name' must not be blank") != std::string::npos);
  // invalid name is permitted if there is no 'port' config
  auto cfg5 = newConfig(R"({"consul": "x:8500",
    jobs: [{name: "myjob_invalid_name", exec: "myexec"}]})", &err);
  CHECK(cfg5 != nullptr);

  // stopping dependency wiring (jobs/config.go:104-113)
  auto cfg6 = newConfig(R"({"consul": "x:8500", jobs: [
    {name: "main-app", exec: "sleep 1", stopTimeout: "2s"},
    {name: "pre-stop", exec: "echo bye",
     when: {source: "main-app", once: "stopping"}}]})", &err);
  CHECK(cfg6 != nullptr);
  if (cfg6) {
    CHECK(cfg6->jobs[0]->stoppingWaitEvent ==
          (Event{EventCode::Stopped, "pre-stop"}));
    CHECK(cfg6->jobs[1]->whenEvent ==
          (Event{EventCode::Stopping, "main-app"}));
  }

  // telemetry synthetic job appended (config/config.go:176-179)
  auto cfg7 = newConfig(R"({"consul": "x:8500",
    telemetry: {port: 19090, interfaces: ["lo"],
      metrics: [{namespace: "app", subsystem: "db", name: "queries",
                 help: "count", type: "counter"}]}})", &err);
  CHECK(cfg7 != nullptr);
  if (cfg7) {
    CHECK_EQ(cfg7->jobs.size(), (size_t)1);
    CHECK_EQ(cfg7->jobs.back()->name, std::string("containerpilot"));
    CHECK(cfg7->jobs.back()->heartbeatInterval == std::chrono::seconds(5));
    CHECK_EQ(cfg7->jobs.back()->ttl, 15);
    CHECK_EQ(cfg7->telemetry->metricConfigs.size(), (size_t)1);
    CHECK_EQ(cfg7->telemetry->metricConfigs[0]->fullName,
             std::string("app_db_queries"));
  }

  // watch config
  auto cfg8 = newConfig(R"({"consul": "x:8500",
    watches: [{name: "backend", interval: 3, tag: "prod"}]})", &err);
  CHECK(cfg8 != nullptr);
  if (cfg8) {
    CHECK_EQ(cfg8->watches[0]->name, std::string("watch.backend"));
    CHECK_EQ(cfg8->watches[0]->serviceName, std::string("backend"));
  }
  CHECK(newConfig(R"({"consul": "x:8500",
    watches: [{name: "backend"}]})", &err) == nullptr);
  CHECK(err.find("interval must be > 0") != std::string::npos);

  // blocking flag: bool (extension), bad values rejected
  auto cfgB = newConfig(R"({"consul": "x:8500",
    watches: [{name: "backend", interval: 5, blocking: true}]})", &err);
  CHECK(cfgB && cfgB->watches[0]->blocking);
  CHECK(newConfig(R"({"consul": "x:8500",
    watches: [{name: "backend", interval: 5, blocking: "nope"}]})",
                  &err) == nullptr);

  // unknown job field rejected (decode.go:15-17 ErrorUnused)
  CHECK(newConfig(R"({"consul": "x:8500",
    jobs: [{name: "j", exec: "x", bogusField: true}]})", &err) == nullptr);
  CHECK(err.find("invalid keys") != std::string::npos);
}

// ---------------------------------------------------------------
// Job state-machine scenarios on a real Loop+Bus (the counterpart of
// jobs/jobs_test.go:15-206's event-sequence assertions against the
// debug ring).

struct JobScenario {
  Loop loop;
  std::shared_ptr<Bus> bus;
  std::vector<std::shared_ptr<Job>> jobs;
  int sigfd = -1;

  JobScenario() {
    bus = std::make_shared<Bus>(loop);
    sigset_t mask;
    sigemptyset(&mask);
    sigaddset(&mask, SIGCHLD);
    sigprocmask(SIG_BLOCK, &mask, nullptr);
    sigfd = signalfd(-1, &mask, SFD_NONBLOCK | SFD_CLOEXEC);
    loop.watchFd(sigfd, EPOLLIN, [this](uint32_t) {
      struct signalfd_siginfo si;
      while (read(sigfd, &si, sizeof(si)) == sizeof(si)) {
      }
      loop.reapChildren();
    });
  }
  ~JobScenario() {
    if (sigfd >= 0) {
      loop.unwatchFd(sigfd);
      close(sigfd);
    }
  }

  std::shared_ptr<Job> addJob(const std::string& jobJson) {
    addJobs("[" + jobJson + "]");
    return jobs.back();
  }

  // parse a full jobs array through newJobConfigs so stopping
  // dependencies get wired (jobs/config.go:99-113)
  void addJobs(const std::string& jobsArrayJson) {
    Json raw = parseJson5(jobsArrayJson);
    std::vector<std::shared_ptr<JobConfig>> cfgs;
    std::string err;
    if (!newJobConfigs(raw, nullptr, &cfgs, &err)) {
      fprintf(stderr, "job config error: %s\n", err.c_str());
      abort();
    }
    for (auto& cfg : cfgs) {
      auto job = std::make_shared<Job>(cfg);
      jobs.push_back(job);
      bus->subscribe(job.get());
    }
  }

  // start all jobs, publish GlobalStartup, run the loop for runMs
  void run(int runMs) {
    for (auto& job : jobs)
      job->run(loop, bus, [] {});
    bus->publish(GlobalStartup);
    loop.addTimeout(std::chrono::milliseconds(runMs),
                    [this] { loop.stop(); });
    loop.run();
  }
};

// probe subscriber recording every event it sees
struct Probe : Subscriber {
  std::vector<Event> events;
  void onEvent(const Event& event) override { events.push_back(event); }
  int count(EventCode code, const std::string& source) const {
    int n = 0;
    for (auto& e : events)
      if (e.code == code && e.source == source) n++;
    return n;
  }
  int indexOf(EventCode code, const std::string& source) const {
    for (size_t i = 0; i < events.size(); i++)
      if (events[i].code == code && events[i].source == source) return (int)i;
    return -1;
  }
};

static void testJobLifecycleSequence() {
  // one-shot job: Startup -> ExitSuccess -> Stopping -> Stopped
  // (jobs_test.go:15-48)
  JobScenario sc;
  Probe probe;
  sc.bus->subscribe(&probe);
  sc.addJob(R"({name: "myjob", exec: "true"})");
  sc.run(1500);
  CHECK_EQ(probe.count(EventCode::ExitSuccess, "myjob"), 1);
  CHECK_EQ(probe.count(EventCode::Stopping, "myjob"), 1);
  CHECK_EQ(probe.count(EventCode::Stopped, "myjob"), 1);
  int iStart = probe.indexOf(EventCode::Startup, "global");
  int iExit = probe.indexOf(EventCode::ExitSuccess, "myjob");
  int iStopping = probe.indexOf(EventCode::Stopping, "myjob");
  int iStopped = probe.indexOf(EventCode::Stopped, "myjob");
  CHECK(iStart < iExit && iExit < iStopping && iStopping < iStopped);
}

static void testJobRestartCounting() {
  // restarts: 2 -> exactly 3 runs (jobs_test.go:127-164)
  JobScenario sc;
  Probe probe;
  sc.bus->subscribe(&probe);
  sc.addJob(R"({name: "flappy", exec: "true", restarts: 2})");
  sc.run(2500);
  CHECK_EQ(probe.count(EventCode::ExitSuccess, "flappy"), 3);
  CHECK_EQ(probe.count(EventCode::Stopped, "flappy"), 1);
}

static void testJobFailedExit() {
  JobScenario sc;
  Probe probe;
  sc.bus->subscribe(&probe);
  sc.addJob(R"({name: "failing", exec: "false", restarts: 1})");
  sc.run(2000);
  CHECK_EQ(probe.count(EventCode::ExitFailed, "failing"), 2);
}

static void testPeriodicJobRuns() {
  // when.interval fires repeatedly (jobs_test.go:166-206)
  JobScenario sc;
  Probe probe;
  sc.bus->subscribe(&probe);
  sc.addJob(R"({name: "tick", exec: "true", when: {interval: "150ms"}})");
  sc.run(1000);
  int runs = probe.count(EventCode::ExitSuccess, "tick");
  CHECK(runs >= 3 && runs <= 8);
}

static void testPreStopJobOnShutdown() {
  // pre-stop jobs get one more run during shutdown (jobs/jobs.go:295-312)
  JobScenario sc;
  Probe probe;
  sc.bus->subscribe(&probe);
  sc.addJobs(R"([
    {name: "main-app", exec: "sleep 30", stopTimeout: "2s"},
    {name: "pre-stop", exec: "true",
     when: {source: "main-app", once: "stopping"}}])");
  sc.loop.addTimeout(std::chrono::milliseconds(300),
                     [&sc] { sc.bus->shutdown(); });
  sc.run(3000);
  CHECK_EQ(probe.count(EventCode::ExitSuccess, "pre-stop"), 1);
  int iPre = probe.indexOf(EventCode::ExitSuccess, "pre-stop");
  int iStopped = probe.indexOf(EventCode::Stopped, "main-app");
  CHECK(iPre >= 0 && iStopped >= 0 && iPre < iStopped);
}

static void testWhenEachFiresRepeatedly() {
  JobScenario sc;
  Probe probe;
  sc.bus->subscribe(&probe);
  sc.addJob(R"({name: "onchange", exec: "true",
                when: {source: "watch.db", each: "changed"}})");
  // fire three synthetic change events, spaced out so the exec finishes
  for (int i = 1; i <= 3; i++) {
    sc.loop.addTimeout(std::chrono::milliseconds(200 * i), [&sc] {
      sc.bus->publish(Event{EventCode::StatusChanged, "watch.db"});
    });
  }
  sc.run(1500);
  CHECK_EQ(probe.count(EventCode::ExitSuccess, "onchange"), 3);
}

static void testDecodeEdges() {
  // weak coercions (config/decode/decode.go ToStrings/WeaklyTypedInput)
  std::vector<std::string> out;
  std::string err;
  CHECK(decode::toStrings(parseJson5("[1, \"a\", true, 2.5]"), &out));
  CHECK_EQ(out.size(), (size_t)4);
  CHECK_EQ(out[0], std::string("1"));
  CHECK_EQ(out[2], std::string("1"));  // bool -> "1"
  CHECK(decode::toStrings(parseJson5("\"solo\""), &out) && out.size() == 1);
  CHECK(decode::toStrings(parseJson5("null"), &out) && out.empty());

  int n = 0;
  CHECK(decode::toInt(parseJson5("\"42\""), &n) && n == 42);
  CHECK(decode::toInt(parseJson5("3.9"), &n) && n == 3);  // truncation
  CHECK(!decode::toInt(parseJson5("\"4x\""), &n));
  bool b = false;
  CHECK(decode::toBool(parseJson5("\"true\""), &b) && b);
  CHECK(!decode::toBool(parseJson5("\"nope\""), &b));

  // template nesting bomb rejects instead of overflowing
  std::string bomb;
  for (int i = 0; i < 5000; i++) bomb += "{{ if 1 }}";
  bool threw = false;
  try {
    renderTemplate(bomb);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
}

static void testDebugRing() {
  // the bus's 10-slot circular debug buffer (events/bus.go:24-54):
  // keeps the last 10 events, drains oldest-first
  Loop loop;
  auto bus = std::make_shared<Bus>(loop);
  for (int i = 0; i < 13; i++)
    bus->publish(Event{EventCode::Metric, "ev-" + std::to_string(i)});
  auto drained = bus->debugEvents();
  CHECK_EQ(drained.size(), (size_t)10);
  CHECK_EQ(drained.front().source, std::string("ev-3"));
  CHECK_EQ(drained.back().source, std::string("ev-12"));
  // drained: a second read is empty
  CHECK_EQ(bus->debugEvents().size(), (size_t)0);
}

static void testMaintenanceMatrix() {
  // maintenance-mode matrix (jobs/jobs_test.go:208-269): health events
  // are suppressed during maintenance and resume after
  JobScenario sc;
  Probe probe;
  sc.bus->subscribe(&probe);
  sc.addJob(R"({name: "svc", exec: "sleep 10",
                health: {exec: "true", interval: "200ms", ttl: 5}})");
  sc.loop.addTimeout(std::chrono::milliseconds(600), [&sc] {
    sc.bus->publish(GlobalEnterMaintenance);
  });
  sc.loop.addTimeout(std::chrono::milliseconds(1400), [&sc] {
    sc.bus->publish(GlobalExitMaintenance);
  });
  int healthyAtEnter = -1, healthyAtExit = -1;
  sc.loop.addTimeout(std::chrono::milliseconds(1300), [&] {
    healthyAtEnter = probe.count(EventCode::StatusHealthy, "svc");
  });
  sc.loop.addTimeout(std::chrono::milliseconds(1450), [&] {
    healthyAtExit = probe.count(EventCode::StatusHealthy, "svc");
  });
  sc.run(2200);
  // some health events before maintenance
  CHECK(healthyAtEnter >= 1);
  // no healthy events published during the maintenance window
  CHECK_EQ(healthyAtExit, healthyAtEnter);
  // and they resume after exitMaintenance
  CHECK(probe.count(EventCode::StatusHealthy, "svc") > healthyAtExit);
}

static void testSignalJobMatrix() {
  // signal-driven jobs fire on their own signal only and repeatedly
  // (jobs/jobs.go:351-357)
  JobScenario sc;
  Probe probe;
  sc.bus->subscribe(&probe);
  sc.addJob(R"({name: "onhup", exec: "true", when: {source: "SIGHUP"}})");
  sc.addJob(R"({name: "onusr2", exec: "true", when: {source: "SIGUSR2"}})");
  for (int i = 1; i <= 2; i++) {
    sc.loop.addTimeout(std::chrono::milliseconds(200 * i),
                       [&sc] { sc.bus->publishSignal("SIGHUP"); });
  }
  sc.loop.addTimeout(std::chrono::milliseconds(500),
                     [&sc] { sc.bus->publishSignal("SIGUSR2"); });
  sc.run(1300);
  CHECK_EQ(probe.count(EventCode::ExitSuccess, "onhup"), 2);
  CHECK_EQ(probe.count(EventCode::ExitSuccess, "onusr2"), 1);
}

static void testStartTimeoutQuitsJob() {
  // when.timeout fires -> TimerExpired{job} published + job quits
  // (jobs/jobs.go:259-264)
  JobScenario sc;
  Probe probe;
  sc.bus->subscribe(&probe);
  sc.addJob(R"({name: "patient", exec: "true",
                when: {source: "ghost", once: "exitSuccess",
                       timeout: "300ms"}})");
  sc.run(1500);
  CHECK_EQ(probe.count(EventCode::ExitSuccess, "patient"), 0);
  CHECK_EQ(probe.count(EventCode::TimerExpired, "patient"), 1);
  CHECK_EQ(probe.count(EventCode::Stopped, "patient"), 1);
}

// ---- HTTP client framing + keep-alive pool (http.cpp) ----
//
// A scripted in-process server: accepts connections on a TCP port and
// answers each request with the next canned raw response, recording how
// many CONNECTIONS it saw — which is what proves (or disproves) reuse.
namespace {

struct ScriptedServer {
  int listenFd = -1;
  int port = 0;
  std::vector<std::string> responses;
  std::atomic<int> connections{0};
  std::atomic<int> requests{0};
  std::atomic<bool> stop{false};
  std::thread thread;

  void start() {
    listenFd = socket(AF_INET, SOCK_STREAM, 0);
    int one = 1;
    setsockopt(listenFd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
    struct sockaddr_in addr;
    memset(&addr, 0, sizeof(addr));
    addr.sin_family = AF_INET;
    addr.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
    CHECK(bind(listenFd, (struct sockaddr*)&addr, sizeof(addr)) == 0);
    socklen_t len = sizeof(addr);
    getsockname(listenFd, (struct sockaddr*)&addr, &len);
    port = ntohs(addr.sin_port);
    CHECK(listen(listenFd, 8) == 0);
    thread = std::thread([this] { serve(); });
  }

  void serve() {
    while (!stop) {
      struct pollfd p{listenFd, POLLIN, 0};
      if (poll(&p, 1, 100) <= 0) continue;
      int fd = accept(listenFd, nullptr, nullptr);
      if (fd < 0) continue;
      struct timeval tv{0, 200000};  // shutdown() must not hang in recv
      setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof(tv));
      connections++;
      // serve requests on this connection until close or script end
      while (!stop) {
        char buf[8192];
        std::string req;
        bool gotReq = false;
        bool peerGone = false;
        while (req.find("\r\n\r\n") == std::string::npos) {
          ssize_t n = recv(fd, buf, sizeof(buf), 0);
          if (n == 0) {
            peerGone = true;
            break;
          }
          if (n < 0) {
            if ((errno == EAGAIN || errno == EWOULDBLOCK) && !stop) continue;
            peerGone = true;
            break;
          }
          req.append(buf, n);
          gotReq = true;
        }
        if (peerGone) break;
        if (!gotReq || req.find("\r\n\r\n") == std::string::npos) break;
        int idx = requests++;
        if (idx >= (int)responses.size()) break;
        const std::string& resp = responses[idx];
        size_t off = 0;
        while (off < resp.size()) {
          ssize_t n = send(fd, resp.data() + off, resp.size() - off,
                           MSG_NOSIGNAL);
          if (n <= 0) break;
          off += n;
        }
        if (resp.find("Connection: close") != std::string::npos) break;
      }
      close(fd);
    }
  }

  void shutdown() {
    stop = true;
    if (thread.joinable()) thread.join();
    if (listenFd >= 0) close(listenFd);
  }
};

}  // namespace

static void testHttpClientFraming() {
  using cpilot::http::request;
  // content-length framing + keep-alive reuse: three requests over ONE
  // connection (the pool holds it between calls)
  {
    ScriptedServer srv;
    std::string ok =
        "HTTP/1.1 200 OK\r\nContent-Type: text/plain\r\n"
        "Content-Length: 5\r\n\r\nhello";
    srv.responses = {ok, ok, ok};
    srv.start();
    std::string target = "127.0.0.1:" + std::to_string(srv.port);
    for (int i = 0; i < 3; i++) {
      auto r = request(target, "GET", "/x", "");
      CHECK(r.ok);
      CHECK_EQ(r.status, 200);
      CHECK_EQ(r.body, std::string("hello"));
    }
    CHECK_EQ(srv.connections.load(), 1);  // reused, not re-connected
    CHECK_EQ(srv.requests.load(), 3);
    srv.shutdown();
  }
  // chunked transfer-encoding is decoded and the connection still reused
  {
    ScriptedServer srv;
    std::string chunked =
        "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n"
        "5\r\nhello\r\n6\r\n world\r\n0\r\n\r\n";
    srv.responses = {chunked, chunked};
    srv.start();
    std::string target = "127.0.0.1:" + std::to_string(srv.port);
    auto r1 = request(target, "GET", "/c", "");
    CHECK(r1.ok);
    CHECK_EQ(r1.body, std::string("hello world"));
    auto r2 = request(target, "GET", "/c", "");
    CHECK(r2.ok);
    CHECK_EQ(r2.body, std::string("hello world"));
    CHECK_EQ(srv.connections.load(), 1);
    srv.shutdown();
  }
  // Connection: close is honored — the next request reconnects
  {
    ScriptedServer srv;
    std::string closing =
        "HTTP/1.1 200 OK\r\nContent-Length: 2\r\n"
        "Connection: close\r\n\r\nok";
    srv.responses = {closing, closing};
    srv.start();
    std::string target = "127.0.0.1:" + std::to_string(srv.port);
    CHECK(request(target, "GET", "/a", "").ok);
    CHECK(request(target, "GET", "/a", "").ok);
    CHECK_EQ(srv.connections.load(), 2);
    srv.shutdown();
  }
  // truncated framed body (server closes mid-body) is an error, not a
  // short success
  {
    ScriptedServer srv;
    srv.responses = {
        "HTTP/1.1 200 OK\r\nContent-Length: 10\r\n"
        "Connection: close\r\n\r\nhalf"};
    srv.start();
    std::string target = "127.0.0.1:" + std::to_string(srv.port);
    auto r = request(target, "GET", "/t", "");
    CHECK(!r.ok);
    CHECK(r.error.find("truncated") != std::string::npos);
    srv.shutdown();
  }
  // stale pooled connection: server restarts between calls; the client
  // retries transparently on a fresh connection
  {
    std::string ok =
        "HTTP/1.1 200 OK\r\nContent-Length: 1\r\n\r\nA";
    int port;
    {
      ScriptedServer srv;
      srv.responses = {ok};
      srv.start();
      port = srv.port;
      std::string target = "127.0.0.1:" + std::to_string(port);
      CHECK(request(target, "GET", "/s", "").ok);  // pools the conn
      srv.shutdown();                              // kills it server-side
    }
    ScriptedServer srv2;
    srv2.responses = {ok};
    srv2.listenFd = socket(AF_INET, SOCK_STREAM, 0);
    int one = 1;
    setsockopt(srv2.listenFd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
    struct sockaddr_in addr;
    memset(&addr, 0, sizeof(addr));
    addr.sin_family = AF_INET;
    addr.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
    addr.sin_port = htons(port);
    CHECK(bind(srv2.listenFd, (struct sockaddr*)&addr, sizeof(addr)) == 0);
    CHECK(listen(srv2.listenFd, 8) == 0);
    srv2.port = port;
    srv2.thread = std::thread([&srv2] { srv2.serve(); });
    std::string target = "127.0.0.1:" + std::to_string(port);
    auto r = request(target, "GET", "/s", "");
    CHECK(r.ok);
    CHECK_EQ(r.body, std::string("A"));
    srv2.shutdown();
  }
}

// ---- HTTP message-head parsing (pure functions, http.hpp) ----

namespace {

// parse a whole request head the way the server does: the head ends just
// past the first blank line
bool parseHead(const std::string& raw, http::Request* req) {
  size_t end = raw.find("\r\n\r\n");
  if (end == std::string::npos) return false;
  return http::parseRequestHead(raw, end + 4, req);
}

// header lines alone, bracketed like a message head
http::Headers parseLines(const std::string& lines) {
  std::string head = "X\r\n" + lines + "\r\n";
  http::Headers h;
  http::parseHeaderLines(head, 3, head.size() - 4, &h);
  return h;
}

}  // namespace

static void testHttpHeadParsing() {
  const size_t kBodyCap = 4 * 1024 * 1024;
  {
    http::Request req;
    CHECK(parseHead("POST /v3/metric?x=1&y=2 HTTP/1.1\r\nHost: a\r\n"
                    "Content-Length: 3\r\n\r\nabc",
                    &req));
    CHECK_EQ(req.method, std::string("POST"));
    CHECK_EQ(req.path, std::string("/v3/metric"));
    CHECK_EQ(req.query, std::string("x=1&y=2"));
    CHECK_EQ(req.headers.size(), (size_t)2);
    CHECK_EQ(req.headers["host"], std::string("a"));
    CHECK_EQ(http::contentLength(req.headers), (size_t)3);
  }
  {
    // the target lies between the first and the last space
    http::Request req;
    CHECK(http::parseRequestLine("GET /a b HTTP/1.1", &req));
    CHECK_EQ(req.method, std::string("GET"));
    CHECK_EQ(req.path, std::string("/a b"));
    CHECK_EQ(req.query, std::string(""));
  }
  {
    http::Request req;
    CHECK(!http::parseRequestLine("GET /x", &req));  // one space
    CHECK(!http::parseRequestLine("GET", &req));
    CHECK(!parseHead("GET /x\r\n\r\n", &req));
  }
  {
    http::Request req;
    CHECK(parseHead("GET / HTTP/1.1\r\n\r\n", &req));
    CHECK_EQ(req.path, std::string("/"));
    CHECK(req.headers.empty());
    CHECK_EQ(http::contentLength(req.headers), (size_t)0);
  }
  // only leading spaces are stripped; tabs and trailing blanks stay
  CHECK_EQ(parseLines("X-A:   v  \r\n")["x-a"], std::string("v  "));
  CHECK_EQ(parseLines("X-B:\tv\r\n")["x-b"], std::string("\tv"));
  {
    // a line without a colon is skipped and later lines still parse
    auto h = parseLines("A: 1\r\ngarbage\r\nB: 2\r\n");
    CHECK_EQ(h.size(), (size_t)2);
    CHECK_EQ(h["a"], std::string("1"));
    CHECK_EQ(h["b"], std::string("2"));
  }
  {
    auto h = parseLines("K: 1\r\nk: 2\r\n");  // the last duplicate wins
    CHECK_EQ(h.size(), (size_t)1);
    CHECK_EQ(h["k"], std::string("2"));
  }
  CHECK_EQ(http::contentLength(parseLines("CONTENT-length: 7\r\n")), (size_t)7);
  CHECK_EQ(http::contentLength(parseLines("Content-Length: abc\r\n")),
           (size_t)0);
  // a negative length wraps far above the body cap (answered 413)
  CHECK(http::contentLength(parseLines("Content-Length: -1\r\n")) > kBodyCap);
  // nothing past the end offset is read as a header
  {
    std::string head = "X\r\nA: 1\r\n\r\nB: 2\r\n\r\n";
    http::Headers h;
    http::parseHeaderLines(head, 3, head.find("\r\n\r\n"), &h);
    CHECK_EQ(h.size(), (size_t)1);
  }

  // client status line
  CHECK_EQ(http::parseStatus("HTTP/1.1 204 No Content\r\n\r\n"), 204);
  CHECK_EQ(http::parseStatus("HTTP/1.1 abc\r\n\r\n"), 0);
  CHECK_EQ(http::parseStatus("HTTP/1.1"), 0);
  CHECK_EQ(http::parseStatus("ICY 200 OK\r\n\r\n"), -1);
  CHECK_EQ(http::parseStatus(""), -1);

  // client chunked detection: any letter case, substring match
  CHECK(http::isChunked(parseLines("Transfer-Encoding: CHUNKED\r\n")));
  CHECK(http::isChunked(parseLines("transfer-encoding: gzip, chunked\r\n")));
  CHECK(!http::isChunked(parseLines("Transfer-Encoding: gzip\r\n")));
  CHECK(!http::isChunked(parseLines("Content-Length: 3\r\n")));
}

// ---- HTTP server + client in one process (http.cpp) ----

namespace {

std::string makeTempDir() {
  char tmpl[] = "/tmp/cpilot-http-XXXXXX";
  const char* dir = mkdtemp(tmpl);
  CHECK(dir != nullptr);
  return dir ? dir : "";
}

// a listening blocker on 127.0.0.1:<port> (0 picks a free one); while it
// is open nobody else can bind the port
int listenBlocker(int* port) {
  int fd = socket(AF_INET, SOCK_STREAM, 0);
  struct sockaddr_in addr;
  memset(&addr, 0, sizeof(addr));
  addr.sin_family = AF_INET;
  addr.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
  addr.sin_port = htons(*port);
  CHECK(bind(fd, (struct sockaddr*)&addr, sizeof(addr)) == 0);
  CHECK(listen(fd, 8) == 0);
  socklen_t len = sizeof(addr);
  getsockname(fd, (struct sockaddr*)&addr, &len);
  *port = ntohs(addr.sin_port);
  return fd;
}

}  // namespace

static void testHttpServerRoundTrip() {
  std::string dir = makeTempDir();
  std::string path = dir + "/s.sock";
  Loop loop;
  http::Server server(loop, [](const http::Request& req) {
    http::Response resp;
    if (req.path == "/missing") {
      resp.status = 404;
      resp.body = "nope\n";
      return resp;
    }
    resp.body = req.method + "|" + req.path + "|" + req.query + "|" + req.body;
    return resp;
  });
  std::string err;
  CHECK(server.listenUnix(path, &err));
  CHECK_EQ(err, std::string(""));

  http::ClientResult post, get, missing;
  ssize_t rawBytes = -1;
  std::thread client([&] {
    std::string target = "unix:" + path;
    post = http::request(target, "POST", "/p?q=1", "body");
    get = http::request(target, "GET", "/g", "");
    missing = http::request(target, "GET", "/missing", "");
    // a request line with one space: closed without a response
    int fd = socket(AF_UNIX, SOCK_STREAM, 0);
    struct sockaddr_un addr;
    memset(&addr, 0, sizeof(addr));
    addr.sun_family = AF_UNIX;
    memcpy(addr.sun_path, path.data(), path.size());
    CHECK(connect(fd, (struct sockaddr*)&addr, sizeof(addr)) == 0);
    const char raw[] = "GET /x\r\n\r\n";
    CHECK_EQ(write(fd, raw, sizeof(raw) - 1), (ssize_t)(sizeof(raw) - 1));
    struct timeval tv{3, 0};  // a server that never closes fails, not hangs
    setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof(tv));
    char buf[64];
    rawBytes = read(fd, buf, sizeof(buf));
    close(fd);
    loop.post([&loop] { loop.stop(); });
  });
  loop.run();
  client.join();
  server.stop();

  CHECK(post.ok);
  CHECK_EQ(post.status, 200);
  CHECK_EQ(post.body, std::string("POST|/p|q=1|body"));
  CHECK(get.ok);
  CHECK_EQ(get.status, 200);
  CHECK_EQ(get.body, std::string("GET|/g||"));
  CHECK(missing.ok);
  CHECK_EQ(missing.status, 404);
  CHECK_EQ(missing.body, std::string("nope\n"));
  CHECK_EQ(rawBytes, (ssize_t)0);  // EOF, zero response bytes

  unlink(path.c_str());
  rmdir(dir.c_str());
}

static void testHttpServerBindRetry() {
  auto noop = [](const http::Request&) { return http::Response{}; };
  // the port is taken at first: the server reports not bound, binds on a
  // retry once the port is free, and then serves
  {
    int port = 0;
    int blocker = listenBlocker(&port);
    Loop loop;
    http::Server server(loop, noop);
    int bound = 0;
    auto listen = [&](std::string* e) {
      return server.listenTcp("127.0.0.1", port, e);
    };
    CHECK(!server.listenRetrying(listen, "test",
                                 "127.0.0.1:" + std::to_string(port),
                                 [&] { bound++; }));
    CHECK_EQ(bound, 0);
    close(blocker);

    http::ClientResult r;
    auto start = Clock::now();
    std::thread client([&] {
      std::string target = "127.0.0.1:" + std::to_string(port);
      while (Clock::now() - start < std::chrono::seconds(3)) {
        r = http::request(target, "GET", "/", "");
        if (r.ok) break;
        usleep(50 * 1000);
      }
      loop.post([&loop] { loop.stop(); });
    });
    loop.run();
    client.join();
    CHECK(r.ok);
    CHECK_EQ(r.status, 200);
    CHECK_EQ(bound, 1);
    CHECK(Clock::now() - start < std::chrono::seconds(3));
    server.stop();
  }
  // stop() while the retry is pending: nothing fires afterwards
  {
    int port = 0;
    int blocker = listenBlocker(&port);
    Loop loop;
    http::Server server(loop, noop);
    int attempts = 0, bound = 0;
    auto listen = [&](std::string* e) {
      attempts++;
      return server.listenTcp("127.0.0.1", port, e);
    };
    CHECK(!server.listenRetrying(listen, "test",
                                 "127.0.0.1:" + std::to_string(port),
                                 [&] { bound++; }));
    CHECK_EQ(attempts, 1);
    server.stop();
    close(blocker);  // a retry that still fired would now bind
    loop.addTimeout(std::chrono::milliseconds(1500), [&loop] { loop.stop(); });
    loop.run();
    CHECK_EQ(attempts, 1);
    CHECK_EQ(bound, 0);
    int again = listenBlocker(&port);  // the port is really free
    close(again);
  }
}

static void testUnixPathTooLong() {
  std::string dir = makeTempDir();
  std::string path = dir + "/" + std::string(200 - dir.size() - 1, 'p');
  CHECK_EQ(path.size(), (size_t)200);
  Loop loop;
  http::Server server(
      loop, [](const http::Request&) { return http::Response{}; });
  std::string err;
  CHECK(!server.listenUnix(path, &err));
  CHECK(err.find("too long") != std::string::npos);
  CHECK(err.find(path) != std::string::npos);

  auto r = http::request("unix:" + path, "GET", "/", "");
  CHECK(!r.ok);
  CHECK(r.error.find("too long") != std::string::npos);

  // neither the path nor its truncation to sun_path's size was created
  CHECK(access(path.c_str(), F_OK) != 0);
  struct sockaddr_un addr;
  CHECK(access(path.substr(0, sizeof(addr.sun_path) - 1).c_str(), F_OK) != 0);
  CHECK_EQ(rmdir(dir.c_str()), 0);  // so the directory is still empty
}

// The shared Go text rules (cpilot/gotext.hpp) on their own: every feature
// that reads text through them is tested elsewhere, through the feature.
// Returns the number of checks made.
static int testGoText() {
  using namespace gotext;
  const int before = checks;
  auto bytes = [](const char* s, size_t n) { return std::string(s, n); };
  auto enc = [](uint32_t cp) {
    std::string out;
    appendUtf8(out, cp);
    return out;
  };

  // ---- UTF-8: the boundary code points of each length ----
  struct Boundary {
    uint32_t cp;
    const char* utf8;
    size_t len;
  };
  const Boundary boundaries[] = {
      {0x7F, "\x7F", 1},         {0x80, "\xC2\x80", 2},
      {0x7FF, "\xDF\xBF", 2},    {0x800, "\xE0\xA0\x80", 3},
      {0xFFFF, "\xEF\xBF\xBF", 3}, {0x10000, "\xF0\x90\x80\x80", 4},
      {0x10FFFF, "\xF4\x8F\xBF\xBF", 4},
  };
  std::string all;
  for (auto& b : boundaries) {
    std::string s(b.utf8, b.len);
    CHECK_EQ(enc(b.cp), s);
    uint32_t cp = 0;
    CHECK_EQ(utf8SeqLen(s, 0, &cp), b.len);
    CHECK_EQ(cp, b.cp);
    CHECK_EQ(utf8SeqLen("x" + s + "x", 1), b.len);
    CHECK_EQ(runeCount(s), (size_t)1);
    all += s;
  }
  std::u32string cps;
  CHECK(decodeUtf8(all, &cps));
  CHECK_EQ(cps.size(), sizeof(boundaries) / sizeof(boundaries[0]));
  CHECK(cps.size() == 7 && cps[0] == 0x7F && cps[3] == 0x800 &&
        cps[6] == 0x10FFFF);
  CHECK_EQ(runeCount(all), (size_t)7);
  CHECK(decodeUtf8("", &cps));
  CHECK(cps.empty());
  CHECK_EQ(runeCount(""), (size_t)0);

  // refused, and each byte of a refused sequence counts as one rune
  const std::string refused[] = {
      "\xED\xA0\x80",      // U+D800 encoded
      "\xED\xBF\xBF",      // U+DFFF encoded
      "\xF4\x90\x80\x80",  // U+110000
      "\xC0\x80",          // overlong 2-byte forms
      "\xC1\xBF",
      "\xE0\x80\x80",      // overlong 3-byte forms
      "\xE0\x9F\xBF",
      "\xF0\x8F\xBF\xBF",  // overlong 4-byte form
      "\xC2",              // truncated at the end of the string
      "\xE2\x80",
      "\xF0\x90\x80",
      "\x80",              // a continuation byte alone
      "\xF8\x88\x80\x80",  // no lead byte
      "\xFF",
      "\xC2\x41",          // lead byte without its continuation
  };
  for (auto& r : refused) {
    CHECK_EQ(utf8SeqLen(r, 0), (size_t)0);
    CHECK_EQ(utf8SeqLen("a" + r, 1), (size_t)0);
    CHECK(!decodeUtf8(r, &cps));
    CHECK(!decodeUtf8("ok" + r, &cps));
    CHECK_EQ(runeCount(r), r.size());
    CHECK_EQ(runeCount("\xE2\x82\xAC" + r), 1 + r.size());
  }

  // ---- white space ----
  const uint32_t spaces[] = {0x09,   0x0A,   0x0B,   0x0C,   0x0D,  0x20,
                             0x85,   0xA0,   0x1680, 0x2000, 0x2005, 0x200A,
                             0x2028, 0x2029, 0x202F, 0x205F, 0x3000};
  std::string everySpace;
  for (uint32_t cp : spaces) {
    CHECK(isSpace(cp));
    std::string sp = enc(cp);
    CHECK_EQ(trimSpace(sp + "x"), std::string("x"));
    CHECK_EQ(trimSpace("x" + sp), std::string("x"));
    CHECK_EQ(trimSpace(sp + "x" + sp), std::string("x"));
    CHECK_EQ(trimSpace(sp + sp + "x y" + sp + sp), std::string("x y"));
    everySpace += sp;
  }
  CHECK_EQ(trimSpace(everySpace), std::string(""));
  CHECK_EQ(trimSpace(everySpace + "x" + everySpace), std::string("x"));
  CHECK_EQ(trimSpace(""), std::string(""));
  CHECK_EQ(trimSpace("x"), std::string("x"));
  // the neighbours of the table's entries are no white space
  const uint32_t nonSpaces[] = {0x08,   0x0E,   0x1F,   0x21,   0x84,  0x86,
                                0x9F,   0xA1,   0x167F, 0x1681, 0x180E, 0x1FFF,
                                0x200B, 0x200C, 0x2027, 0x202A, 0x202E, 0x2030,
                                0x205E, 0x2060, 0x2FFF, 0x3001, 0xFEFF};
  for (uint32_t cp : nonSpaces) {
    CHECK(!isSpace(cp));
    std::string kept = enc(cp) + "x" + enc(cp);
    CHECK_EQ(trimSpace(kept), kept);
    CHECK_EQ(trimSpace(" " + kept + "\t"), kept);
    CHECK_EQ(trimSpace("\xE2\x80\x83" + kept + "\xC2\xA0"), kept);
  }
  // a malformed byte is no space: it stays and the trimming stops there
  const std::string malformed[] = {
      "\x85",      // the bytes of U+0085 and U+00A0 without their lead byte
      "\xA0",
      "\xC2",      // a lead byte whose continuation is missing
      "\xE2\x80",  // two thirds of U+2000..U+200A
      "\xC0\xA0",  // U+0020 in an overlong form
  };
  for (auto& m : malformed) {
    CHECK_EQ(trimSpace(" x " + m), "x " + m);
    CHECK_EQ(trimSpace(m + " x "), m + " x");
    CHECK_EQ(trimSpace(" " + m + " "), m);
    CHECK_EQ(trimSpace("\xC2\xA0 " + m), m);
  }
  CHECK_EQ(trimSpace(bytes(" \0 ", 3)), bytes("\0", 1));
  CHECK_EQ(trimSpace(bytes(" a \0 b ", 7)), bytes("a \0 b", 5));

  // ---- strconv.Atoi ----
  auto atoiOf = [](const char* s, int64_t want) {
    int64_t got = want ^ 1;
    return atoi(s, &got) && got == want;
  };
  auto atoiRefuses = [](const std::string& s) {
    int64_t got = 0;
    return !atoi(s, &got);
  };
  CHECK(atoiOf("0", 0));
  CHECK(atoiOf("-0", 0));
  CHECK(atoiOf("+7", 7));
  CHECK(atoiOf("007", 7));
  CHECK(atoiOf("9223372036854775807", INT64_MAX));
  CHECK(atoiOf("-9223372036854775808", INT64_MIN));
  CHECK(atoiRefuses("9223372036854775808"));
  CHECK(atoiRefuses("-9223372036854775809"));
  CHECK(atoiRefuses("99999999999999999999"));
  CHECK(atoiRefuses(""));
  CHECK(atoiRefuses("+"));
  CHECK(atoiRefuses("-"));
  CHECK(atoiRefuses("1 "));
  CHECK(atoiRefuses(" 1"));
  CHECK(atoiRefuses("1_0"));
  CHECK(atoiRefuses("0x1"));
  CHECK(atoiRefuses("1.0"));
  CHECK(atoiRefuses("--1"));
  CHECK(atoiRefuses(bytes("1\0", 2)));

  // ---- hex digits ----
  CHECK_EQ(hexVal('0'), 0);
  CHECK_EQ(hexVal('9'), 9);
  CHECK_EQ(hexVal('a'), 10);
  CHECK_EQ(hexVal('f'), 15);
  CHECK_EQ(hexVal('A'), 10);
  CHECK_EQ(hexVal('F'), 15);
  for (char c : {'g', 'G', '/', ':', '@', '`', ' ', '\0', '\xE9'})
    CHECK_EQ(hexVal(c), -1);

  // ---- the decimal float grammar ----
  for (const char* s : {"0", "12", ".5", "5.", "1.5", "1e5", "1E5", "1e+5",
                        "1e-5", ".5e1", "5.e1", "007"})
    CHECK(isDecimalFloat(s));
  for (const char* s : {"", ".", "e5", ".e5", "1e", "1e+", "1e-", "+1", "-1",
                        "1 ", " 1", "0x1", "1_0", "1.2.3", "1e5.0", "1f",
                        "inf", "nan"})
    CHECK(!isDecimalFloat(s));
  CHECK(!isDecimalFloat(bytes("1\0", 2)));

  // ---- strconv.ParseFloat ----
  auto floatOf = [](const std::string& s, double want) {
    double got = 0;
    if (!parseFloat(s, &got)) return false;
    if (std::isnan(want)) return std::isnan(got);
    return got == want && std::signbit(got) == std::signbit(want);
  };
  auto floatRefuses = [](const std::string& s) {
    double got = 0;
    return !parseFloat(s, &got);
  };
  const double inf = std::numeric_limits<double>::infinity();
  CHECK(floatOf("1", 1));
  CHECK(floatOf("7.5", 7.5));
  CHECK(floatOf(".5", 0.5));
  CHECK(floatOf("5.", 5));
  CHECK(floatOf("+5", 5));
  CHECK(floatOf("-0", -0.0));
  CHECK(floatOf("1E1", 10));
  CHECK(floatOf("1e-999", 0));
  CHECK(floatOf("-1e-999", -0.0));
  CHECK(floatOf("1.7976931348623157e308", std::numeric_limits<double>::max()));
  CHECK(floatOf("inf", inf));
  CHECK(floatOf("+Infinity", inf));
  CHECK(floatOf("-INF", -inf));
  CHECK(floatOf("NaN", std::numeric_limits<double>::quiet_NaN()));
  CHECK(floatRefuses(""));
  CHECK(floatRefuses(" "));
  CHECK(floatRefuses(" 1"));  // trimming is the caller's business
  CHECK(floatRefuses("1 "));
  CHECK(floatRefuses("0x1p3"));
  CHECK(floatRefuses("0x10"));
  CHECK(floatRefuses("1_000"));
  CHECK(floatRefuses("nan(x)"));
  CHECK(floatRefuses("+nan"));
  CHECK(floatRefuses("-nan"));
  CHECK(floatRefuses("--1"));
  CHECK(floatRefuses("+"));
  CHECK(floatRefuses("."));
  CHECK(floatRefuses("1e"));
  CHECK(floatRefuses("1e+"));
  CHECK(floatRefuses("e5"));
  CHECK(floatRefuses("1e999"));
  CHECK(floatRefuses("-1e999"));
  CHECK(floatRefuses("1 2"));
  CHECK(floatRefuses("infinit"));
  CHECK(floatRefuses(bytes("1\0" "2", 3)));
  CHECK(floatRefuses(bytes("inf\0", 4)));

  // ---- the rule of health.interval and the sensors' durations ----
  auto positive = [](const char* json5, int64_t wantMs) {
    Duration got{0};
    return parsePositiveDuration(parseJson5(json5), &got) &&
           got == std::chrono::milliseconds(wantMs);
  };
  auto notPositive = [](const char* json5) {
    Duration got{0};
    return !parsePositiveDuration(parseJson5(json5), &got);
  };
  CHECK(positive("1", 1000));
  CHECK(positive("\"1\"", 1000));
  CHECK(positive("\"500ms\"", 500));
  CHECK(positive("\"1ms\"", 1));
  CHECK(positive("\"1m30s\"", 90000));
  CHECK(notPositive("\"999us\""));
  CHECK(notPositive("\"0\""));
  CHECK(notPositive("0"));
  CHECK(notPositive("-1"));
  CHECK(notPositive("\"\""));
  CHECK(notPositive("\"ms\""));
  CHECK(notPositive("\".5s\""));
  CHECK(notPositive("\"+5s\""));
  CHECK(notPositive("\"5\\u00a0s\""));
  CHECK(notPositive("1.5"));
  CHECK(notPositive("true"));
  CHECK(notPositive("null"));
  CHECK(notPositive("[1]"));
  CHECK(notPositive("9223372037"));
  return checks - before;
}

int main() {
  testJson5();
  testDurations();
  testTemplate();
  testEvents();
  testParseArgs();
  testIps();
  testConfig();
  testJobLifecycleSequence();
  testJobRestartCounting();
  testJobFailedExit();
  testPeriodicJobRuns();
  testPreStopJobOnShutdown();
  testWhenEachFiresRepeatedly();
  testDecodeEdges();
  testDebugRing();
  testMaintenanceMatrix();
  testSignalJobMatrix();
  testStartTimeoutQuitsJob();
  testHttpClientFraming();
  testHttpHeadParsing();
  testHttpServerRoundTrip();
  testHttpServerBindRetry();
  testUnixPathTooLong();
  int goTextChecks = testGoText();
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("all unit tests passed (%d checks, %d of them in testGoText)\n",
         checks.load(), goTextChecks);
  return 0;
}
