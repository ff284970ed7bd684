// Tests for the native telemetry sensors (cpilot/sensor.hpp): the
// extraction table, counter deltas, the file source against files made
// here in a temp dir, and the engine on a real Loop and Bus against a
// listener opened here on 127.0.0.1.
// Run via `bin/cpilot_sensortests`; exits non-zero if any check failed.
#include <arpa/inet.h>
#include <dirent.h>
#include <fcntl.h>
#include <netinet/in.h>
#include <sys/epoll.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "cpilot/events.hpp"
#include "cpilot/json.hpp"
#include "cpilot/log.hpp"
#include "cpilot/loop.hpp"
#include "cpilot/sensor.hpp"

using namespace cpilot;
using namespace cpilot::sensor;
using std::chrono::milliseconds;

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

// ---------------- extraction ----------------

RecordSpec record(const std::string& json5) {
  RecordSpec rec;
  std::string key, err;
  if (!parseRecord(parseJson5(json5), &rec, &key, &err)) {
    fprintf(stderr, "bad record %s: %s %s\n", json5.c_str(), key.c_str(),
            err.c_str());
    exit(1);
  }
  return rec;
}

void expectValue(const std::string& body, const std::string& rec, double want,
                 int line) {
  double got = 0;
  std::string reason;
  bool ok = extract(body, record(rec), &got, &reason);
  if (!ok || memcmp(&got, &want, sizeof(got)) != 0) {
    fprintf(stderr, "FAIL %s:%d: %s -> %s%.17g, want %.17g\n", __FILE__, line,
            rec.c_str(), ok ? "" : (reason + " / ").c_str(), got, want);
    failures++;
  }
}

void expectReason(const std::string& body, const std::string& rec,
                  const std::string& want, int line) {
  double got = 0;
  std::string reason;
  bool ok = extract(body, record(rec), &got, &reason);
  if (ok || reason != want) {
    fprintf(stderr, "FAIL %s:%d: %s -> %s, want reason '%s'\n", __FILE__, line,
            rec.c_str(), ok ? "a value" : ("'" + reason + "'").c_str(),
            want.c_str());
    failures++;
  }
}
#define VALUE(body, rec, want) expectValue(body, rec, want, __LINE__)
#define REASON(body, rec, want) expectReason(body, rec, want, __LINE__)

const char* kMeminfo =
    "MemTotal:       263856972 kB\n"
    "MemFree:        12345678 kB\n"
    "MemAvailable:   200000000 kB\n";
const char* kStub =
    "Active connections: 291 \r\n"
    "server accepts handled requests\r\n"
    " 16630948 16630948 31070465 \r\n"
    "Reading: 6 Writing: 179 Waiting: 106 \r\n";
const char* kJson =
    "{\"queue\": {\"depth\": 7, \"a/b\": 1.5, \"m~n\": \"  42 \", "
    "\"list\": [10, [20, 30], {\"x\": -4}]}, \"name\": \"app\", "
    "\"up\": true, \"none\": null, \"\": 9}";

void testExtraction() {
  const std::string m = "{metric: 'm', ";
  // whole body
  VALUE("12345\n", "{metric: 'm'}", 12345.0);
  VALUE("  \t-1.5e3\r\n", "{metric: 'm'}", -1500.0);
  VALUE("0x10", "{metric: 'm'}", 16.0);
  VALUE("7", "{metric: 'm', scale: 0.5}", 3.5);
  REASON("", "{metric: 'm'}", "not a number: \"\"");
  REASON(" \n", "{metric: 'm'}", "not a number: \"\"");
  REASON("12 kB", "{metric: 'm'}", "not a number: \"12 kB\"");
  REASON("12x", "{metric: 'm'}", "not a number: \"12x\"");
  REASON("nan", "{metric: 'm'}", "not a number: \"nan\"");
  REASON("inf", "{metric: 'm'}", "not a number: \"inf\"");
  REASON("-Infinity", "{metric: 'm'}", "not a number: \"-Infinity\"");
  REASON("1e999", "{metric: 'm'}", "not a number: \"1e999\"");
  REASON(std::string("1\0002", 3), "{metric: 'm'}",
         "not a number: \"1\\02\"");  // NUL shown as \0
  REASON(std::string(100, '9') + "x", "{metric: 'm'}",
         "not a number: \"" + std::string(64, '9') + "...\"");
  REASON("1e308", "{metric: 'm', scale: 100}", "value out of range");

  // line prefix
  VALUE(kMeminfo, m + "line: 'MemAvailable:', field: 2, scale: 1024}",
        200000000.0 * 1024);
  VALUE(kMeminfo, m + "line: 'Mem', field: 2}", 263856972.0);  // first match
  VALUE("  \tkey 5\n", m + "line: 'key', field: 2}", 5.0);
  VALUE("x\n\nkey: 9", m + "line: 'key:', field: 2}", 9.0);  // no final \n
  VALUE("5 apples", m + "line: '5'}", 5.0);  // field defaults to 1
  REASON(kMeminfo, m + "line: 'SwapFree:', field: 2}",
         "no line starts with \"SwapFree:\"");
  REASON(kMeminfo, m + "line: 'MemFree:', field: 4}", "line has 3 fields");
  REASON(kMeminfo, m + "line: 'MemFree:', field: 3}",
         "not a number: \"kB\"");
  REASON(kMeminfo, m + "line: 'MemFree:'}", "not a number: \"MemFree:\"");
  REASON("", m + "line: 'a'}", "no line starts with \"a\"");

  // line number, CRLF
  VALUE(kStub, m + "lineNumber: 3, field: 1}", 16630948.0);
  VALUE(kStub, m + "lineNumber: 3, field: 3}", 31070465.0);
  VALUE(kStub, m + "lineNumber: 1, field: 3}", 291.0);
  VALUE(kStub, m + "lineNumber: 4, field: 6}", 106.0);
  VALUE(kStub, m + "line: 'Reading:', field: 4}", 179.0);
  VALUE("1\n2\n3", m + "lineNumber: 3}", 3.0);
  REASON(kStub, m + "lineNumber: 5}", "no line 5");
  REASON("1\n2\n", m + "lineNumber: 3}", "no line 3");
  REASON("", m + "lineNumber: 1}", "no line 1");
  REASON("1\n\n3\n", m + "lineNumber: 2}", "line has 0 fields");
  REASON(kStub, m + "lineNumber: 3, field: 4}", "line has 3 fields");
  REASON(kStub, m + "lineNumber: 2}", "not a number: \"server\"");

  // json pointer
  VALUE(kJson, m + "json: '/queue/depth'}", 7.0);
  VALUE(kJson, m + "json: '/queue/a~1b', scale: 2}", 3.0);
  VALUE(kJson, m + "json: '/queue/m~0n'}", 42.0);
  VALUE(kJson, m + "json: '/queue/list/0'}", 10.0);
  VALUE(kJson, m + "json: '/queue/list/1/1'}", 30.0);
  VALUE(kJson, m + "json: '/queue/list/2/x'}", -4.0);
  VALUE(kJson, m + "json: '/'}", 9.0);  // the empty key
  VALUE("  3.25\r\n", m + "json: ''}", 3.25);  // the whole document
  REASON(kJson, m + "json: '/queue/missing'}",
         "json: no value at /queue/missing");
  REASON(kJson, m + "json: '/queue/list/3'}",
         "json: no value at /queue/list/3");
  REASON(kJson, m + "json: '/queue/list/01'}",
         "json: no value at /queue/list/01");
  REASON(kJson, m + "json: '/queue/list/-'}",
         "json: no value at /queue/list/-");
  REASON(kJson, m + "json: '/queue/depth/x'}",
         "json: no value at /queue/depth/x");
  REASON(kJson, m + "json: '/name'}", "not a number: \"app\"");
  REASON(kJson, m + "json: '/up'}", "not a number: \"bool\"");
  REASON(kJson, m + "json: '/none'}", "not a number: \"null\"");
  REASON(kJson, m + "json: '/queue'}", "not a number: \"object\"");
  REASON(kJson, m + "json: '/queue/list'}", "not a number: \"array\"");
  REASON("", m + "json: '/a'}", "json: unexpected end of input");
  REASON("{\"a\": 1} x", m + "json: '/a'}",
         "json: unexpected trailing characters");
  REASON("{\"a\": ", m + "json: '/a'}", "json: unexpected end of input");

  // record config errors
  auto bad = [](const std::string& json5, const std::string& wantKey) {
    RecordSpec rec;
    std::string key, err;
    bool ok = parseRecord(parseJson5(json5), &rec, &key, &err);
    if (ok || key != wantKey) {
      fprintf(stderr, "FAIL record %s: key '%s', want '%s'\n", json5.c_str(),
              key.c_str(), wantKey.c_str());
      failures++;
    }
  };
  bad("{}", ".metric");
  bad("{metric: 'm', line: 'a', lineNumber: 1}", ".line");
  bad("{metric: 'm', json: '/a', line: 'a'}", ".json");
  bad("{metric: 'm', json: '/a', field: 2}", ".json");
  bad("{metric: 'm', json: 'a'}", ".json");
  bad("{metric: 'm', json: '/a~2'}", ".json");
  bad("{metric: 'm', field: 2}", ".field");
  bad("{metric: 'm', lineNumber: 0}", ".lineNumber");
  bad("{metric: 'm', line: 'a', field: 0}", ".field");
  bad("{metric: 'm', scale: 'x'}", ".scale");
  bad("{metric: 'm', scale: Infinity}", ".scale");
  bad("{metric: 'm', regex: 'x'}", "");

  CHECK_EQ(formatValue(0.1), std::string("0.1"));
  CHECK_EQ(formatValue(5), std::string("5"));
  CHECK_EQ(formatValue(204800000000.0), std::string("204800000000"));
  CHECK_EQ(formatValue(2.5e20), std::string("2.5e+20"));
  CHECK_EQ(formatValue(1.0 / 3), std::string("0.3333333333333333"));
}

// ---------------- counter ----------------

void testCounter() {
  CounterBaseline c;
  double d = -1;
  CHECK(!c.feed(10, &d));  // baseline
  CHECK(c.feed(15, &d));
  CHECK_EQ(d, 5.0);
  CHECK(c.feed(3, &d));  // a reset: the new value
  CHECK_EQ(d, 3.0);
  CHECK(c.feed(3, &d));
  CHECK_EQ(d, 0.0);
  c.reset();
  CHECK(!c.feed(100, &d));  // baseline again
  CHECK(c.feed(101, &d));
  CHECK_EQ(d, 1.0);
}

// ---------------- file source ----------------

std::string tmpDir;

void writeFile(const std::string& path, const std::string& data) {
  std::string tmp = path + ".tmp";
  FILE* f = fopen(tmp.c_str(), "wb");
  if (!f) {
    perror("fopen");
    exit(1);
  }
  fwrite(data.data(), 1, data.size(), f);
  fclose(f);
  rename(tmp.c_str(), path.c_str());
}

void testFileSource() {
  std::string body, reason;
  CHECK(!readFileSource(tmpDir + "/missing", &body, &reason));
  CHECK_EQ(reason, std::string("open: No such file or directory"));

  CHECK(!readFileSource(tmpDir, &body, &reason));
  CHECK_EQ(reason, std::string("not a regular file"));

  std::string fifo = tmpDir + "/fifo";
  CHECK(mkfifo(fifo.c_str(), 0600) == 0);
  TimePoint t0 = Clock::now();
  CHECK(!readFileSource(fifo, &body, &reason));  // no writer: must not hang
  CHECK_EQ(reason, std::string("not a regular file"));
  CHECK(Clock::now() - t0 < milliseconds(1000));

  std::string big = tmpDir + "/big";
  writeFile(big, std::string(kMaxSourceBytes + 1, '1'));
  CHECK(!readFileSource(big, &body, &reason));
  CHECK_EQ(reason, std::string("source too large"));
  CHECK(body.empty());

  writeFile(big, std::string(kMaxSourceBytes, '1'));
  CHECK(readFileSource(big, &body, &reason));
  CHECK_EQ(body.size(), kMaxSourceBytes);
  unlink(big.c_str());

  writeFile(tmpDir + "/value", "42\n");
  CHECK(readFileSource(tmpDir + "/value", &body, &reason));
  CHECK_EQ(body, std::string("42\n"));

  // procfs reports size 0: still read to EOF
  CHECK(readFileSource("/proc/self/stat", &body, &reason));
  CHECK(!body.empty());
}

// ---------------- engine ----------------

struct Recorder : Subscriber {
  std::vector<Event> events;
  void onEvent(const Event& e) override { events.push_back(e); }
};

int countOpenFds() {
  int n = 0;
  DIR* d = opendir("/proc/self/fd");
  if (!d) return -1;
  while (struct dirent* e = readdir(d))
    if (e->d_name[0] != '.') n++;
  closedir(d);
  return n;
}

void runLoop(Loop& loop, int ms, std::function<bool()> done = nullptr) {
  uint64_t deadline = loop.addTimeout(milliseconds(ms), [&] { loop.stop(); });
  uint64_t poll = 0;
  if (done)
    poll = loop.addInterval(milliseconds(1), [&] {
      if (done()) loop.stop();
    });
  loop.run();
  loop.cancelTimer(deadline);
  if (poll) loop.cancelTimer(poll);
}

// A scripted HTTP peer on 127.0.0.1 served from the test's loop; the
// sensor's fetch runs on a worker thread, so both make progress.
struct Server {
  Loop& loop;
  std::string reply;  // full response bytes
  int delayMs;        // < 0: never answer
  int lfd = -1;
  int port = 0;
  int requests = 0;
  std::map<int, std::string> in;
  std::vector<uint64_t> timers;

  Server(Loop& l, std::string r, int delay = 0)
      : loop(l), reply(std::move(r)), delayMs(delay) {
    lfd = socket(AF_INET, SOCK_STREAM | SOCK_NONBLOCK | SOCK_CLOEXEC, 0);
    struct sockaddr_in addr;
    memset(&addr, 0, sizeof(addr));
    addr.sin_family = AF_INET;
    addr.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
    socklen_t len = sizeof(addr);
    if (bind(lfd, (struct sockaddr*)&addr, sizeof(addr)) != 0 ||
        listen(lfd, 64) != 0 ||
        getsockname(lfd, (struct sockaddr*)&addr, &len) != 0) {
      perror("test listener");
      exit(1);
    }
    port = ntohs(addr.sin_port);
    loop.watchFd(lfd, EPOLLIN, [this](uint32_t) { onAccept(); });
  }

  ~Server() {
    for (uint64_t t : timers) loop.cancelTimer(t);
    std::vector<int> fds;
    for (auto& kv : in) fds.push_back(kv.first);
    for (int fd : fds) closeConn(fd);
    loop.unwatchFd(lfd);
    close(lfd);
  }

  void closeConn(int fd) {
    if (!in.count(fd)) return;
    loop.unwatchFd(fd);
    close(fd);
    in.erase(fd);
  }

  void onAccept() {
    while (true) {
      int fd = accept4(lfd, nullptr, nullptr, SOCK_NONBLOCK | SOCK_CLOEXEC);
      if (fd < 0) return;
      in[fd] = "";
      loop.watchFd(fd, EPOLLIN, [this, fd](uint32_t) { onData(fd); });
    }
  }

  void answer(int fd) {
    if (!in.count(fd)) return;
    ssize_t unused = send(fd, reply.data(), reply.size(), MSG_NOSIGNAL);
    (void)unused;
    closeConn(fd);
  }

  void onData(int fd) {
    char buf[4096];
    bool had = in[fd].find("\r\n\r\n") != std::string::npos;
    while (true) {
      ssize_t n = recv(fd, buf, sizeof(buf), 0);
      if (n > 0) {
        in[fd].append(buf, (size_t)n);
        continue;
      }
      if (n < 0 && (errno == EAGAIN || errno == EINTR)) break;
      closeConn(fd);  // peer closed or reset
      return;
    }
    if (had || in[fd].find("\r\n\r\n") == std::string::npos) return;
    requests++;
    if (delayMs < 0) return;
    if (delayMs == 0) {
      answer(fd);
      return;
    }
    timers.push_back(
        loop.addTimeout(milliseconds(delayMs), [this, fd] { answer(fd); }));
  }
};

std::string httpReply(int code, const std::string& body) {
  return "HTTP/1.1 " + std::to_string(code) +
         " X\r\nContent-Length: " + std::to_string(body.size()) +
         "\r\nConnection: close\r\n\r\n" + body;
}

std::shared_ptr<SensorSpec> specFor(const std::string& json5) {
  std::map<std::string, prom::MetricType> metrics = {
      {"t_g_a", prom::MetricType::Gauge},
      {"t_g_b", prom::MetricType::Gauge},
      {"t_c_n", prom::MetricType::Counter}};
  std::vector<std::shared_ptr<SensorSpec>> out;
  std::string err;
  if (!newSensorSpecs(parseJson5("[" + json5 + "]"), metrics, &out, &err) ||
      out.size() != 1) {
    fprintf(stderr, "bad sensor %s: %s\n", json5.c_str(), err.c_str());
    exit(1);
  }
  return out[0];
}

std::string httpSensor(const Server& s, const std::string& rest) {
  return "{name: 'web', http: 'http://127.0.0.1:" + std::to_string(s.port) +
         "/stats', " + rest + "}";
}

struct Rig {
  Loop loop;
  std::shared_ptr<Bus> bus = std::make_shared<Bus>(loop);
  Recorder rec;
  WorkerPool pool{2};
  Rig() { bus->subscribe(&rec); }
  ~Rig() {
    pool.stop();
    if (bus) bus->unsubscribe(&rec);
  }
  std::vector<std::string> sources() const {
    std::vector<std::string> out;
    for (auto& e : rec.events) {
      CHECK(e.code == EventCode::Metric);
      out.push_back(e.source);
    }
    return out;
  }
};

void testEnginePeriodicFile() {
  Rig rig;
  std::string path = tmpDir + "/gauge";
  writeFile(path, "key 10 20\n");
  auto s = std::make_shared<Sensor>(
      specFor("{name: 'ff', file: '" + path + "', interval: '20ms', record: ["
              "{metric: 't_g_a', line: 'key', field: 2},"
              "{metric: 't_g_b', line: 'key', field: 3, scale: 2},"
              "{metric: 't_c_n', line: 'key', field: 2}]}"),
      nullptr);
  s->start(rig.loop, rig.bus, &rig.pool);
  runLoop(rig.loop, 2000, [&] { return s->okCount() >= 2; });
  writeFile(path, "key 13 20\n");
  uint64_t seen = s->okCount();
  runLoop(rig.loop, 2000, [&] { return s->okCount() >= seen + 2; });
  s->stop();
  runLoop(rig.loop, 30);
  CHECK_EQ(s->errorCount(), (uint64_t)0);
  auto got = rig.sources();
  // first sample: both gauges, the counter only sets its baseline
  CHECK(got.size() >= 8);
  if (got.size() >= 5) {
    CHECK_EQ(got[0], std::string("t_g_a|10"));
    CHECK_EQ(got[1], std::string("t_g_b|40"));
    CHECK_EQ(got[2], std::string("t_g_a|10"));
    CHECK_EQ(got[3], std::string("t_g_b|40"));
    CHECK_EQ(got[4], std::string("t_c_n|0"));
  }
  int jumps = 0;
  for (auto& g : got)
    if (g == "t_c_n|3") jumps++;
  CHECK_EQ(jumps, 1);
  size_t n = rig.rec.events.size();
  runLoop(rig.loop, 60);
  CHECK_EQ(rig.rec.events.size(), n);  // stopped means stopped

  // a restart forgets the counter baseline
  s->start(rig.loop, rig.bus, &rig.pool);
  rig.rec.events.clear();
  runLoop(rig.loop, 2000, [&] { return rig.rec.events.size() >= 2; });
  s->stop();
  got = rig.sources();
  CHECK(got.size() >= 2);
  if (got.size() >= 2) {
    CHECK_EQ(got[0], std::string("t_g_a|13"));
    CHECK_EQ(got[1], std::string("t_g_b|40"));
  }
}

void testEnginePartialFailure() {
  Rig rig;
  std::string path = tmpDir + "/partial";
  writeFile(path, "a 1\nb x\n");
  auto s = std::make_shared<Sensor>(
      specFor("{name: 'pp', file: '" + path + "', interval: '10ms', record: ["
              "{metric: 't_g_a', line: 'b', field: 2},"
              "{metric: 't_g_b', line: 'a', field: 2}]}"),
      nullptr);
  s->start(rig.loop, rig.bus, &rig.pool);
  runLoop(rig.loop, 2000, [&] { return s->errorCount() >= 1; });
  s->stop();
  runLoop(rig.loop, 20);
  CHECK_EQ(s->okCount(), (uint64_t)0);
  auto got = rig.sources();
  CHECK(!got.empty());
  for (auto& g : got) CHECK_EQ(g, std::string("t_g_b|1"));
}

void testEngineHttp() {
  Rig rig;
  Server srv(rig.loop, httpReply(200, "{\"q\": {\"d\": 4}, \"n\": \"2.5\"}"));
  auto s = std::make_shared<Sensor>(
      specFor(httpSensor(srv, "interval: '20ms', record: ["
                              "{metric: 't_g_a', json: '/q/d'},"
                              "{metric: 't_g_b', json: '/n'}]")),
      nullptr);
  s->start(rig.loop, rig.bus, &rig.pool);
  runLoop(rig.loop, 2000, [&] { return s->okCount() >= 3; });
  s->stop();
  runLoop(rig.loop, 30);
  auto got = rig.sources();
  CHECK(got.size() >= 6);
  for (size_t i = 0; i + 1 < got.size(); i += 2) {
    CHECK_EQ(got[i], std::string("t_g_a|4"));
    CHECK_EQ(got[i + 1], std::string("t_g_b|2.5"));
  }
  // one fetch per sample, not one per record
  // (a fetch that stop() cut off was requested but never became a sample)
  uint64_t samples = s->okCount() + s->errorCount();
  CHECK((uint64_t)srv.requests == samples ||
        (uint64_t)srv.requests == samples + 1);
}

void testEngineHttpStatus() {
  Rig rig;
  Server srv(rig.loop, httpReply(503, "7"));
  auto s = std::make_shared<Sensor>(
      specFor(httpSensor(srv, "interval: '10ms', record: [{metric: 't_g_a'}]")),
      nullptr);
  s->start(rig.loop, rig.bus, &rig.pool);
  runLoop(rig.loop, 2000, [&] { return s->errorCount() >= 2; });
  s->stop();
  CHECK_EQ(s->okCount(), (uint64_t)0);
  CHECK(rig.rec.events.empty());
}

void testEngineHttpTooLarge() {
  Rig rig;
  Server srv(rig.loop,
             httpReply(200, std::string(kMaxSourceBytes + 1, '1')));
  auto s = std::make_shared<Sensor>(
      specFor(httpSensor(srv, "interval: '10ms', timeout: '2s', "
                              "record: [{metric: 't_g_a'}]")),
      nullptr);
  s->start(rig.loop, rig.bus, &rig.pool);
  runLoop(rig.loop, 3000, [&] { return s->errorCount() >= 1; });
  s->stop();
  CHECK_EQ(s->okCount(), (uint64_t)0);
  CHECK(s->errorCount() >= 1);
  CHECK(rig.rec.events.empty());
}

void testEngineSkipWhileInFlight() {
  Rig rig;
  Server srv(rig.loop, httpReply(200, "5"), /*delayMs=*/120);
  auto s = std::make_shared<Sensor>(
      specFor(httpSensor(srv, "interval: '20ms', timeout: '1s', "
                              "record: [{metric: 't_g_a'}]")),
      nullptr);
  s->start(rig.loop, rig.bus, &rig.pool);
  runLoop(rig.loop, 3000, [&] { return s->okCount() >= 2; });
  s->stop();
  runLoop(rig.loop, 20);
  // ~6 ticks pass per answer: they are skipped, never queued
  CHECK(s->skippedTicks() >= 4);
  CHECK_EQ(s->errorCount(), (uint64_t)0);
  CHECK(srv.requests <= (int)s->okCount() + 1);
  for (auto& g : rig.sources()) CHECK_EQ(g, std::string("t_g_a|5"));
}

void testEngineTimeout() {
  Rig rig;
  Server srv(rig.loop, "", /*delayMs=*/-1);
  auto s = std::make_shared<Sensor>(
      specFor(httpSensor(srv, "interval: '200ms', timeout: '50ms', "
                              "record: [{metric: 't_g_a'}]")),
      nullptr);
  s->start(rig.loop, rig.bus, &rig.pool);
  TimePoint t0 = Clock::now();
  runLoop(rig.loop, 3000, [&] { return s->errorCount() >= 1; });
  // first tick inside (100, 200] ms, plus the 50 ms deadline
  CHECK(Clock::now() - t0 < milliseconds(600));
  CHECK(!s->inFlight());
  s->stop();
  CHECK_EQ(s->errorCount(), (uint64_t)1);
  CHECK(rig.rec.events.empty());
}

void testEngineCancelInFlight() {
  int before = countOpenFds();
  {
    Rig rig;
    Server srv(rig.loop, "", /*delayMs=*/-1);
    auto s = std::make_shared<Sensor>(
        specFor(httpSensor(srv, "interval: '20ms', timeout: '30s', "
                                "record: [{metric: 't_g_a'}]")),
        nullptr);
    s->start(rig.loop, rig.bus, &rig.pool);
    runLoop(rig.loop, 2000, [&] { return srv.requests >= 1; });
    CHECK(s->inFlight());
    TimePoint t0 = Clock::now();
    s->stop();
    rig.pool.stop();  // joins the worker: the cancel must have released it
    CHECK(Clock::now() - t0 < milliseconds(1000));
    runLoop(rig.loop, 50);  // the late result is delivered and dropped
    CHECK(rig.rec.events.empty());
    CHECK_EQ(s->okCount() + s->errorCount(), (uint64_t)0);
  }
  CHECK_EQ(countOpenFds(), before);
}

void testEngineBusDropped() {
  Loop loop;
  WorkerPool pool(1);
  auto bus = std::make_shared<Bus>(loop);
  Server srv(loop, httpReply(200, "5"), /*delayMs=*/60);
  auto s = std::make_shared<Sensor>(
      specFor(httpSensor(srv, "interval: '20ms', timeout: '1s', "
                              "record: [{metric: 't_g_a'}]")),
      nullptr);
  s->start(loop, bus, &pool);
  runLoop(loop, 2000, [&] { return srv.requests >= 1; });
  CHECK(s->inFlight());
  bus.reset();  // the generation's bus goes away with a fetch in flight
  runLoop(loop, 2000, [&] { return !s->inFlight(); });
  CHECK(!s->inFlight());
  CHECK_EQ(s->okCount() + s->errorCount(), (uint64_t)0);
  s->stop();
  pool.stop();
}

void testSensorsSet() {
  // the set owns its pool; stop joins it and is idempotent
  Rig rig;
  std::string path = tmpDir + "/set";
  writeFile(path, "3\n");
  std::map<std::string, prom::MetricType> metrics = {
      {"t_g_a", prom::MetricType::Gauge}};
  std::vector<std::shared_ptr<SensorSpec>> specs;
  std::string err, list = "[";
  for (int i = 0; i < 6; i++)
    list += "{name: 's" + std::to_string(i) + "', file: '" + path +
            "', interval: '10ms', record: [{metric: 't_g_a'}]},";
  CHECK(newSensorSpecs(parseJson5(list + "]"), metrics, &specs, &err));
  Sensors set(specs);
  set.start(rig.loop, rig.bus);
  runLoop(rig.loop, 2000, [&] { return rig.rec.events.size() >= 12; });
  set.stop();
  set.stop();
  size_t n = rig.rec.events.size();
  CHECK(n >= 12);
  runLoop(rig.loop, 50);
  CHECK_EQ(rig.rec.events.size(), n);
  std::string text = prom::Registry::global().expose();
  CHECK(text.find("containerpilot_sensor_samples{sensor=\"s0\",result=\"ok\"}") !=
        std::string::npos);
  CHECK(text.find(
            "containerpilot_sensor_samples{sensor=\"s5\",result=\"error\"} 0") !=
        std::string::npos);
}

}  // namespace

int main() {
  logging::setLevel(logging::Level::Fatal);  // failures here are scripted
  char tmpl[] = "/tmp/cpilot-sensortests-XXXXXX";
  if (!mkdtemp(tmpl)) {
    perror("mkdtemp");
    return 1;
  }
  tmpDir = tmpl;

  testExtraction();
  testCounter();
  testFileSource();
  testEnginePeriodicFile();
  testEnginePartialFailure();
  testEngineHttp();
  testEngineHttpStatus();
  testEngineHttpTooLarge();
  testEngineSkipWhileInFlight();
  testEngineTimeout();
  testEngineCancelInFlight();
  testEngineBusDropped();
  testSensorsSet();

  std::string cleanup = "rm -rf '" + tmpDir + "'";
  if (system(cleanup.c_str()) != 0) perror("cleanup");

  if (failures) {
    fprintf(stderr, "%d sensor test failure(s)\n", failures);
    return 1;
  }
  printf("all sensor tests passed\n");
  return 0;
}
