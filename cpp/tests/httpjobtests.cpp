// Tests for http jobs (`jobs[].http`: the action mode of the probe engine
// in cpilot/probe.hpp, wired into Job in cpilot/jobs.hpp): the spec parser
// and the config rules, the request bytes, and a Job with an http action
// driven on a real Loop and Bus against a scripted listener on 127.0.0.1
// served from the same loop.
// Run via `bin/cpilot_httpjobtests`; exits non-zero if any check failed.
#include <arpa/inet.h>
#include <dirent.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <signal.h>
#include <sys/epoll.h>
#include <sys/signalfd.h>
#include <sys/socket.h>
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "cpilot/events.hpp"
#include "cpilot/jobs.hpp"
#include "cpilot/json.hpp"
#include "cpilot/log.hpp"
#include "cpilot/loop.hpp"
#include "cpilot/probe.hpp"
#include "cpilot/version.hpp"

using namespace cpilot;
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

// ---------------- spec parser ----------------

void testSpecParser() {
  health::ProbeSpec spec;
  std::string key, err;
  CHECK(health::parseHttpAction(parseJson5("'http://[::1]:8001/tick'"), &spec,
                                &key, &err));
  CHECK(spec.action);
  CHECK_EQ(spec.method, std::string("GET"));
  CHECK_EQ(spec.hostHeader, std::string("[::1]:8001"));
  CHECK_EQ(spec.path, std::string("/tick"));
  CHECK_EQ(spec.url, std::string("http://[::1]:8001/tick"));
  CHECK(!spec.hasBody);

  health::ProbeSpec full;
  CHECK(health::parseHttpAction(
      parseJson5("{url: 'http://127.0.0.1:8000/drain?x=1', method: 'POST', "
                 "headers: {'Content-Type': 'application/json', 'X-A': 'b'}, "
                 "body: '{\"grace\": 10}', expect: [200, 202]}"),
      &full, &key, &err));
  CHECK_EQ(full.method, std::string("POST"));
  CHECK_EQ(full.path, std::string("/drain?x=1"));
  CHECK(full.hasBody);
  CHECK_EQ(full.body, std::string("{\"grace\": 10}"));
  CHECK_EQ(full.expect.size(), (size_t)2);
  CHECK_EQ(full.headers.size(), (size_t)2);
  CHECK_EQ(full.url, std::string("http://127.0.0.1:8000/drain?x=1"));

  for (const char* m : {"GET", "HEAD", "POST", "PUT", "PATCH", "DELETE"}) {
    health::ProbeSpec s;
    CHECK(health::parseHttpAction(
        parseJson5(std::string("{url: 'http://127.0.0.1/', method: '") + m +
                   "'}"),
        &s, &key, &err));
    CHECK_EQ(s.method, std::string(m));
  }
  // an empty body is still a body; null is none
  health::ProbeSpec empty;
  CHECK(health::parseHttpAction(
      parseJson5("{url: 'http://127.0.0.1/', method: 'DELETE', body: ''}"),
      &empty, &key, &err));
  CHECK(empty.hasBody && empty.body.empty());
  health::ProbeSpec none;
  CHECK(health::parseHttpAction(
      parseJson5("{url: 'http://127.0.0.1/', body: null}"), &none, &key, &err));
  CHECK(!none.hasBody);
  // the limit itself passes
  health::ProbeSpec big;
  CHECK(health::parseHttpAction(
      parseJson5("{url: 'http://127.0.0.1/', method: 'PUT', body: '" +
                 std::string(health::kActionMaxBody, 'x') + "'}"),
      &big, &key, &err));
  CHECK_EQ(big.body.size(), health::kActionMaxBody);

  // health.http keeps its own, narrower rules
  health::ProbeSpec probe;
  CHECK(!health::parseHttpProbe(
      parseJson5("{url: 'http://127.0.0.1/', method: 'POST'}"), &probe, &key,
      &err));
  CHECK_EQ(key, std::string(".method"));
  CHECK_EQ(err, std::string("must be 'GET' or 'HEAD'"));
  CHECK(!health::parseHttpProbe(
      parseJson5("{url: 'http://127.0.0.1/', body: 'x'}"), &probe, &key, &err));
  CHECK_EQ(err, std::string("invalid keys: body"));
  CHECK(health::parseHttpProbe(
      parseJson5("{url: 'http://127.0.0.1/', headers: {Host: 'x'}}"), &probe,
      &key, &err));
  CHECK(!probe.action);
}

// ---------------- config rules ----------------

bool jobsOk(const std::string& jobs, std::string* err,
            std::vector<std::shared_ptr<JobConfig>>* out = nullptr) {
  std::vector<std::shared_ptr<JobConfig>> cfgs;
  bool ok = newJobConfigs(parseJson5("[" + jobs + "]"), nullptr, &cfgs, err);
  if (out) *out = cfgs;
  return ok;
}

void expectRefused(const std::string& jobs, const std::string& want,
                   int line) {
  std::string err;
  if (jobsOk(jobs, &err) || err != want) {
    fprintf(stderr, "FAIL %s:%d: %s -> '%s', want '%s'\n", __FILE__, line,
            jobs.c_str(), err.c_str(), want.c_str());
    failures++;
  }
}
#define REFUSED(jobs, want) expectRefused(jobs, want, __LINE__)

const std::string U = "url: 'http://127.0.0.1:9/x'";

void testConfigRules() {
  std::string err;
  std::vector<std::shared_ptr<JobConfig>> cfgs;

  // accepted shapes, and the deadline each one gets
  CHECK(jobsOk("{name: 'r', http: 'http://localhost:9090/-/reload', "
               "when: {source: 'watch.t', each: 'changed'}}",
               &err, &cfgs));
  if (cfgs.size() == 1) {
    CHECK(cfgs[0]->http != nullptr);
    CHECK(cfgs[0]->exec == nullptr && cfgs[0]->signal == nullptr);
    CHECK_EQ(cfgs[0]->http->name(), std::string("r"));
    CHECK(cfgs[0]->http->spec().action);
    CHECK(cfgs[0]->http->spec().timeout == Duration(std::chrono::seconds(10)));
    CHECK_EQ(cfgs[0]->restartLimit, 0);
  }
  CHECK(jobsOk("{name: 'r', http: {" + U + "}, timeout: '15s'}", &err, &cfgs));
  CHECK(cfgs.size() == 1 &&
        cfgs[0]->http->spec().timeout == Duration(std::chrono::seconds(15)));
  CHECK(jobsOk("{name: 'r', http: {" + U + "}, when: {interval: '30s'}}", &err,
               &cfgs));
  CHECK(cfgs.size() == 1 &&
        cfgs[0]->http->spec().timeout == Duration(std::chrono::seconds(30)) &&
        cfgs[0]->restartLimit == kUnlimited);
  CHECK(jobsOk("{name: 'r', http: {" + U + "}, when: {interval: '30s'}, "
               "timeout: '2s', restarts: 3}", &err, &cfgs));
  CHECK(cfgs.size() == 1 &&
        cfgs[0]->http->spec().timeout == Duration(std::chrono::seconds(2)) &&
        cfgs[0]->restartLimit == 3);
  CHECK(jobsOk("{name: 'r', http: {" + U + "}, restarts: 'never'}", &err));
  CHECK(jobsOk("{name: 'r', http: {" + U + "}, restarts: 0}", &err));
  CHECK(jobsOk("{name: 'app', exec: 'sleep 1'}, {name: 'pre-stop', "
               "stopTimeout: '3s', http: {" + U + ", method: 'POST'}, "
               "when: {source: 'app', once: 'stopping'}}", &err, &cfgs));
  if (cfgs.size() == 2) {
    CHECK(cfgs[1]->whenEvent == (Event{EventCode::Stopping, "app"}));
    CHECK(cfgs[0]->stoppingWaitEvent ==
          (Event{EventCode::Stopped, "pre-stop"}));
  }
  // a job without `http` is parsed as before
  CHECK(jobsOk("{name: 'app', exec: 'sleep 1', http: null}", &err, &cfgs));
  CHECK(cfgs.size() == 1 && cfgs[0]->http == nullptr && cfgs[0]->exec);

  // restarts: only with when.interval
  REFUSED("{name: 'r', http: {" + U + "}, restarts: 3}",
          "job[r].http cannot be combined with restarts '3' unless "
          "'when.interval' is set");
  REFUSED("{name: 'r', http: {" + U + "}, restarts: 'unlimited', "
          "when: {source: 'a', once: 'healthy'}}",
          "job[r].http cannot be combined with restarts 'unlimited' unless "
          "'when.interval' is set");

  // exclusions
  REFUSED("{name: 'r', exec: 'true', http: {" + U + "}}",
          "job[r].http cannot be combined with 'exec'");
  REFUSED("{name: 'app', exec: 'sleep 1'}, {name: 'r', http: {" + U + "}, "
          "signal: {job: 'app', send: 'HUP'}}",
          "job[r].http cannot be combined with 'signal'");
  for (std::string extra :
       {"port: 80", "health: {exec: 'true', interval: 1, ttl: 2}",
        "logging: {raw: true}"}) {
    std::string key = extra.substr(0, extra.find(':'));
    REFUSED("{name: 'r', http: {" + U + "}, " + extra + "}",
            "job[r].http cannot be combined with '" + key +
                "': an http job starts no process");
  }
  REFUSED("{name: 'r', http: {" + U + "}, timeout: '0s'}",
          "job[r].timeout '0s' cannot be less than 1ms");

  // the spec's own errors name their key
  REFUSED("{name: 'r', http: 7}",
          "job[r].http: must be a URL string or an object");
  REFUSED("{name: 'r', http: {" + U + ", retries: 2}}",
          "job[r].http: invalid keys: retries");
  REFUSED("{name: 'r', http: {method: 'POST'}}",
          "job[r].http.url: is required and must be a string");
  REFUSED("{name: 'r', http: 'https://127.0.0.1/'}",
          "job[r].http: https is not supported: TLS checks are not run on "
          "the reactor (use a health.exec check instead)");
  REFUSED("{name: 'r', http: {url: 'ftp://127.0.0.1/'}}",
          "job[r].http.url: malformed URL 'ftp://127.0.0.1/': expected "
          "http://HOST[:PORT][/path]");
  REFUSED("{name: 'r', http: {url: 'http://prometheus:9090/-/reload'}}",
          "job[r].http.url: host 'prometheus' is not an IP literal: names "
          "are not resolved on the reactor (use an IP address or "
          "'localhost', or a health.exec check where DNS is needed)");
  REFUSED("{name: 'r', http: {url: 'http://127.0.0.1:0/'}}",
          "job[r].http.url: port '0' must be a number between 1 and 65535");
  REFUSED("{name: 'r', http: {url: 'http://127.0.0.1:65536/'}}",
          "job[r].http.url: port '65536' must be a number between 1 and "
          "65535");
  REFUSED("{name: 'r', http: {url: 'http://127.0.0.1/a b'}}",
          "job[r].http.url: malformed URL 'http://127.0.0.1/a b': "
          "whitespace, control characters and fragments are not allowed");
  REFUSED("{name: 'r', http: {" + U + ", method: 'TRACE'}}",
          "job[r].http.method: must be one of 'GET', 'HEAD', 'POST', 'PUT', "
          "'PATCH' or 'DELETE'");
  REFUSED("{name: 'r', http: {" + U + ", method: 'post'}}",
          "job[r].http.method: must be one of 'GET', 'HEAD', 'POST', 'PUT', "
          "'PATCH' or 'DELETE'");
  REFUSED("{name: 'r', http: {" + U + ", expect: 99}}",
          "job[r].http.expect: entries must be between 100 and 599, got 99");
  REFUSED("{name: 'r', http: {" + U + ", expect: [200, 600]}}",
          "job[r].http.expect: entries must be between 100 and 599, got 600");
  REFUSED("{name: 'r', http: {" + U + ", expect: []}}",
          "job[r].http.expect: must not be an empty list");
  REFUSED("{name: 'r', http: {" + U + ", expect: '200'}}",
          "job[r].http.expect: must be an int or a list of ints");
  REFUSED("{name: 'r', http: {" + U + ", headers: ['a']}}",
          "job[r].http.headers: must be an object of strings");
  REFUSED("{name: 'r', http: {" + U + ", headers: {A: 1}}}",
          "job[r].http.headers: must be an object of strings");
  REFUSED("{name: 'r', http: {" + U + ", headers: {A: 'x\\r\\nB: y'}}}",
          "job[r].http.headers: names and values must not contain CR or LF");
  REFUSED("{name: 'r', http: {" + U + ", headers: {'A B': 'x'}}}",
          "job[r].http.headers: names must be non-empty and free of ':' and "
          "whitespace");
  for (const char* own : {"Host", "host", "CONNECTION", "Content-Length",
                          "content-length", "Transfer-Encoding"}) {
    REFUSED("{name: 'r', http: {" + U + ", method: 'POST', headers: {'" +
                std::string(own) + "': 'x'}}}",
            "job[r].http.headers: '" + std::string(own) +
                "' is set by the daemon and cannot be configured");
  }
  REFUSED("{name: 'r', http: {" + U + ", method: 'POST', body: 5}}",
          "job[r].http.body: must be a string");
  REFUSED("{name: 'r', http: {" + U + ", body: 'x'}}",
          "job[r].http.body: cannot be sent with method 'GET': use POST, "
          "PUT, PATCH or DELETE");
  REFUSED("{name: 'r', http: {" + U + ", method: 'HEAD', body: 'x'}}",
          "job[r].http.body: cannot be sent with method 'HEAD': use POST, "
          "PUT, PATCH or DELETE");
  REFUSED("{name: 'r', http: {" + U + ", method: 'POST', body: '" +
              std::string(health::kActionMaxBody + 1, 'x') + "'}}",
          "job[r].http.body: must be at most 65536 bytes, got 65537");
}

// ---------------- request bytes ----------------

std::string requestOf(const std::string& http) {
  std::vector<std::shared_ptr<JobConfig>> cfgs;
  std::string err;
  if (!jobsOk("{name: 'r', http: " + http + "}", &err, &cfgs)) {
    fprintf(stderr, "bad http job %s: %s\n", http.c_str(), err.c_str());
    failures++;
    return "";
  }
  return health::buildProbeRequest(cfgs[0]->http->spec());
}

void testRequestBytes() {
  const std::string common = std::string("User-Agent: containerpilot/") +
                             kVersion +
                             "\r\nAccept: */*\r\nConnection: close\r\n";
  CHECK_EQ(requestOf("'http://[::1]:8001/tick'"),
           "GET /tick HTTP/1.1\r\nHost: [::1]:8001\r\n" + common + "\r\n");
  CHECK_EQ(requestOf("{url: 'http://localhost/x', method: 'DELETE'}"),
           "DELETE /x HTTP/1.1\r\nHost: localhost\r\n" + common + "\r\n");
  CHECK_EQ(requestOf("{url: 'http://localhost:9090/-/reload', "
                     "method: 'POST'}"),
           "POST /-/reload HTTP/1.1\r\nHost: localhost:9090\r\n" + common +
               "Content-Length: 0\r\n\r\n");
  // header order: as configured, after the daemon's own
  CHECK_EQ(requestOf("{url: 'http://127.0.0.1:8000/drain?now=1', "
                     "method: 'POST', headers: {'Content-Type': "
                     "'application/json', 'X-Zed': '1', 'Authorization': "
                     "'Bearer t'}, body: '{\"grace\": 10}'}"),
           "POST /drain?now=1 HTTP/1.1\r\nHost: 127.0.0.1:8000\r\n" + common +
               "Content-Length: 13\r\nContent-Type: application/json\r\n"
               "X-Zed: 1\r\nAuthorization: Bearer t\r\n\r\n{\"grace\": 10}");
  CHECK_EQ(requestOf("{url: 'http://127.0.0.1/', method: 'DELETE', "
                     "body: 'gone'}"),
           "DELETE / HTTP/1.1\r\nHost: 127.0.0.1\r\n" + common +
               "Content-Length: 4\r\n\r\ngone");
  // a probe spec builds what it always built
  health::ProbeSpec probe;
  std::string key, err;
  CHECK(health::parseHttpProbe(
      parseJson5("{url: 'http://127.0.0.1:80/h', method: 'HEAD', "
                 "headers: {A: 'b'}}"),
      &probe, &key, &err));
  CHECK_EQ(health::buildProbeRequest(probe),
           "HEAD /h HTTP/1.1\r\nHost: 127.0.0.1:80\r\n" + common +
               "A: b\r\n\r\n");
}

// ---------------- a scripted listener ----------------

int countOpenFds() {
  int n = 0;
  DIR* d = opendir("/proc/self/fd");
  if (!d) return -1;
  while (struct dirent* e = readdir(d))
    if (e->d_name[0] != '.') n++;
  closedir(d);
  return n - 1;  // the directory's own fd
}

// Plays one response per connection once the request's head has arrived:
// `first` after `delayMs`, then `rest` in chunks on a 1 ms timer, then
// what `end` says. What the client did to the connection is recorded.
struct Peer {
  enum class End { KeepOpen, ShutWr, Close };

  Loop& loop;
  std::string first, rest;
  End end = End::KeepOpen;
  int delayMs = 0;
  int restDelayMs = 0;
  size_t chunk = 65536;
  bool closeOnRequest = false;
  bool silent = false;

  int lfd = -1;
  int port = 0;
  int acceptedCount = 0;
  std::string received;
  bool writeFailed = false;  // a send() hit a reset or a closed pipe
  bool wroteAll = false;
  bool sawFin = false;    // the client closed orderly
  bool sawReset = false;  // the client closed abortively
  bool resetBeforeWroteAll = false;

  struct Conn {
    std::string out;
    bool started = false;
    TimePoint restAt;
  };
  std::map<int, Conn> conns;
  uint64_t drip = 0;
  std::vector<uint64_t> timers;

  explicit Peer(Loop& l) : loop(l) {
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
    drip = loop.addInterval(milliseconds(1), [this] { onDrip(); });
  }

  ~Peer() {
    loop.cancelTimer(drip);
    for (uint64_t t : timers) loop.cancelTimer(t);
    while (!conns.empty()) closeConn(conns.begin()->first);
    loop.unwatchFd(lfd);
    close(lfd);
  }

  std::string url(const std::string& path = "/hook") const {
    return "http://127.0.0.1:" + std::to_string(port) + path;
  }

  void closeConn(int fd) {
    loop.unwatchFd(fd);
    close(fd);
    conns.erase(fd);
  }

  void onAccept() {
    while (true) {
      int fd = accept4(lfd, nullptr, nullptr, SOCK_NONBLOCK | SOCK_CLOEXEC);
      if (fd < 0) return;
      acceptedCount++;
      int one = 1;
      setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
      conns[fd];
      loop.watchFd(fd, EPOLLIN, [this, fd](uint32_t) { onData(fd); });
    }
  }

  void onData(int fd) {
    auto it = conns.find(fd);
    if (it == conns.end()) return;
    char buf[4096];
    while (true) {
      ssize_t n = recv(fd, buf, sizeof(buf), 0);
      if (n > 0) {
        received.append(buf, (size_t)n);
        continue;
      }
      if (n < 0 && (errno == EAGAIN || errno == EINTR)) break;
      if (n == 0) sawFin = true;
      else sawReset = true;
      if (!wroteAll && !silent && !closeOnRequest) resetBeforeWroteAll = true;
      closeConn(fd);
      return;
    }
    if (it->second.started ||
        received.find("\r\n\r\n") == std::string::npos)
      return;
    it->second.started = true;
    if (closeOnRequest) {
      closeConn(fd);
      return;
    }
    if (silent) return;
    timers.push_back(loop.addTimeout(milliseconds(delayMs), [this, fd] {
      auto c = conns.find(fd);
      if (c == conns.end()) return;
      c->second.out = first + rest;
      c->second.restAt = Clock::now() + milliseconds(restDelayMs);
      writeSome(fd, c->second, first.size());
    }));
  }

  void writeSome(int fd, Conn& c, size_t want) {
    if (want > c.out.size()) want = c.out.size();
    if (want) {
      ssize_t n = send(fd, c.out.data(), want, MSG_NOSIGNAL);
      if (n > 0) {
        c.out.erase(0, (size_t)n);
      } else if (errno != EAGAIN && errno != EINTR) {
        writeFailed = true;
        c.out.clear();
        return;
      }
    }
    if (!c.out.empty()) return;
    wroteAll = true;
    if (end == End::ShutWr) shutdown(fd, SHUT_WR);
    else if (end == End::Close) closeConn(fd);
  }

  void onDrip() {
    TimePoint now = Clock::now();
    std::vector<int> due;
    for (auto& kv : conns)
      if (!kv.second.out.empty() && now >= kv.second.restAt)
        due.push_back(kv.first);
    for (int fd : due) writeSome(fd, conns[fd], chunk);
  }
};

std::string reply(int code, const std::string& body, bool withLength = true) {
  return "HTTP/1.1 " + std::to_string(code) + " Whatever\r\n" +
         (withLength ? "Content-Length: " + std::to_string(body.size()) +
                           "\r\n"
                     : "") +
         "X-Served-By: peer\r\n\r\n" + body;
}

// ---------------- a Job on a real Loop and Bus ----------------

struct Recorder : Subscriber {
  std::vector<Event> events;
  void onEvent(const Event& e) override { events.push_back(e); }
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
  // exit and error events of job `web`, in order, as "Code source"
  std::vector<std::string> outcome() const {
    std::vector<std::string> out;
    for (auto& e : events) {
      if (e.code == EventCode::ExitSuccess && e.source == "web")
        out.push_back("ExitSuccess web");
      else if (e.code == EventCode::ExitFailed && e.source == "web")
        out.push_back("ExitFailed web");
      else if (e.code == EventCode::Error)
        out.push_back("Error " + e.source);
    }
    return out;
  }
};

struct Rig {
  Loop loop;
  std::shared_ptr<Bus> bus = std::make_shared<Bus>(loop);
  Recorder rec;
  Peer peer{loop};
  std::vector<std::shared_ptr<JobConfig>> cfgs;
  std::vector<std::shared_ptr<Job>> jobs;
  int sigfd = -1;

  Rig() {
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
    bus->subscribe(&rec);
  }

  // the listener's port is known only now, so jobs come after construction
  void start(const std::string& jobsJson) {
    std::string err;
    if (!newJobConfigs(parseJson5(jobsJson), nullptr, &cfgs, &err)) {
      fprintf(stderr, "job config error: %s\n", err.c_str());
      exit(1);
    }
    for (auto& cfg : cfgs) {
      jobs.push_back(std::make_shared<Job>(cfg));
      bus->subscribe(jobs.back().get());
    }
    for (auto& job : jobs) job->run(loop, bus, [] {});
    bus->publish(GlobalStartup);
  }

  // job `web`: one request per `watch.t` change
  void startWeb(const std::string& http, const std::string& timeout = "2s") {
    start("[{name: 'web', http: " + http + ", timeout: '" + timeout +
          "', when: {source: 'watch.t', each: 'changed'}}]");
  }

  ~Rig() {
    bus->shutdown();
    spin(5000, [this] { return allDone(); });
    for (auto& cfg : cfgs)
      if (cfg->exec && cfg->exec->running()) cfg->exec->kill();
    spin(2000, [this] { return allDone(); });
    CHECK(allDone());
    bus->unsubscribe(&rec);
    loop.unwatchFd(sigfd);
    close(sigfd);
  }

  bool allDone() const {
    for (auto& job : jobs)
      if (!job->isComplete()) return false;
    for (auto& cfg : cfgs)
      if (cfg->exec && cfg->exec->running()) return false;
    return true;
  }

  bool spin(int ms, std::function<bool()> done = nullptr) {
    uint64_t deadline = loop.addTimeout(milliseconds(ms), [&] { loop.stop(); });
    uint64_t poll = 0;
    if (done)
      poll = loop.addInterval(milliseconds(1), [&] {
        if (done()) loop.stop();
      });
    loop.run();
    loop.cancelTimer(deadline);
    if (poll) loop.cancelTimer(poll);
    return done ? done() : true;
  }

  void trigger() { bus->publish(Event{EventCode::StatusChanged, "watch.t"}); }

  bool exited() const {
    return rec.count(EventCode::ExitSuccess, "web") +
               rec.count(EventCode::ExitFailed, "web") > 0;
  }

  // one request: until the job's exit event, then a little longer to
  // catch what must not follow
  void once(int ms = 3000) {
    trigger();
    CHECK(spin(ms, [this] { return exited(); }));
    spin(30);
  }
};

using Outcome = std::vector<std::string>;

void test200WithLength() {
  // the body comes 30 ms after the head: a client that reset at the status
  // line, as a probe does, would make that second write fail
  Rig rig;
  rig.peer.first = reply(200, "reloaded\n").substr(0, 40);
  rig.peer.rest = reply(200, "reloaded\n").substr(40);
  rig.peer.restDelayMs = 30;
  rig.startWeb("{url: '" + rig.peer.url("/-/reload?x=1") +
               "', method: 'POST', headers: {'X-A': 'b'}, body: 'now'}");
  TimePoint t0 = Clock::now();
  rig.once();
  CHECK(Clock::now() - t0 >= milliseconds(30));
  CHECK(rig.rec.outcome() == Outcome{"ExitSuccess web"});
  CHECK_EQ(rig.peer.received,
           health::buildProbeRequest(rig.cfgs[0]->http->spec()));
  CHECK(rig.peer.received.find("POST /-/reload?x=1 HTTP/1.1\r\n") == 0);
  // the response was fully written, and only then did the client leave
  CHECK(rig.peer.wroteAll && !rig.peer.writeFailed);
  CHECK(!rig.peer.resetBeforeWroteAll);
  CHECK(rig.peer.sawFin || rig.peer.sawReset);
  CHECK(!rig.cfgs[0]->http->running());
  // `each`: still there for the next change
  CHECK(!rig.jobs[0]->isComplete());
  rig.trigger();
  CHECK(rig.spin(3000, [&] {
    return rig.rec.count(EventCode::ExitSuccess, "web") == 2;
  }));
  CHECK_EQ(rig.peer.acceptedCount, 2);
}

void test200ThenClose() {
  // no length: the response ends at the peer's FIN, which the client
  // answers with an orderly close of its own
  Rig rig;
  rig.peer.first = reply(200, "", false);
  rig.peer.rest = std::string(5000, 'r');
  rig.peer.restDelayMs = 30;
  rig.peer.end = Peer::End::ShutWr;
  rig.startWeb("'" + rig.peer.url() + "'");
  rig.once();
  CHECK(rig.rec.outcome() == Outcome{"ExitSuccess web"});
  CHECK(rig.peer.wroteAll && !rig.peer.writeFailed);
  CHECK(!rig.peer.resetBeforeWroteAll);
  CHECK(rig.peer.sawFin && !rig.peer.sawReset);
}

void test503() {
  Rig rig;
  rig.peer.first = reply(503, "down\n").substr(0, 30);
  rig.peer.rest = reply(503, "down\n").substr(30);
  rig.peer.restDelayMs = 20;
  rig.startWeb("'" + rig.peer.url() + "'");
  rig.once();
  CHECK(rig.rec.outcome() ==
        (Outcome{"ExitFailed web", "Error web: unexpected status 503"}));
  // an unacceptable response is read out as well
  CHECK(rig.peer.wroteAll && !rig.peer.writeFailed);
  CHECK(!rig.peer.resetBeforeWroteAll);
}

void testExpect() {
  {
    Rig rig;
    rig.peer.first = reply(202, "");
    rig.startWeb("{url: '" + rig.peer.url() + "', expect: [200, 202]}");
    rig.once();
    CHECK(rig.rec.outcome() == Outcome{"ExitSuccess web"});
  }
  Rig other;
  other.peer.first = reply(200, "");
  other.startWeb("{url: '" + other.peer.url() + "', expect: 204}");
  other.once();
  CHECK(other.rec.outcome() ==
        (Outcome{"ExitFailed web", "Error web: unexpected status 200"}));
}

void testGarbage() {
  Rig rig;
  rig.peer.first = "SSH-2.0-OpenSSH_9.6\r\n";
  rig.startWeb("'" + rig.peer.url() + "'");
  rig.once();
  CHECK(rig.rec.outcome() ==
        (Outcome{"ExitFailed web", "Error web: malformed response"}));
}

void testClosedBeforeStatusLine() {
  Rig rig;
  rig.peer.closeOnRequest = true;
  rig.startWeb("'" + rig.peer.url() + "'");
  rig.once();
  CHECK(rig.rec.outcome() ==
        (Outcome{"ExitFailed web",
                 "Error web: connection closed before response"}));
}

void testRefused() {
  Rig rig;
  int port = rig.peer.port;
  // a port nobody listens on: the one of a listener just closed
  {
    Loop other;
    Peer gone(other);
    port = gone.port;
  }
  rig.startWeb("'http://127.0.0.1:" + std::to_string(port) + "/'");
  rig.once();
  CHECK(rig.rec.outcome() ==
        (Outcome{"ExitFailed web",
                 std::string("Error web: ") + strerror(ECONNREFUSED)}));
}

void testBytewiseStatusLine() {
  Rig rig;
  rig.peer.first = "";
  rig.peer.rest = reply(200, "ok\n");
  rig.peer.chunk = 1;
  rig.startWeb("'" + rig.peer.url() + "'");
  rig.once();
  CHECK(rig.rec.outcome() == Outcome{"ExitSuccess web"});
  CHECK(rig.peer.wroteAll && !rig.peer.writeFailed);
  CHECK(!rig.peer.resetBeforeWroteAll);
}

void testMoreThanTheCap() {
  // 200 and then 3 MiB without a length or an end: the job is done once
  // the cap has gone by, long before its deadline
  Rig rig;
  rig.peer.first = reply(200, "", false);
  rig.peer.rest = std::string(3 * health::kActionMaxDrain, 'z');
  rig.startWeb("'" + rig.peer.url() + "'", "5s");
  TimePoint t0 = Clock::now();
  rig.once(4000);
  CHECK(Clock::now() - t0 < milliseconds(2500));
  CHECK(rig.rec.outcome() == Outcome{"ExitSuccess web"});
  CHECK(!rig.peer.wroteAll);
  CHECK(!rig.cfgs[0]->http->running());
}

void testLengthBeyondTheCap() {
  // an announced length the cap ends
  Rig rig;
  rig.peer.first = "HTTP/1.1 200 OK\r\nContent-Length: 99999999\r\n\r\n";
  rig.peer.rest = std::string(2 * health::kActionMaxDrain, 'z');
  rig.startWeb("'" + rig.peer.url() + "'", "5s");
  rig.once(4000);
  CHECK(rig.rec.outcome() == Outcome{"ExitSuccess web"});
  CHECK(!rig.peer.wroteAll);
}

void testNeverAnswers() {
  Rig rig;
  rig.peer.silent = true;
  rig.startWeb("'" + rig.peer.url() + "'", "100ms");
  TimePoint t0 = Clock::now();
  rig.once();
  CHECK(Clock::now() - t0 >= milliseconds(100));
  CHECK(rig.rec.outcome() ==
        (Outcome{"ExitFailed web", "Error web: timeout after 100ms"}));
  CHECK(!rig.cfgs[0]->http->running());
}

void testDeadlineDuringDrain() {
  // a 200 whose body never ends: the deadline ends the drain, not the 200
  Rig rig;
  rig.peer.first = reply(200, "", false) + "partial";
  rig.startWeb("'" + rig.peer.url() + "'", "150ms");
  TimePoint t0 = Clock::now();
  rig.trigger();
  rig.spin(60);
  // decided, but not published before the drain ends
  CHECK(rig.rec.outcome().empty());
  CHECK(rig.cfgs[0]->http->running());
  CHECK(rig.spin(3000, [&] { return rig.exited(); }));
  CHECK(Clock::now() - t0 >= milliseconds(150));
  rig.spin(30);
  CHECK(rig.rec.outcome() == Outcome{"ExitSuccess web"});
}

void testHeadHasNoBody() {
  // a HEAD response announces a length that never comes
  Rig rig;
  rig.peer.first = "HTTP/1.1 200 OK\r\nContent-Length: 500\r\n\r\n";
  rig.startWeb("{url: '" + rig.peer.url() + "', method: 'HEAD'}", "2s");
  TimePoint t0 = Clock::now();
  rig.once();
  CHECK(Clock::now() - t0 < milliseconds(1000));
  CHECK(rig.rec.outcome() == Outcome{"ExitSuccess web"});
}

void testStartWhileInFlight() {
  Rig rig;
  rig.peer.first = reply(200, "ok\n");
  rig.peer.delayMs = 120;
  rig.startWeb("'" + rig.peer.url() + "'");
  rig.trigger();
  rig.spin(30);
  CHECK(rig.cfgs[0]->http->running());
  rig.trigger();
  rig.trigger();
  rig.bus->publish(Event{EventCode::Signal, "SIGHUP"});
  CHECK(rig.spin(3000, [&] { return rig.exited(); }));
  rig.spin(60);
  CHECK(rig.rec.outcome() == Outcome{"ExitSuccess web"});
  CHECK_EQ(rig.peer.acceptedCount, 1);
  // nothing was queued either: the next change is one more request
  rig.trigger();
  CHECK(rig.spin(3000, [&] {
    return rig.rec.count(EventCode::ExitSuccess, "web") == 2;
  }));
  CHECK_EQ(rig.peer.acceptedCount, 2);
}

void testIgnoredTicksUseNoRestart() {
  // interval 40 ms, answer after 100 ms: two ticks fall into every request
  // and must not count against `restarts: 2`, so three requests are made
  Rig rig;
  rig.peer.first = reply(200, "ok\n");
  rig.peer.delayMs = 100;
  rig.start("[{name: 'web', http: '" + rig.peer.url() +
            "', when: {interval: '40ms'}, timeout: '1s', restarts: 2}]");
  CHECK(rig.spin(5000, [&] {
    return rig.rec.count(EventCode::Stopped, "web") == 1;
  }));
  CHECK_EQ(rig.peer.acceptedCount, 3);
}

void testSignalStartWhileInFlight() {
  Rig rig;
  rig.peer.first = reply(200, "ok\n");
  rig.peer.delayMs = 100;
  rig.start("[{name: 'web', http: '" + rig.peer.url() +
            "', when: {source: 'SIGHUP'}}]");
  rig.bus->publish(Event{EventCode::Signal, "SIGHUP"});
  rig.spin(20);
  rig.bus->publish(Event{EventCode::Signal, "SIGHUP"});
  CHECK(rig.spin(3000, [&] { return rig.exited(); }));
  rig.spin(50);
  CHECK_EQ(rig.peer.acceptedCount, 1);
  CHECK_EQ(rig.rec.count(EventCode::ExitSuccess, "web"), 1);
}

void testCleanupWhileInFlight() {
  int fdsBefore = countOpenFds();
  {
    Rig rig;
    rig.peer.silent = true;
    rig.startWeb("'" + rig.peer.url() + "'", "300ms");
    long idle = rig.cfgs[0]->http.use_count();
    int fdsIdle = countOpenFds();
    rig.trigger();
    rig.spin(30);
    CHECK(rig.cfgs[0]->http->running());
    CHECK(rig.cfgs[0]->http.use_count() > idle);
    // the client's socket and the listener's accepted one
    CHECK_EQ(countOpenFds(), fdsIdle + 2);
    rig.bus->publish(Event{EventCode::Quit, "web"});
    CHECK(rig.spin(2000, [&] { return rig.jobs[0]->isComplete(); }));
    CHECK(!rig.cfgs[0]->http->running());
    CHECK_EQ(rig.rec.count(EventCode::Stopped, "web"), 1);
    // past the deadline: the timer was cancelled, so nothing more is said
    // and nothing holds on to the request
    rig.spin(400);
    CHECK(rig.rec.outcome().empty());
    CHECK_EQ((long)rig.cfgs[0]->http.use_count(), idle);
    // the listener saw the abortive close and dropped its side
    CHECK(rig.peer.sawReset);
    CHECK_EQ(countOpenFds(), fdsIdle);
  }
  CHECK_EQ(countOpenFds(), fdsBefore);
}

void testKillWhileInFlight() {
  // the kill sweep: the request is dropped and the job ends without an
  // exit event, so whatever waits for its `stopped` moves on
  Rig rig;
  rig.peer.silent = true;
  rig.startWeb("'" + rig.peer.url() + "'", "5s");
  rig.trigger();
  rig.spin(30);
  rig.jobs[0]->kill();
  CHECK(!rig.cfgs[0]->http->running());
  CHECK(rig.spin(1000, [&] { return rig.jobs[0]->isComplete(); }));
  CHECK(rig.rec.outcome().empty());
  CHECK_EQ(rig.rec.count(EventCode::Stopped, "web"), 1);
}

void testPreStopChain() {
  // shutdown: Stopping{app} starts pre-stop, whose request takes 150 ms;
  // only after its `stopped` is app terminated
  Rig rig;
  rig.peer.first = reply(200, "drained\n");
  rig.peer.delayMs = 150;
  rig.start("[{name: 'app', exec: 'sleep 30', stopTimeout: '5s'}, "
            "{name: 'web', http: {url: '" + rig.peer.url("/drain") +
            "', method: 'POST', body: '{\"grace\": 10}'}, timeout: '3s', "
            "when: {source: 'app', once: 'stopping'}}]");
  CHECK(rig.spin(5000, [&] { return rig.cfgs[0]->exec->pid() > 0; }));
  CHECK_EQ(rig.peer.acceptedCount, 0);
  TimePoint t0 = Clock::now();
  rig.bus->shutdown();
  CHECK(rig.spin(5000, [&] { return rig.allDone(); }));
  CHECK(Clock::now() - t0 >= milliseconds(150));
  CHECK(Clock::now() - t0 < milliseconds(3000));
  CHECK_EQ(rig.peer.acceptedCount, 1);
  CHECK(rig.peer.received.find("POST /drain HTTP/1.1\r\n") == 0);
  int iStopping = rig.rec.indexOf(EventCode::Stopping, "app");
  int iWeb = rig.rec.indexOf(EventCode::ExitSuccess, "web");
  int iWebStopped = rig.rec.indexOf(EventCode::Stopped, "web");
  int iAppExit = rig.rec.indexOf(EventCode::ExitFailed, "app");  // SIGTERM
  int iStopped = rig.rec.indexOf(EventCode::Stopped, "app");
  CHECK(iStopping >= 0 && iStopping < iWeb && iWeb < iWebStopped &&
        iWebStopped < iStopped);
  // the target was not touched before the request was done
  CHECK(iAppExit < 0 || iAppExit > iWebStopped);
  CHECK_EQ(rig.rec.count(EventCode::ExitFailed, "web"), 0);
}

void testSubscription() {
  std::vector<std::shared_ptr<JobConfig>> cfgs;
  std::string err;
  CHECK(jobsOk("{name: 'a', http: 'http://127.0.0.1:9/', "
               "when: {source: 'watch.t', each: 'changed'}}, "
               "{name: 'b', exec: 'true', "
               "when: {source: 'watch.t', each: 'changed'}}",
               &err, &cfgs));
  if (cfgs.size() != 2) return;
  // as narrow as an exec job's
  CHECK_EQ(Job(cfgs[0]).subscription().sources.size(),
           Job(cfgs[1]).subscription().sources.size());
}

}  // namespace

int main() {
  logging::setLevel(logging::Level::Fatal);  // failures here are scripted

  testSpecParser();
  testConfigRules();
  testRequestBytes();
  testSubscription();
  test200WithLength();
  test200ThenClose();
  test503();
  testExpect();
  testGarbage();
  testClosedBeforeStatusLine();
  testRefused();
  testBytewiseStatusLine();
  testMoreThanTheCap();
  testLengthBeyondTheCap();
  testNeverAnswers();
  testDeadlineDuringDrain();
  testHeadHasNoBody();
  testStartWhileInFlight();
  testIgnoredTicksUseNoRestart();
  testSignalStartWhileInFlight();
  testCleanupWhileInFlight();
  testKillWhileInFlight();
  testPreStopChain();

  if (failures) {
    fprintf(stderr, "%d http job test failure(s)\n", failures);
    return 1;
  }
  printf("all http job tests passed\n");
  return 0;
}
