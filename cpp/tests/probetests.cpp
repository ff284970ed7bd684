// Tests for the native health-probe engine (cpilot/probe.hpp). Drives a
// real Loop and Bus with a recording subscriber against listeners opened
// here on 127.0.0.1; everything runs on the one loop thread.
// Run via `bin/cpilot_probetests`; exits non-zero if any check failed.
#include <arpa/inet.h>
#include <dirent.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <sys/epoll.h>
#include <sys/resource.h>
#include <sys/socket.h>
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "cpilot/events.hpp"
#include "cpilot/json.hpp"
#include "cpilot/log.hpp"
#include "cpilot/loop.hpp"
#include "cpilot/probe.hpp"
#include "cpilot/version.hpp"

using namespace cpilot;
using namespace cpilot::health;
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

const std::string kName = "check.web";

struct Recorder : Subscriber {
  std::vector<Event> events;
  std::vector<TimePoint> at;
  void onEvent(const Event& e) override {
    events.push_back(e);
    at.push_back(Clock::now());
  }
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

// run the loop for `ms`, or until `done` returns true (polled every ms)
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

// A scripted peer on 127.0.0.1, served from the same loop as the probe.
struct Server {
  enum class Act { Hold, Reply, ReplyBytewise, CloseOnAccept, CloseOnRequest };

  Loop& loop;
  Act act;
  std::string reply;
  int lfd = -1;
  int port = 0;
  int acceptedCount = 0;
  std::string received;            // every request byte, all connections
  std::map<int, std::string> out;  // bytewise replies in progress
  std::vector<int> open;
  uint64_t drip = 0;

  Server(Loop& l, Act a, std::string r = "")
      : loop(l), act(a), reply(std::move(r)) {
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
    if (act == Act::ReplyBytewise)
      // one byte per millisecond with TCP_NODELAY: each byte leaves as
      // its own segment and the probe gets to read between them
      drip = loop.addInterval(milliseconds(1), [this] {
        for (auto it = out.begin(); it != out.end();) {
          if (it->second.empty()) {
            it = out.erase(it);
            continue;
          }
          if (send(it->first, it->second.data(), 1, MSG_NOSIGNAL) == 1)
            it->second.erase(0, 1);
          else
            it->second.clear();  // probe already closed: done
          ++it;
        }
      });
  }

  ~Server() {
    if (drip) loop.cancelTimer(drip);
    for (int fd : open) closeConn(fd, false);
    loop.unwatchFd(lfd);
    close(lfd);
  }

  std::string hostPort() const { return "127.0.0.1:" + std::to_string(port); }

  void closeConn(int fd, bool forget = true) {
    loop.unwatchFd(fd);
    close(fd);
    out.erase(fd);
    if (forget)
      for (auto it = open.begin(); it != open.end(); ++it)
        if (*it == fd) {
          open.erase(it);
          break;
        }
  }

  void onAccept() {
    while (true) {
      int fd = accept4(lfd, nullptr, nullptr, SOCK_NONBLOCK | SOCK_CLOEXEC);
      if (fd < 0) return;
      acceptedCount++;
      if (act == Act::CloseOnAccept) {
        close(fd);
        continue;
      }
      int one = 1;
      setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
      open.push_back(fd);
      loop.watchFd(fd, EPOLLIN, [this, fd](uint32_t) { onData(fd); });
    }
  }

  void onData(int fd) {
    char buf[4096];
    while (true) {
      ssize_t n = recv(fd, buf, sizeof(buf), 0);
      if (n > 0) {
        received.append(buf, (size_t)n);
        continue;
      }
      if (n < 0 && (errno == EAGAIN || errno == EINTR)) break;
      closeConn(fd);  // peer closed or reset
      return;
    }
    if (received.find("\r\n\r\n") == std::string::npos) return;
    switch (act) {
      case Act::Reply: {
        ssize_t unused = send(fd, reply.data(), reply.size(), MSG_NOSIGNAL);
        (void)unused;
        break;
      }
      case Act::ReplyBytewise:
        if (!out.count(fd)) out[fd] = reply;
        break;
      case Act::CloseOnRequest:
        closeConn(fd);
        break;
      default:
        break;
    }
  }
};

std::string statusReply(int code) {
  return "HTTP/1.1 " + std::to_string(code) +
         " Whatever\r\nContent-Length: 0\r\n\r\n";
}

ProbePtr tcpProbe(const std::string& hostPort, int timeoutMs) {
  ProbeSpec spec;
  std::string err;
  if (!parseTcpProbe(hostPort, &spec, &err)) {
    fprintf(stderr, "bad tcp spec %s: %s\n", hostPort.c_str(), err.c_str());
    exit(1);
  }
  spec.timeout = milliseconds(timeoutMs);
  return std::make_shared<Probe>(std::move(spec), kName);
}

ProbePtr httpProbe(const std::string& json5, int timeoutMs) {
  ProbeSpec spec;
  std::string key, err;
  if (!parseHttpProbe(parseJson5(json5), &spec, &key, &err)) {
    fprintf(stderr, "bad http spec %s: %s %s\n", json5.c_str(), key.c_str(),
            err.c_str());
    exit(1);
  }
  spec.timeout = milliseconds(timeoutMs);
  return std::make_shared<Probe>(std::move(spec), kName);
}

std::string urlFor(const Server& s, const std::string& path = "/health") {
  return "http://127.0.0.1:" + std::to_string(s.port) + path;
}

// One loop + bus + recorder per scenario; run() drives the probe until a
// verdict (or `ms`) and then a little longer to catch stray events.
struct Rig {
  Loop loop;
  std::shared_ptr<Bus> bus = std::make_shared<Bus>(loop);
  Recorder rec;
  Rig() { bus->subscribe(&rec); }
  ~Rig() {
    if (bus) bus->unsubscribe(&rec);
  }
  void go(const ProbePtr& p, int ms = 2000) {
    p->run(loop, bus);
    runLoop(loop, ms, [&] { return !rec.events.empty() && !p->running(); });
    runLoop(loop, 20);
  }
  void expectPass() {
    CHECK_EQ(rec.events.size(), (size_t)1);
    if (rec.events.size() == 1)
      CHECK(rec.events[0] == (Event{EventCode::ExitSuccess, kName}));
  }
  // ExitFailed first, then its Error, nothing else
  void expectFail(const std::string& reason) {
    CHECK_EQ(rec.events.size(), (size_t)2);
    if (rec.events.size() != 2) return;
    CHECK(rec.events[0] == (Event{EventCode::ExitFailed, kName}));
    CHECK(rec.events[1].code == EventCode::Error);
    if (rec.events[1].source != kName + ": " + reason) {
      fprintf(stderr, "  got reason '%s', want '%s: %s'\n",
              rec.events[1].source.c_str(), kName.c_str(), reason.c_str());
      failures++;
    }
  }
};

void testTcpPass() {
  Rig rig;
  Server srv(rig.loop, Server::Act::Hold);
  auto p = tcpProbe(srv.hostPort(), 1000);
  CHECK_EQ(p->name(), kName);
  rig.go(p);
  rig.expectPass();
  CHECK(!p->running());
  CHECK_EQ(srv.acceptedCount, 1);

  // localhost means 127.0.0.1
  Rig rig2;
  Server srv2(rig2.loop, Server::Act::Hold);
  rig2.go(tcpProbe("localhost:" + std::to_string(srv2.port), 1000));
  rig2.expectPass();
}

void testTcpRefused() {
  int port;
  {
    Loop scratch;
    Server gone(scratch, Server::Act::Hold);
    port = gone.port;
  }  // bound, port read, closed: nothing listens there now
  Rig rig;
  rig.go(tcpProbe("127.0.0.1:" + std::to_string(port), 1000));
  rig.expectFail(strerror(ECONNREFUSED));
}

void testHttpStatuses() {
  {
    Rig rig;
    Server srv(rig.loop, Server::Act::Reply, statusReply(200));
    rig.go(httpProbe("\"" + urlFor(srv) + "\"", 1000));
    rig.expectPass();
  }
  {
    Rig rig;
    Server srv(rig.loop, Server::Act::Reply, statusReply(503));
    rig.go(httpProbe("\"" + urlFor(srv) + "\"", 1000));
    rig.expectFail("unexpected status 503");
  }
  {  // expect: [204] against a 200
    Rig rig;
    Server srv(rig.loop, Server::Act::Reply, statusReply(200));
    rig.go(httpProbe("{url: \"" + urlFor(srv) + "\", expect: [204]}", 1000));
    rig.expectFail("unexpected status 200");
  }
  {  // expect as a bare int, outside 2xx
    Rig rig;
    Server srv(rig.loop, Server::Act::Reply, statusReply(404));
    rig.go(httpProbe("{url: \"" + urlFor(srv) + "\", expect: 404}", 1000));
    rig.expectPass();
  }
  {  // a status line with no reason phrase, HTTP/1.0
    Rig rig;
    Server srv(rig.loop, Server::Act::Reply, "HTTP/1.0 204\r\n\r\n");
    rig.go(httpProbe("\"" + urlFor(srv) + "\"", 1000));
    rig.expectPass();
  }
  {  // a CRLF-terminated line that is no status line
    Rig rig;
    Server srv(rig.loop, Server::Act::Reply, "SSH-2.0-OpenSSH_9.6\r\n");
    rig.go(httpProbe("\"" + urlFor(srv) + "\"", 1000));
    rig.expectFail("malformed response");
  }
}

void testRequestOnTheWire() {
  {  // HEAD sends HEAD
    Rig rig;
    Server srv(rig.loop, Server::Act::Reply, statusReply(200));
    rig.go(httpProbe("{url: \"" + urlFor(srv, "/up") + "\", method: \"HEAD\"}",
                     1000));
    rig.expectPass();
    CHECK(srv.received.compare(0, 19, "HEAD /up HTTP/1.1\r\n") == 0);
  }
  {  // the whole request, byte for byte; Host exactly as written
    Rig rig;
    Server srv(rig.loop, Server::Act::Reply, statusReply(200));
    std::string authority = "localhost:" + std::to_string(srv.port);
    rig.go(httpProbe("{url: \"http://" + authority + "/health?deep=1\", "
                     "headers: {\"X-Token\": \"a b\", "
                     "Authorization: \"Bearer z\"}}",
                     1000));
    rig.expectPass();
    std::string want = "GET /health?deep=1 HTTP/1.1\r\nHost: " + authority +
                       "\r\nUser-Agent: containerpilot/" + kVersion +
                       "\r\nAccept: */*\r\nConnection: close\r\n"
                       "X-Token: a b\r\nAuthorization: Bearer z\r\n\r\n";
    CHECK_EQ(srv.received, want);
  }
  {  // default path, query without a path
    ProbeSpec spec;
    std::string key, err;
    CHECK(parseHttpProbe(Json("http://10.1.2.3"), &spec, &key, &err));
    CHECK_EQ(spec.path, std::string("/"));
    CHECK_EQ(spec.target, std::string("10.1.2.3:80"));
    CHECK_EQ(spec.hostHeader, std::string("10.1.2.3"));
    ProbeSpec q;
    CHECK(parseHttpProbe(Json("http://[::1]:8080?x=1"), &q, &key, &err));
    CHECK_EQ(q.path, std::string("/?x=1"));
    CHECK_EQ(q.hostHeader, std::string("[::1]:8080"));
    CHECK_EQ((int)q.addr.ss_family, (int)AF_INET6);
  }
}

void testSplitStatusLine() {
  Rig rig;
  Server srv(rig.loop, Server::Act::ReplyBytewise, statusReply(200));
  rig.go(httpProbe("\"" + urlFor(srv) + "\"", 2000));
  rig.expectPass();

  Rig rig2;
  Server srv2(rig2.loop, Server::Act::ReplyBytewise, statusReply(500));
  rig2.go(httpProbe("\"" + urlFor(srv2) + "\"", 2000));
  rig2.expectFail("unexpected status 500");
}

void testNoCrlfIn8K() {
  Rig rig;
  Server srv(rig.loop, Server::Act::Reply,
             std::string(kProbeMaxStatusLine, 'x'));
  rig.go(httpProbe("\"" + urlFor(srv) + "\"", 1000));
  rig.expectFail("malformed response");

  // one byte short of the cap, then the peer holds: no verdict but the
  // timeout's
  Rig rig2;
  Server srv2(rig2.loop, Server::Act::Reply,
              std::string(kProbeMaxStatusLine - 1, 'x'));
  rig2.go(httpProbe("\"" + urlFor(srv2) + "\"", 100));
  rig2.expectFail("timeout after 100ms");
}

void testPeerCloses() {
  {  // closes after reading the request
    Rig rig;
    Server srv(rig.loop, Server::Act::CloseOnRequest);
    rig.go(httpProbe("\"" + urlFor(srv) + "\"", 1000));
    rig.expectFail("connection closed before response");
  }
  {  // closes straight after accept (the request may meet a reset)
    Rig rig;
    Server srv(rig.loop, Server::Act::CloseOnAccept);
    rig.go(httpProbe("\"" + urlFor(srv) + "\"", 1000));
    rig.expectFail("connection closed before response");
  }
}

void testTimeout() {
  const int kTimeoutMs = 150;
  Rig rig;
  Server srv(rig.loop, Server::Act::Hold);
  auto p = httpProbe("\"" + urlFor(srv) + "\"", kTimeoutMs);
  TimePoint t0 = Clock::now();
  p->run(rig.loop, rig.bus);
  CHECK(p->running());
  // not before the timeout ...
  runLoop(rig.loop, kTimeoutMs - 30);
  CHECK_EQ(rig.rec.events.size(), (size_t)0);
  CHECK(p->running());
  // ... exactly one verdict at it, and nothing more by twice the timeout
  runLoop(rig.loop, kTimeoutMs + 30);
  rig.expectFail("timeout after 150ms");
  CHECK(!p->running());
  if (!rig.rec.at.empty()) {
    CHECK(rig.rec.at[0] - t0 >= milliseconds(kTimeoutMs));
    CHECK(rig.rec.at[0] - t0 < milliseconds(2 * kTimeoutMs));
  }
  CHECK(Clock::now() - t0 >= milliseconds(2 * kTimeoutMs));
  CHECK_EQ(rig.rec.events.size(), (size_t)2);
  CHECK_EQ(probeDurationString(std::chrono::seconds(5)), std::string("5s"));
  CHECK_EQ(probeDurationString(milliseconds(1500)), std::string("1500ms"));
}

void testOverlapSkipsTick() {
  {  // hung peer: the second run is dropped, one verdict at the timeout
    Rig rig;
    Server srv(rig.loop, Server::Act::Hold);
    auto p = httpProbe("\"" + urlFor(srv) + "\"", 100);
    p->run(rig.loop, rig.bus);
    runLoop(rig.loop, 30);
    p->run(rig.loop, rig.bus);
    runLoop(rig.loop, 250);
    rig.expectFail("timeout after 100ms");
    CHECK_EQ(srv.acceptedCount, 1);
  }
  {  // back-to-back before the loop turns: one connection, one pass
    Rig rig;
    Server srv(rig.loop, Server::Act::Hold);
    auto p = tcpProbe(srv.hostPort(), 1000);
    p->run(rig.loop, rig.bus);
    p->run(rig.loop, rig.bus);
    runLoop(rig.loop, 100);
    rig.expectPass();
    CHECK_EQ(srv.acceptedCount, 1);
    // and the probe is reusable once the first run has finished
    p->run(rig.loop, rig.bus);
    runLoop(rig.loop, 100);
    CHECK_EQ(rig.rec.events.size(), (size_t)2);
    CHECK_EQ(srv.acceptedCount, 2);
  }
}

void testCancelPublishesNothing() {
  Rig rig;
  Server srv(rig.loop, Server::Act::Hold);
  auto p = httpProbe("\"" + urlFor(srv) + "\"", 100);
  p->run(rig.loop, rig.bus);
  runLoop(rig.loop, 30);
  CHECK(p->running());
  p->cancel();
  CHECK(!p->running());
  runLoop(rig.loop, 200);  // past the (canceled) timeout
  CHECK_EQ(rig.rec.events.size(), (size_t)0);
  p->cancel();  // idle cancel is a no-op
  // cancel before the loop ever turned
  auto q = tcpProbe(srv.hostPort(), 100);
  q->run(rig.loop, rig.bus);
  q->cancel();
  runLoop(rig.loop, 150);
  CHECK_EQ(rig.rec.events.size(), (size_t)0);
}

void testSocketFailsImmediately() {
  Rig rig;
  Server srv(rig.loop, Server::Act::Hold);
  auto p = tcpProbe(srv.hostPort(), 100);
  struct rlimit saved, none;
  getrlimit(RLIMIT_NOFILE, &saved);
  none = saved;
  none.rlim_cur = 0;  // open fds stay valid; socket() now fails EMFILE
  setrlimit(RLIMIT_NOFILE, &none);
  p->run(rig.loop, rig.bus);
  setrlimit(RLIMIT_NOFILE, &saved);
  CHECK(!p->running());
  runLoop(rig.loop, 150);
  rig.expectFail(strerror(EMFILE));
  CHECK_EQ(srv.acceptedCount, 0);
}

void testBusDroppedInFlight() {
  Loop loop;
  Recorder rec;
  auto bus = std::make_shared<Bus>(loop);
  std::weak_ptr<Bus> weak = bus;
  bus->subscribe(&rec);
  Server srv(loop, Server::Act::Hold);
  auto hung = httpProbe("\"" + urlFor(srv) + "\"", 80);
  auto quick = tcpProbe(srv.hostPort(), 80);
  hung->run(loop, bus);
  quick->run(loop, bus);
  bus.reset();  // the owner lets go mid-flight; the runs keep it alive
  CHECK(!weak.expired());
  runLoop(loop, 200);
  // both verdicts landed on that bus, then the last reference went
  CHECK_EQ(rec.events.size(), (size_t)3);
  CHECK(!hung->running());
  CHECK(!quick->running());
  CHECK(weak.expired());

  // a probe dropped by ITS owner mid-flight finishes on its own too
  auto bus2 = std::make_shared<Bus>(loop);
  Recorder rec2;
  bus2->subscribe(&rec2);
  httpProbe("\"" + urlFor(srv) + "\"", 50)->run(loop, bus2);
  runLoop(loop, 120);
  CHECK_EQ(rec2.events.size(), (size_t)2);
  bus2->unsubscribe(&rec2);
}

void testParseErrors() {
  ProbeSpec s;
  std::string key, err;
  CHECK(!parseTcpProbe("db.internal:5432", &s, &err));
  CHECK(err.find("names are not resolved on the reactor") != std::string::npos);
  CHECK(err.find("health.exec") != std::string::npos);
  CHECK(!parseTcpProbe("127.0.0.1", &s, &err));
  CHECK(!parseTcpProbe("127.0.0.1:0", &s, &err));
  CHECK(!parseTcpProbe("127.0.0.1:65536", &s, &err));
  CHECK(!parseTcpProbe("::1:80", &s, &err));
  CHECK(parseTcpProbe("[::1]:80", &s, &err));
  CHECK(!parseHttpProbe(Json("https://127.0.0.1/"), &s, &key, &err));
  CHECK(err.find("health.exec") != std::string::npos);
  CHECK(!parseHttpProbe(Json("127.0.0.1/health"), &s, &key, &err));
  CHECK(err.find("malformed URL") != std::string::npos);
}

}  // namespace

int main() {
  logging::setLevel(logging::Level::Fatal);  // failures here are scripted
  int fdsBefore = countOpenFds();

  testTcpPass();
  testTcpRefused();
  testHttpStatuses();
  testRequestOnTheWire();
  testSplitStatusLine();
  testNoCrlfIn8K();
  testPeerCloses();
  testTimeout();
  testOverlapSkipsTick();
  testCancelPublishesNothing();
  testSocketFailsImmediately();
  testBusDroppedInFlight();
  testParseErrors();

  int fdsAfter = countOpenFds();
  CHECK(fdsBefore > 0);
  CHECK_EQ(fdsBefore, fdsAfter);

  if (failures) {
    fprintf(stderr, "%d probe test check(s) failed\n", failures);
    return 1;
  }
  printf("all probe tests passed\n");
  return 0;
}
