#include "cpilot/probe.hpp"

#include <arpa/inet.h>
#include <netinet/in.h>
#include <sys/epoll.h>
#include <unistd.h>

#include <strings.h>

#include <cerrno>
#include <cstring>

#include "cpilot/decode.hpp"
#include "cpilot/http.hpp"
#include "cpilot/log.hpp"
#include "cpilot/version.hpp"

namespace cpilot {
namespace health {

const char* const kProbeMalformed = "malformed response";
const char* const kProbeClosedEarly = "connection closed before response";

// ---------------- config ----------------

namespace {

bool parsePort(const std::string& text, int* out, std::string* err) {
  if (text.empty() || text.size() > 5) {
    *err = "port '" + text + "' must be a number between 1 and 65535";
    return false;
  }
  int port = 0;
  for (char c : text) {
    if (c < '0' || c > '9') {
      *err = "port '" + text + "' must be a number between 1 and 65535";
      return false;
    }
    port = port * 10 + (c - '0');
  }
  if (port < 1 || port > 65535) {
    *err = "port '" + text + "' must be a number between 1 and 65535";
    return false;
  }
  *out = port;
  return true;
}

// HOST[:PORT] -> sockaddr. HOST is an IPv4 literal, a bracketed IPv6
// literal, or `localhost` (127.0.0.1). defaultPort 0 means the port is
// required.
bool parseAuthority(const std::string& authority, int defaultPort,
                    ProbeSpec* out, std::string* err) {
  std::string host, portText;
  bool haveP = false, v6 = false;
  if (!authority.empty() && authority[0] == '[') {
    size_t close = authority.find(']');
    if (close == std::string::npos) {
      *err = "unterminated '[' in host";
      return false;
    }
    host = authority.substr(1, close - 1);
    v6 = true;
    std::string rest = authority.substr(close + 1);
    if (!rest.empty()) {
      if (rest[0] != ':') {
        *err = "unexpected text after ']' in host";
        return false;
      }
      haveP = true;
      portText = rest.substr(1);
    }
  } else {
    size_t colon = authority.rfind(':');
    if (colon != std::string::npos) {
      host = authority.substr(0, colon);
      portText = authority.substr(colon + 1);
      haveP = true;
    } else {
      host = authority;
    }
    if (host.find(':') != std::string::npos) {
      *err = "IPv6 literals must be bracketed, as in [::1]:8080";
      return false;
    }
  }
  if (host.empty()) {
    *err = "missing host";
    return false;
  }
  int port = defaultPort;
  if (haveP) {
    if (!parsePort(portText, &port, err)) return false;
  } else if (defaultPort == 0) {
    *err = "missing port, expected HOST:PORT";
    return false;
  }

  memset(&out->addr, 0, sizeof(out->addr));
  if (v6) {
    auto* sa = reinterpret_cast<struct sockaddr_in6*>(&out->addr);
    if (inet_pton(AF_INET6, host.c_str(), &sa->sin6_addr) != 1) {
      *err = "'" + host + "' is not a valid IPv6 literal";
      return false;
    }
    sa->sin6_family = AF_INET6;
    sa->sin6_port = htons((uint16_t)port);
    out->addrLen = sizeof(*sa);
  } else {
    auto* sa = reinterpret_cast<struct sockaddr_in*>(&out->addr);
    const char* literal = host == "localhost" ? "127.0.0.1" : host.c_str();
    if (inet_pton(AF_INET, literal, &sa->sin_addr) != 1) {
      *err = "host '" + host +
             "' is not an IP literal: names are not resolved on the "
             "reactor (use an IP address or 'localhost', or a health.exec "
             "check where DNS is needed)";
      return false;
    }
    sa->sin_family = AF_INET;
    sa->sin_port = htons((uint16_t)port);
    out->addrLen = sizeof(*sa);
  }
  out->target = (v6 ? "[" + host + "]" : host) + ":" + std::to_string(port);
  return true;
}

bool hasCtlOrSpace(const std::string& s) {
  for (unsigned char c : s)
    if (c <= ' ' || c == 0x7f) return true;
  return false;
}

bool parseProbeUrl(const std::string& url, ProbeSpec* out, std::string* err) {
  static const std::string kHttp = "http://";
  if (url.compare(0, 8, "https://") == 0) {
    *err = "https is not supported: TLS checks are not run on the reactor "
           "(use a health.exec check instead)";
    return false;
  }
  if (url.compare(0, kHttp.size(), kHttp) != 0) {
    *err = "malformed URL '" + url + "': expected http://HOST[:PORT][/path]";
    return false;
  }
  if (hasCtlOrSpace(url) || url.find('#') != std::string::npos) {
    *err = "malformed URL '" + url +
           "': whitespace, control characters and fragments are not allowed";
    return false;
  }
  std::string rest = url.substr(kHttp.size());
  size_t end = rest.find_first_of("/?");
  std::string authority = rest.substr(0, end);
  std::string tail = end == std::string::npos ? "" : rest.substr(end);
  if (authority.empty() || authority.find('@') != std::string::npos) {
    *err = "malformed URL '" + url + "': expected http://HOST[:PORT][/path]";
    return false;
  }
  std::string aerr;
  if (!parseAuthority(authority, 80, out, &aerr)) {
    *err = "malformed URL '" + url + "': " + aerr;
    // the no-DNS rule and port range read better without the prefix
    if (aerr.compare(0, 5, "host ") == 0 || aerr.compare(0, 5, "port ") == 0)
      *err = aerr;
    return false;
  }
  out->hostHeader = authority;
  if (tail.empty()) out->path = "/";
  else if (tail[0] == '?') out->path = "/" + tail;
  else out->path = tail;
  return true;
}

}  // namespace

bool parseTcpProbe(const std::string& hostPort, ProbeSpec* out,
                   std::string* err) {
  out->kind = ProbeSpec::Kind::Tcp;
  return parseAuthority(hostPort, 0, out, err);
}

namespace {

bool equalsIgnoreCase(const std::string& a, const char* b) {
  return strcasecmp(a.c_str(), b) == 0;
}

// `health.http` and `jobs[].http` share every rule; an action adds the
// methods that change state, `body`, and the refusal of the headers the
// daemon sets itself
bool parseHttpSpec(const Json& raw, bool action, ProbeSpec* out,
                   std::string* errKey, std::string* err) {
  out->kind = ProbeSpec::Kind::Http;
  out->action = action;
  errKey->clear();
  if (raw.isString()) {
    out->url = raw.str();
    return parseProbeUrl(raw.str(), out, err);
  }
  if (!raw.isObject()) {
    *err = "must be a URL string or an object";
    return false;
  }
  bool keysOk =
      action ? decode::checkKeys(
                   raw, {"url", "method", "headers", "expect", "body"}, err)
             : decode::checkKeys(raw, {"url", "method", "headers", "expect"},
                                 err);
  if (!keysOk) return false;

  const Json* url = raw.find("url");
  if (!url || !url->isString() || url->str().empty()) {
    *errKey = ".url";
    *err = "is required and must be a string";
    return false;
  }
  if (!parseProbeUrl(url->str(), out, err)) {
    *errKey = ".url";
    return false;
  }
  out->url = url->str();

  if (const Json* method = raw.find("method")) {
    bool ok = method->isString() &&
              (method->str() == "GET" || method->str() == "HEAD");
    if (action && !ok && method->isString())
      for (const char* m : {"POST", "PUT", "PATCH", "DELETE"})
        ok = ok || method->str() == m;
    if (!ok) {
      *errKey = ".method";
      *err = action ? "must be one of 'GET', 'HEAD', 'POST', 'PUT', 'PATCH' "
                      "or 'DELETE'"
                    : "must be 'GET' or 'HEAD'";
      return false;
    }
    out->method = method->str();
  }

  if (const Json* body = action ? raw.find("body") : nullptr) {
    if (!body->isNull()) {
      *errKey = ".body";
      if (!body->isString()) {
        *err = "must be a string";
        return false;
      }
      if (body->str().size() > kActionMaxBody) {
        *err = "must be at most " + std::to_string(kActionMaxBody) +
               " bytes, got " + std::to_string(body->str().size());
        return false;
      }
      if (out->method == "GET" || out->method == "HEAD") {
        *err = "cannot be sent with method '" + out->method +
               "': use POST, PUT, PATCH or DELETE";
        return false;
      }
      out->hasBody = true;
      out->body = body->str();
      errKey->clear();
    }
  }

  if (const Json* headers = raw.find("headers")) {
    if (!headers->isNull() && !headers->isObject()) {
      *errKey = ".headers";
      *err = "must be an object of strings";
      return false;
    }
    for (auto& kv : headers->object()) {
      *errKey = ".headers";
      if (!kv.second.isString()) {
        *err = "must be an object of strings";
        return false;
      }
      if (kv.first.find_first_of("\r\n") != std::string::npos ||
          kv.second.str().find_first_of("\r\n") != std::string::npos) {
        *err = "names and values must not contain CR or LF";
        return false;
      }
      if (kv.first.empty() || kv.first.find(':') != std::string::npos ||
          hasCtlOrSpace(kv.first)) {
        *err = "names must be non-empty and free of ':' and whitespace";
        return false;
      }
      if (action)
        for (const char* own : {"Host", "Connection", "Content-Length",
                                "Transfer-Encoding"})
          if (equalsIgnoreCase(kv.first, own)) {
            *err = "'" + kv.first + "' is set by the daemon and cannot be "
                   "configured";
            return false;
          }
      out->headers.emplace_back(kv.first, kv.second.str());
    }
    errKey->clear();
  }

  if (const Json* expect = raw.find("expect")) {
    auto addCode = [&](const Json& v) {
      if (!v.isInt()) {
        *err = "must be an int or a list of ints";
        return false;
      }
      if (v.asInt() < 100 || v.asInt() > 599) {
        *err = "entries must be between 100 and 599, got " +
               std::to_string(v.asInt());
        return false;
      }
      out->expect.push_back((int)v.asInt());
      return true;
    };
    *errKey = ".expect";
    if (expect->isArray()) {
      if (expect->array().empty()) {
        *err = "must not be an empty list";
        return false;
      }
      for (auto& v : expect->array())
        if (!addCode(v)) return false;
    } else if (!addCode(*expect)) {
      return false;
    }
    errKey->clear();
  }
  return true;
}

}  // namespace

bool parseHttpProbe(const Json& raw, ProbeSpec* out, std::string* errKey,
                    std::string* err) {
  return parseHttpSpec(raw, false, out, errKey, err);
}

bool parseHttpAction(const Json& raw, ProbeSpec* out, std::string* errKey,
                     std::string* err) {
  return parseHttpSpec(raw, true, out, errKey, err);
}

std::string buildProbeRequest(const ProbeSpec& spec) {
  std::string req = spec.method + " " + spec.path + " HTTP/1.1\r\n";
  req += "Host: " + spec.hostHeader + "\r\n";
  req += std::string("User-Agent: containerpilot/") + kVersion + "\r\n";
  req += "Accept: */*\r\n";
  req += "Connection: close\r\n";
  // a length-less POST, PUT or PATCH is refused (411) by many servers
  if (spec.hasBody || spec.method == "POST" || spec.method == "PUT" ||
      spec.method == "PATCH")
    req += "Content-Length: " + std::to_string(spec.body.size()) + "\r\n";
  for (auto& kv : spec.headers) req += kv.first + ": " + kv.second + "\r\n";
  req += "\r\n";
  req += spec.body;
  return req;
}

std::string probeDurationString(Duration d) {
  long long ns = (long long)d.count();
  if (ns % 1000000000LL == 0) return std::to_string(ns / 1000000000LL) + "s";
  if (ns % 1000000LL == 0) return std::to_string(ns / 1000000LL) + "ms";
  if (ns % 1000LL == 0) return std::to_string(ns / 1000LL) + "us";
  return std::to_string(ns) + "ns";
}

// ---------------- runtime ----------------

Probe::Probe(ProbeSpec spec, std::string name)
    : spec_(std::move(spec)), name_(std::move(name)) {
  if (spec_.kind == ProbeSpec::Kind::Http) request_ = buildProbeRequest(spec_);
}

Probe::~Probe() {
  // only reachable with a live socket when the loop itself was destroyed
  // mid-run (its callbacks held the last references); the epoll set is
  // gone with it, so there is nothing to unwatch
  if (fd_ >= 0) close(fd_);
}

void Probe::run(Loop& loop, std::shared_ptr<Bus> bus) {
  if (running()) {
    // single-instance skip: a tick that finds the previous probe still
    // in flight is dropped, never queued
    LOG_DEBUG("%s still in flight, skipping this tick", name_.c_str());
    return;
  }
  LOG_DEBUG("%s probe %s", name_.c_str(), spec_.target.c_str());
  loop_ = &loop;
  bus_ = std::move(bus);
  sent_ = 0;
  rbuf_.clear();
  code_ = 0;
  verdict_.clear();
  drained_ = 0;
  headDone_ = bodyKnown_ = false;
  bodyEnd_ = 0;

  fd_ = socket(spec_.addr.ss_family, SOCK_STREAM | SOCK_NONBLOCK | SOCK_CLOEXEC,
               0);
  if (fd_ < 0) {
    failErrno(errno);
    return;
  }
  int rc;
  do {
    rc = connect(fd_, reinterpret_cast<const struct sockaddr*>(&spec_.addr),
                 spec_.addrLen);
  } while (rc != 0 && errno == EINTR);
  if (rc != 0 && errno != EINPROGRESS) {
    failErrno(errno);
    return;
  }

  auto self = shared_from_this();
  state_ = State::Connecting;
  try {
    loop.watchFd(fd_, EPOLLOUT, [this, self](uint32_t ev) { onIo(ev); });
  } catch (const std::exception&) {
    // epoll_ctl ADD failed (ENOMEM / ENOSPC): the fd was never watched
    int err = errno;
    close(fd_);
    fd_ = -1;
    state_ = State::Idle;
    failErrno(err);
    return;
  }
  if (spec_.timeout > Duration(0))
    timer_ = loop.addTimeout(spec_.timeout, [this, self] {
      timer_ = 0;
      onTimeout();
    });
  if (rc == 0) onConnected();
}

void Probe::cancel() {
  if (!running()) return;
  LOG_DEBUG("%s canceled in flight", name_.c_str());
  teardown();
}

std::shared_ptr<Bus> Probe::teardown(bool orderly) {
  if (fd_ >= 0) {
    if (state_ != State::Idle) loop_->unwatchFd(fd_);
    // abortive close: the daemon always closes first, so an orderly
    // close would park every check's port in TIME_WAIT on this side.
    // After the peer's FIN the peer closed first and holds the TIME_WAIT,
    // so an action that read its response out closes orderly.
    if (!orderly) {
      struct linger lg = {1, 0};
      setsockopt(fd_, SOL_SOCKET, SO_LINGER, &lg, sizeof(lg));
    }
    close(fd_);
    fd_ = -1;
  }
  if (timer_) {
    loop_->cancelTimer(timer_);
    timer_ = 0;
  }
  state_ = State::Idle;
  rbuf_.clear();
  return std::move(bus_);
}

void Probe::pass() {
  auto bus = teardown();
  LOG_DEBUG("%s passed", name_.c_str());
  bus->publish(Event{EventCode::ExitSuccess, name_});
}

void Probe::fail(const std::string& reason, bool timedOut) {
  auto bus = teardown();
  // a failed action is the job's own outcome, like a non-zero exit
  if (timedOut || spec_.action)
    LOG_WARN("%s: %s", name_.c_str(), reason.c_str());
  else
    LOG_ERROR("%s: %s", name_.c_str(), reason.c_str());
  bus->publish(Event{EventCode::ExitFailed, name_});
  bus->publish(Event{EventCode::Error, name_ + ": " + reason});
}

void Probe::failErrno(int err) {
  // once connected, a reset is the peer going away without answering
  if (state_ != State::Idle && state_ != State::Connecting &&
      (err == ECONNRESET || err == EPIPE)) {
    fail(kProbeClosedEarly);
    return;
  }
  fail(strerror(err));
}

void Probe::onTimeout() {
  if (!running()) return;
  if (state_ == State::Draining) {
    // the verdict was decided at the status line and stands
    finishDrain(false);
    return;
  }
  fail("timeout after " + probeDurationString(spec_.timeout), true);
}

void Probe::onIo(uint32_t events) {
  switch (state_) {
    case State::Connecting: {
      int err = 0;
      socklen_t len = sizeof(err);
      if (getsockopt(fd_, SOL_SOCKET, SO_ERROR, &err, &len) != 0) err = errno;
      if (err != 0) {
        failErrno(err);
        break;
      }
      // Trust the socket, not the event mask: the loop hands out a whole
      // epoll batch, and an fd number closed and reused earlier in the
      // batch can still have the previous socket's event queued behind
      // it. Still connecting means this wakeup was not ours; the timeout
      // timer bounds the wait either way.
      struct sockaddr_storage peer;
      socklen_t plen = sizeof(peer);
      if (getpeername(fd_, reinterpret_cast<struct sockaddr*>(&peer),
                      &plen) != 0) {
        if (errno != ENOTCONN) failErrno(errno);
        break;
      }
      onConnected();
      break;
    }
    // once connected, the write/read itself reports EPOLLERR/EPOLLHUP
    // conditions (as an errno or as end-of-stream), so every wakeup
    // makes progress or ends the run
    case State::Sending:
      onWritable();
      break;
    case State::Reading:
      onReadable();
      break;
    case State::Draining:
      onDrainReadable();
      break;
    case State::Idle:
      break;
  }
}

void Probe::onConnected() {
  if (spec_.kind == ProbeSpec::Kind::Tcp) {
    pass();
    return;
  }
  state_ = State::Sending;
  onWritable();
}

void Probe::onWritable() {
  while (sent_ < request_.size()) {
    ssize_t n = send(fd_, request_.data() + sent_, request_.size() - sent_,
                     MSG_NOSIGNAL);
    if (n > 0) {
      sent_ += (size_t)n;
    } else if (n < 0 && errno == EINTR) {
      continue;
    } else if (n < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) {
      return;  // short write: EPOLLOUT stays armed
    } else {
      failErrno(n < 0 ? errno : EPIPE);
      return;
    }
  }
  state_ = State::Reading;
  loop_->modifyFd(fd_, EPOLLIN);
}

void Probe::onReadable() {
  char buf[2048];
  while (true) {
    size_t room = kProbeMaxStatusLine - rbuf_.size();
    ssize_t n = recv(fd_, buf, room < sizeof(buf) ? room : sizeof(buf), 0);
    if (n > 0) {
      // the CRLF may straddle two segments: rescan from one byte back
      size_t from = rbuf_.empty() ? 0 : rbuf_.size() - 1;
      rbuf_.append(buf, (size_t)n);
      size_t crlf = rbuf_.find("\r\n", from);
      if (crlf != std::string::npos) {
        judgeStatusLine(crlf);
        return;
      }
      if (rbuf_.size() >= kProbeMaxStatusLine) {
        fail(kProbeMalformed);
        return;
      }
    } else if (n == 0) {
      fail(kProbeClosedEarly);
      return;
    } else if (errno == EINTR) {
      continue;
    } else if (errno == EAGAIN || errno == EWOULDBLOCK) {
      return;
    } else {
      failErrno(errno);
      return;
    }
  }
}

// "HTTP/1.x SSS" followed by end of line or a space; nothing after the
// status line is read
void Probe::judgeStatusLine(size_t crlf) {
  const std::string& l = rbuf_;
  auto digit = [&](size_t i) { return l[i] >= '0' && l[i] <= '9'; };
  if (crlf < 12 || l.compare(0, 7, "HTTP/1.") != 0 || !digit(7) ||
      l[8] != ' ' || !digit(9) || !digit(10) || !digit(11) ||
      (crlf > 12 && l[12] != ' ')) {
    fail(kProbeMalformed);
    return;
  }
  int code = (l[9] - '0') * 100 + (l[10] - '0') * 10 + (l[11] - '0');
  bool ok = false;
  if (spec_.expect.empty()) {
    ok = code >= 200 && code <= 299;
  } else {
    for (int want : spec_.expect) ok = ok || want == code;
  }
  if (spec_.action) {
    code_ = code;
    if (!ok) verdict_ = "unexpected status " + std::to_string(code);
    beginDrain(crlf);
    return;
  }
  if (ok) pass();
  else fail("unexpected status " + std::to_string(code));
}

// ---------------- actions: read the response out ----------------
//
// The verdict stands from the status line on. The server is doing real
// work for an action, and a reset while it writes its response is an error
// in its log, so the rest is read and discarded until the peer closes, the
// announced Content-Length has arrived, kActionMaxDrain bytes went by or
// the deadline hits, whichever is first.

void Probe::beginDrain(size_t crlf) {
  state_ = State::Draining;
  drained_ = rbuf_.size();
  // rbuf_ keeps the head (from the status line's CRLF on) until it ends
  rbuf_.erase(0, crlf);
  if (drainComplete()) {
    finishDrain(false);
    return;
  }
  onDrainReadable();
}

// called after every read: looks for the end of the head once, then only
// compares counters
bool Probe::drainComplete() {
  if (!headDone_) {
    // rbuf_ starts at the status line's CRLF, so a response without
    // header lines ends its head right there
    size_t end = rbuf_.find("\r\n\r\n");
    if (end != std::string::npos) {
      headDone_ = true;
      http::Headers headers;
      http::parseHeaderLines(rbuf_, 2, end, &headers);
      size_t headEnd = drained_ - (rbuf_.size() - (end + 4));
      bool noBody = spec_.method == "HEAD" || code_ < 200 || code_ == 204 ||
                    code_ == 304;
      if (noBody) {
        bodyKnown_ = true;
        bodyEnd_ = headEnd;
      } else if (!http::isChunked(headers) && headers.count("content-length")) {
        size_t len = http::contentLength(headers);
        bodyKnown_ = true;
        // a length that wraps is one the cap ends
        bodyEnd_ = len > kActionMaxDrain ? kActionMaxDrain + 1 : headEnd + len;
      }
      rbuf_.clear();
    } else if (rbuf_.size() > kActionMaxHead) {
      // no length will be learnt from a head this long: the response
      // ends at close or at the cap
      headDone_ = true;
      rbuf_.clear();
    }
  }
  if (bodyKnown_ && drained_ >= bodyEnd_) return true;
  return drained_ >= kActionMaxDrain;
}

void Probe::onDrainReadable() {
  char buf[16384];
  while (true) {
    ssize_t n = recv(fd_, buf, sizeof(buf), 0);
    if (n > 0) {
      drained_ += (size_t)n;
      if (!headDone_) rbuf_.append(buf, (size_t)n);
      if (drainComplete()) {
        finishDrain(false);
        return;
      }
    } else if (n == 0) {
      finishDrain(true);
      return;
    } else if (errno == EINTR) {
      continue;
    } else if (errno == EAGAIN || errno == EWOULDBLOCK) {
      return;
    } else {
      finishDrain(false);  // reset by the peer: nothing more will come
      return;
    }
  }
}

void Probe::finishDrain(bool peerClosed) {
  auto bus = teardown(peerClosed);
  if (verdict_.empty()) {
    LOG_INFO("%s: %s %s answered %d", name_.c_str(), spec_.method.c_str(),
             spec_.url.c_str(), code_);
    bus->publish(Event{EventCode::ExitSuccess, name_});
    return;
  }
  LOG_WARN("%s: %s", name_.c_str(), verdict_.c_str());
  bus->publish(Event{EventCode::ExitFailed, name_});
  bus->publish(Event{EventCode::Error, name_ + ": " + verdict_});
}

}  // namespace health
}  // namespace cpilot
