#include "cpilot/http.hpp"

#include <sys/epoll.h>

#include <arpa/inet.h>
#include <fcntl.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <poll.h>
#include <openssl/err.h>
#include <openssl/ssl.h>
#include <sys/socket.h>
#include <sys/un.h>
#include <unistd.h>

#include <cctype>
#include <cstring>

#include "cpilot/log.hpp"

namespace cpilot {
namespace http {

const char* statusText(int code) {
  switch (code) {
    case 200: return "OK";
    case 400: return "Bad Request";
    case 404: return "Not Found";
    case 405: return "Method Not Allowed";
    case 409: return "Conflict";
    case 411: return "Length Required";
    case 413: return "Payload Too Large";
    case 422: return "Unprocessable Entity";
    case 431: return "Request Header Fields Too Large";
    case 500: return "Internal Server Error";
    default: return "";
  }
}

// hardening limits: the reference gets equivalent protection from
// net/http's defaults (1 MiB header cap, read deadlines)
static constexpr size_t kMaxHeaderBytes = 64 * 1024;
static constexpr size_t kMaxBodyBytes = 4 * 1024 * 1024;
static constexpr int kConnDeadlineSecs = 10;
static constexpr int kListenAttempts = 10;  // one second apart

struct Server::Conn {
  int fd = -1;
  std::string inbuf;
  bool headersDone = false;
  size_t contentLength = 0;
  size_t headerEnd = 0;
  Request req;
  // async response write state (flushed via EPOLLOUT, never by
  // blocking the reactor)
  std::string outbuf;
  size_t outoff = 0;
  bool writing = false;
  uint64_t deadlineTimer = 0;
};

Server::Server(Loop& loop, Handler handler)
    : loop_(loop), handler_(std::move(handler)) {}

Server::~Server() { stop(); }

static void setNonblock(int fd) {
  fcntl(fd, F_SETFL, fcntl(fd, F_GETFL, 0) | O_NONBLOCK);
  fcntl(fd, F_SETFD, FD_CLOEXEC);
}

// Fill a unix sockaddr; a path that does not fit is an error, never
// truncated (the socket would live at a path nobody asked for).
static bool unixAddr(const std::string& path, struct sockaddr_un* addr,
                     std::string* err) {
  memset(addr, 0, sizeof(*addr));
  addr->sun_family = AF_UNIX;
  if (path.size() >= sizeof(addr->sun_path)) {
    *err = "unix socket path too long (" + std::to_string(path.size()) +
           " bytes, limit " + std::to_string(sizeof(addr->sun_path) - 1) +
           "): " + path;
    return false;
  }
  memcpy(addr->sun_path, path.data(), path.size());
  return true;
}

// takes ownership of fd (which may be -1 from a failed socket())
bool Server::bindAndListen(int fd, const struct sockaddr* addr, socklen_t len,
                           std::string* err) {
  if (fd < 0 || bind(fd, addr, len) != 0 || listen(fd, 128) != 0) {
    *err = strerror(errno);
    if (fd >= 0) close(fd);
    return false;
  }
  setNonblock(fd);
  listenFd_ = fd;
  loop_.watchFd(fd, EPOLLIN, [this](uint32_t) { acceptReady(); });
  return true;
}

bool Server::listenUnix(const std::string& path, std::string* err) {
  struct sockaddr_un addr;
  if (!unixAddr(path, &addr, err)) return false;
  int fd = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
  return bindAndListen(fd, (struct sockaddr*)&addr, sizeof(addr), err);
}

bool Server::listenTcp(const std::string& ip, int port, std::string* err) {
  struct sockaddr_in addr;
  memset(&addr, 0, sizeof(addr));
  addr.sin_family = AF_INET;
  addr.sin_port = htons(port);
  // empty, 0.0.0.0 and unparseable addresses all mean "any"
  if (inet_pton(AF_INET, ip.c_str(), &addr.sin_addr) != 1)
    addr.sin_addr.s_addr = INADDR_ANY;
  int fd = socket(AF_INET, SOCK_STREAM | SOCK_CLOEXEC, 0);
  int one = 1;
  if (fd >= 0) setsockopt(fd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
  return bindAndListen(fd, (struct sockaddr*)&addr, sizeof(addr), err);
}

bool Server::listenRetrying(ListenFn listen, const std::string& name,
                            const std::string& addr,
                            std::function<void()> onBound, int attempt) {
  std::string err;
  if (listen(&err)) {
    onBound();
    return true;
  }
  if (attempt == 1)
    LOG_WARN("%s: error listening at %s: %s (retrying)", name.c_str(),
             addr.c_str(), err.c_str());
  if (attempt >= kListenAttempts) {
    // parity with the reference's log.Fatal after exhausted retries
    logging::logf(logging::Level::Fatal, "error listening to socket at %s: %s",
                  addr.c_str(), err.c_str());
    return false;
  }
  retryTimer_ = loop_.addTimeout(std::chrono::seconds(1), [=] {
    retryTimer_ = 0;
    listenRetrying(listen, name, addr, onBound, attempt + 1);
  });
  return false;
}

void Server::stop() {
  if (retryTimer_) {
    loop_.cancelTimer(retryTimer_);
    retryTimer_ = 0;
  }
  if (listenFd_ >= 0) {
    loop_.unwatchFd(listenFd_);
    close(listenFd_);
    listenFd_ = -1;
  }
  // closeConn also cancels the deadline timer, whose callback captures
  // this server
  while (!conns_.empty()) {
    std::shared_ptr<Conn> c = conns_.begin()->second;  // outlives the erase
    closeConn(c);
  }
}

void Server::acceptReady() {
  while (true) {
    int fd = accept(listenFd_, nullptr, nullptr);
    if (fd < 0) return;
    setNonblock(fd);
    auto c = std::make_shared<Conn>();
    c->fd = fd;
    conns_[fd] = c;
    armDeadline(c);
    loop_.watchFd(fd, EPOLLIN | EPOLLHUP, [this, c](uint32_t) {
      if (c->writing)
        connWritable(c);
      else
        connReadable(c);
    });
  }
}

// Hard per-connection deadline: a client that dribbles its request
// (slow-loris) or refuses to read the response is dropped, freeing the
// fd and buffer. Armed on accept and re-armed once when the response
// starts.
void Server::armDeadline(const std::shared_ptr<Conn>& c) {
  if (c->deadlineTimer) loop_.cancelTimer(c->deadlineTimer);
  c->deadlineTimer =
      loop_.addTimeout(std::chrono::seconds(kConnDeadlineSecs), [this, c] {
        c->deadlineTimer = 0;
        closeConn(c);
      });
}

void Server::closeConn(const std::shared_ptr<Conn>& c) {
  if (c->fd < 0) return;
  if (c->deadlineTimer) {
    loop_.cancelTimer(c->deadlineTimer);
    c->deadlineTimer = 0;
  }
  loop_.unwatchFd(c->fd);
  close(c->fd);
  conns_.erase(c->fd);
  c->fd = -1;
}

// Serialize the response and flush as much as the socket accepts now;
// the remainder drains via EPOLLOUT so a slow reader never blocks the
// reactor (it is dropped at the connection deadline instead).
void Server::beginWrite(const std::shared_ptr<Conn>& c,
                        const Response& resp) {
  std::string out = "HTTP/1.1 " + std::to_string(resp.status) + " " +
                    statusText(resp.status) + "\r\n";
  out += "Content-Type: " + resp.contentType + "\r\n";
  out += "Content-Length: " + std::to_string(resp.body.size()) + "\r\n";
  out += "Connection: close\r\n\r\n";
  out += resp.body;
  c->outbuf = std::move(out);
  c->outoff = 0;
  c->writing = true;
  armDeadline(c);  // fresh deadline for the write phase
  connWritable(c);
}

void Server::connWritable(std::shared_ptr<Conn> c) {
  if (c->fd < 0) return;
  while (c->outoff < c->outbuf.size()) {
    ssize_t n =
        write(c->fd, c->outbuf.data() + c->outoff, c->outbuf.size() - c->outoff);
    if (n > 0) {
      c->outoff += n;
    } else if (n < 0 && errno == EINTR) {
      continue;
    } else if (n < 0 && errno == EAGAIN) {
      loop_.modifyFd(c->fd, EPOLLOUT | EPOLLHUP);
      return;  // resume when the socket drains
    } else {
      break;  // peer gone
    }
  }
  closeConn(c);
}

void Server::connReadable(std::shared_ptr<Conn> c) {
  char buf[8192];
  while (true) {
    ssize_t n = read(c->fd, buf, sizeof(buf));
    if (n > 0) {
      c->inbuf.append(buf, n);
      if (c->inbuf.size() > kMaxHeaderBytes + kMaxBodyBytes) {
        closeConn(c);
        return;
      }
      continue;
    }
    if (n < 0 && errno == EAGAIN) break;
    if (n < 0 && errno == EINTR) continue;
    // EOF or error before a complete request
    if (!c->headersDone || c->inbuf.size() < c->headerEnd + c->contentLength) {
      closeConn(c);
      return;
    }
    break;
  }

  if (!c->headersDone) {
    size_t end = c->inbuf.find("\r\n\r\n");
    if (end == std::string::npos) {
      if (c->inbuf.size() > kMaxHeaderBytes) beginWrite(c, errorResponse(431));
      return;  // wait for more (bounded by the connection deadline)
    }
    c->headerEnd = end + 4;
    if (c->headerEnd > kMaxHeaderBytes) {
      beginWrite(c, errorResponse(431));
      return;
    }
    if (!parseRequestHead(c->inbuf, c->headerEnd, &c->req)) {
      closeConn(c);
      return;
    }
    c->contentLength = contentLength(c->req.headers);
    c->headersDone = true;
    // no chunked request support: require a length (net/http would
    // dechunk; our endpoints only ever see small bodies)
    if (c->req.headers.count("transfer-encoding")) {
      beginWrite(c, errorResponse(411));
      return;
    }
    if (c->contentLength > kMaxBodyBytes) {
      beginWrite(c, errorResponse(413));
      return;
    }
  }
  if (c->inbuf.size() < c->headerEnd + c->contentLength) return;
  c->req.body = c->inbuf.substr(c->headerEnd, c->contentLength);

  beginWrite(c, handler_(c->req));
}

Response Server::errorResponse(int status) {
  Response resp;
  resp.status = status;
  resp.body = std::string(statusText(status)) + "\n";
  return resp;
}

// ---------------- message-head parsing ----------------

static std::string toLower(std::string s) {
  for (auto& ch : s) ch = (char)tolower((unsigned char)ch);
  return s;
}

void parseHeaderLines(const std::string& head, size_t pos, size_t end,
                      Headers* out) {
  while (pos < end) {
    size_t eol = head.find("\r\n", pos);
    if (eol == std::string::npos || eol > end) break;
    const char* c = (const char*)memchr(head.data() + pos, ':', eol - pos);
    if (c) {
      size_t colon = c - head.data();
      size_t vstart = colon + 1;
      while (vstart < eol && head[vstart] == ' ') vstart++;
      (*out)[toLower(head.substr(pos, colon - pos))] =
          head.substr(vstart, eol - vstart);
    }
    pos = eol + 2;
  }
}

bool parseRequestLine(const std::string& line, Request* req) {
  size_t sp1 = line.find(' ');
  size_t sp2 = line.rfind(' ');
  if (sp1 == std::string::npos || sp2 == sp1) return false;
  req->method = line.substr(0, sp1);
  std::string target = line.substr(sp1 + 1, sp2 - sp1 - 1);
  size_t q = target.find('?');
  req->path = target.substr(0, q);
  req->query = q == std::string::npos ? "" : target.substr(q + 1);
  return true;
}

bool parseRequestHead(const std::string& buf, size_t headerEnd, Request* req) {
  size_t lineEnd = buf.find("\r\n");
  if (lineEnd == std::string::npos || lineEnd + 4 > headerEnd) return false;
  if (!parseRequestLine(buf.substr(0, lineEnd), req)) return false;
  parseHeaderLines(buf, lineEnd + 2, headerEnd - 4, &req->headers);
  return true;
}

int parseStatus(const std::string& resp) {
  if (resp.compare(0, 5, "HTTP/") != 0) return -1;
  // no space at all: find() gives npos and atoi reads from the start
  return atoi(resp.c_str() + resp.find(' ') + 1);
}

size_t contentLength(const Headers& headers) {
  auto it = headers.find("content-length");
  return it == headers.end() ? 0 : (size_t)atoll(it->second.c_str());
}

bool isChunked(const Headers& headers) {
  auto it = headers.find("transfer-encoding");
  return it != headers.end() &&
         toLower(it->second).find("chunked") != std::string::npos;
}

// ---------------- blocking client ----------------

const char* const kBodyTooLarge = "response body too large";

void CancelToken::arm(int fd) {
  std::lock_guard<std::mutex> l(mu_);
  fd_ = fd;
  if (cancelled_) ::shutdown(fd, SHUT_RDWR);
}

void CancelToken::disarm() {
  std::lock_guard<std::mutex> l(mu_);
  fd_ = -1;
}

void CancelToken::cancel() {
  std::lock_guard<std::mutex> l(mu_);
  cancelled_ = true;
  if (fd_ >= 0) ::shutdown(fd_, SHUT_RDWR);
}

bool CancelToken::cancelled() {
  std::lock_guard<std::mutex> l(mu_);
  return cancelled_;
}

namespace {

void setIoTimeout(int fd, int timeoutMs) {
  struct timeval tv;
  tv.tv_sec = timeoutMs / 1000;
  tv.tv_usec = (timeoutMs % 1000) * 1000;
  setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof(tv));
  setsockopt(fd, SOL_SOCKET, SO_SNDTIMEO, &tv, sizeof(tv));
}

int connectTarget(const std::string& target, std::string* err) {
  int fd = -1;
  if (target.rfind("unix:", 0) == 0) {
    struct sockaddr_un addr;
    if (!unixAddr(target.substr(5), &addr, err)) return -1;
    fd = socket(AF_UNIX, SOCK_STREAM | SOCK_CLOEXEC, 0);
    if (fd < 0 || connect(fd, (struct sockaddr*)&addr, sizeof(addr)) != 0) {
      *err = strerror(errno);
      if (fd >= 0) close(fd);
      return -1;
    }
  } else {
    std::string host = target;
    std::string port = "80";
    size_t colon = target.rfind(':');
    if (colon != std::string::npos) {
      host = target.substr(0, colon);
      port = target.substr(colon + 1);
    }
    struct addrinfo hints;
    memset(&hints, 0, sizeof(hints));
    hints.ai_family = AF_UNSPEC;
    hints.ai_socktype = SOCK_STREAM;
    struct addrinfo* res = nullptr;
    int rc = getaddrinfo(host.c_str(), port.c_str(), &hints, &res);
    if (rc != 0) {
      *err = gai_strerror(rc);
      return -1;
    }
    for (struct addrinfo* ai = res; ai; ai = ai->ai_next) {
      fd = socket(ai->ai_family, ai->ai_socktype | SOCK_CLOEXEC,
                  ai->ai_protocol);
      if (fd < 0) continue;
      if (connect(fd, ai->ai_addr, ai->ai_addrlen) == 0) break;
      close(fd);
      fd = -1;
    }
    freeaddrinfo(res);
    if (fd < 0) *err = "connection refused";
  }
  return fd;
}

// thin transport abstraction so the request logic is shared between
// plain sockets and TLS sessions
struct Transport {
  int fd = -1;
  SSL_CTX* ctx = nullptr;
  SSL* ssl = nullptr;

  ~Transport() {
    if (ssl) {
      SSL_shutdown(ssl);
      SSL_free(ssl);
    }
    if (ctx) SSL_CTX_free(ctx);
    if (fd >= 0) close(fd);
  }

  bool startTls(const std::string& host, const TlsOptions& tls,
                std::string* err) {
    ctx = SSL_CTX_new(TLS_client_method());
    if (!ctx) {
      *err = "SSL_CTX_new failed";
      return false;
    }
    if (!tls.caFile.empty() || !tls.caPath.empty()) {
      if (SSL_CTX_load_verify_locations(
              ctx, tls.caFile.empty() ? nullptr : tls.caFile.c_str(),
              tls.caPath.empty() ? nullptr : tls.caPath.c_str()) != 1) {
        *err = "failed to load CA certificates";
        return false;
      }
    } else {
      SSL_CTX_set_default_verify_paths(ctx);
    }
    if (!tls.certFile.empty() &&
        (SSL_CTX_use_certificate_chain_file(ctx, tls.certFile.c_str()) != 1 ||
         SSL_CTX_use_PrivateKey_file(ctx, tls.keyFile.c_str(),
                                     SSL_FILETYPE_PEM) != 1)) {
      *err = "failed to load client certificate/key";
      return false;
    }
    SSL_CTX_set_verify(
        ctx, tls.insecureSkipVerify ? SSL_VERIFY_NONE : SSL_VERIFY_PEER,
        nullptr);
    ssl = SSL_new(ctx);
    SSL_set_fd(ssl, fd);
    std::string sniHost = tls.serverName.empty() ? host : tls.serverName;
    // strip :port for SNI/verification
    size_t colon = sniHost.rfind(':');
    if (colon != std::string::npos) sniHost = sniHost.substr(0, colon);
    SSL_set_tlsext_host_name(ssl, sniHost.c_str());
    if (!tls.insecureSkipVerify) SSL_set1_host(ssl, sniHost.c_str());
    if (SSL_connect(ssl) != 1) {
      unsigned long e = ERR_get_error();
      char ebuf[256];
      ERR_error_string_n(e, ebuf, sizeof(ebuf));
      *err = std::string("TLS handshake failed: ") + ebuf;
      return false;
    }
    return true;
  }

  ssize_t send(const char* data, size_t len) {
    return ssl ? SSL_write(ssl, data, (int)len) : write(fd, data, len);
  }
  ssize_t recv(char* data, size_t len) {
    return ssl ? SSL_read(ssl, data, (int)len) : read(fd, data, len);
  }
};

// Thread-local keep-alive pool: one cached plain-TCP/unix connection
// per target, giving the same connection reuse the reference's consul
// client inherits from Go's http.Transport. Plain + uncancellable
// requests only (TLS sessions and cancellable long-polls stay
// per-request). At thousands of TTL updates/sec, per-request connects
// burned measurable CPU on both the daemon and the agent.
struct ConnPool {
  std::map<std::string, int> conns;
  // close pooled fds at thread exit: consul workers are joined on
  // every generation teardown, so a leak here compounds per reload
  ~ConnPool() {
    for (auto& kv : conns) close(kv.second);
  }
};
thread_local ConnPool connPool;

int poolTake(const std::string& target) {
  auto it = connPool.conns.find(target);
  if (it == connPool.conns.end()) return -1;
  int fd = it->second;
  connPool.conns.erase(it);
  return fd;
}

void poolStore(const std::string& target, int fd) {
  int& slot = connPool.conns.emplace(target, -1).first->second;
  if (slot >= 0) close(slot);
  slot = fd;
}

// incremental chunked-body decoder: returns true once the terminal
// chunk is complete, filling *out with the decoded bytes
bool tryDechunk(const std::string& data, std::string* out) {
  out->clear();
  size_t pos = 0;
  while (true) {
    size_t eol = data.find("\r\n", pos);
    if (eol == std::string::npos) return false;
    long len = strtol(data.substr(pos, eol - pos).c_str(), nullptr, 16);
    if (len < 0) return false;
    if (len == 0) return true;  // terminal chunk (ignore trailers)
    if (data.size() < eol + 2 + (size_t)len + 2) return false;
    out->append(data, eol + 2, (size_t)len);
    pos = eol + 2 + (size_t)len + 2;
  }
}

// A pooled connection when allowed and available, else a fresh one;
// either way it carries this request's timeouts (a pooled fd still has
// the previous request's).
int acquireConn(const std::string& target, int timeoutMs, bool usePool,
                bool* fromPool, std::string* err) {
  int fd = usePool ? poolTake(target) : -1;
  *fromPool = fd >= 0;
  if (fd < 0) fd = connectTarget(target, err);
  if (fd >= 0) setIoTimeout(fd, timeoutMs);
  return fd;
}

std::string serialiseRequest(const std::string& method, const std::string& path,
                             const std::string& host, bool keepAlive,
                             const Headers& headers, const std::string& body,
                             const std::string& contentType) {
  std::string req = method + " " + path + " HTTP/1.1\r\n";
  req += "Host: " + host + "\r\n";
  req += keepAlive ? "Connection: keep-alive\r\n" : "Connection: close\r\n";
  for (auto& kv : headers) req += kv.first + ": " + kv.second + "\r\n";
  if (!body.empty() || method == "POST" || method == "PUT") {
    req += "Content-Type: " + contentType + "\r\n";
    req += "Content-Length: " + std::to_string(body.size()) + "\r\n";
  }
  req += "\r\n";
  req += body;
  return req;
}

bool writeAll(Transport& t, const std::string& data) {
  size_t off = 0;
  while (off < data.size()) {
    ssize_t n = t.send(data.data() + off, data.size() - off);
    if (n > 0)
      off += n;
    else if (!(n < 0 && errno == EINTR && !t.ssl))
      return false;
  }
  return true;
}

// false on EOF or error/timeout
bool readMore(Transport& t, std::string* resp) {
  char buf[8192];
  while (true) {
    ssize_t n = t.recv(buf, sizeof(buf));
    if (n > 0) {
      resp->append(buf, n);
      return true;
    }
    if (!(n < 0 && errno == EINTR && !t.ssl)) return false;
  }
}

enum class ReadResult { Ok, Empty, Malformed, Truncated, TooLarge };

// Read incrementally: the head first, then exactly the framed body.
// Fills status, headers and body; *bodyFramed is false when the body
// ran to EOF, which leaves the connection unusable.
ReadResult readResponse(Transport& t, ClientResult* result, bool* bodyFramed,
                        size_t maxBody) {
  std::string resp;
  size_t headerEnd;
  while ((headerEnd = resp.find("\r\n\r\n")) == std::string::npos) {
    if (!readMore(t, &resp)) break;
  }
  if (resp.empty()) return ReadResult::Empty;
  int status = parseStatus(resp);
  if (headerEnd == std::string::npos || status < 0)
    return ReadResult::Malformed;
  result->status = status;
  parseHeaderLines(resp, resp.find("\r\n") + 2, headerEnd, &result->headers);

  const size_t bodyStart = headerEnd + 4;
  *bodyFramed = true;
  if (isChunked(result->headers)) {
    // timeout/EOF mid-body: a truncated framed body is an error, not a
    // short success (Go's client errors the same way)
    std::string decoded;
    while (!tryDechunk(resp.substr(bodyStart), &decoded)) {
      if (maxBody && decoded.size() > maxBody) return ReadResult::TooLarge;
      if (!readMore(t, &resp)) return ReadResult::Truncated;
    }
    if (maxBody && decoded.size() > maxBody) return ReadResult::TooLarge;
    result->body = std::move(decoded);
  } else if (result->headers.count("content-length")) {
    size_t want = contentLength(result->headers);
    if (maxBody && want > maxBody) return ReadResult::TooLarge;
    while (resp.size() < bodyStart + want) {
      if (!readMore(t, &resp)) return ReadResult::Truncated;
    }
    result->body = resp.substr(bodyStart, want);
  } else {
    // no framing: read to EOF, connection not reusable
    while (readMore(t, &resp)) {
      if (maxBody && resp.size() - bodyStart > maxBody)
        return ReadResult::TooLarge;
    }
    result->body = resp.substr(bodyStart);
    *bodyFramed = false;
  }
  return ReadResult::Ok;
}

// reuse only when the server did not ask to close and sent a real status
bool serverKeepsAlive(const ClientResult& result) {
  auto it = result.headers.find("connection");
  bool closes = it != result.headers.end() &&
                toLower(it->second).find("close") != std::string::npos;
  return !closes && result.status > 0;
}

}  // namespace

ClientResult request(const std::string& target, const std::string& method,
                     const std::string& path, const std::string& body,
                     const std::string& contentType,
                     const std::map<std::string, std::string>& headers,
                     int timeoutMs, const TlsOptions* tls,
                     CancelToken* cancel, size_t maxBody) {
  ClientResult result;
  if (cancel && cancel->cancelled()) {
    result.error = "cancelled";
    return result;
  }
  const bool tlsOn = tls && tls->enabled;
  // pooling applies to plain, uncancellable requests only
  const bool reusable = !tlsOn && cancel == nullptr;
  const std::string host =
      target.rfind("unix:", 0) == 0 ? "localhost" : target;
  const std::string req = serialiseRequest(method, path, host, reusable,
                                           headers, body, contentType);

  // A pooled connection may have gone stale while idle, which shows as a
  // failed write or an empty read; only then is there a second attempt,
  // always on a fresh connection.
  for (int attempt = 0; attempt < 2; attempt++) {
    result = ClientResult{};
    Transport t;
    bool fromPool = false;
    t.fd = acquireConn(target, timeoutMs, reusable && attempt == 0, &fromPool,
                       &result.error);
    if (t.fd < 0) return result;
    struct Disarm {
      CancelToken* ct;
      ~Disarm() {
        if (ct) ct->disarm();
      }
    } disarm{cancel};
    if (cancel) cancel->arm(t.fd);
    if (tlsOn && !t.startTls(host, *tls, &result.error)) return result;

    if (!writeAll(t, req)) {
      if (fromPool) continue;  // retry case 1: stale keep-alive
      break;                   // "write failed"
    }
    bool bodyFramed = false;
    ReadResult rr = readResponse(t, &result, &bodyFramed, maxBody);
    if (rr == ReadResult::Empty && fromPool)
      continue;  // retry case 2: the server closed the idle connection
    if (rr == ReadResult::Empty || rr == ReadResult::Malformed) {
      result.error = (cancel && cancel->cancelled()) ? "cancelled"
                                                     : "malformed response";
      return result;
    }
    if (rr == ReadResult::Truncated) {
      result.error = "truncated response body";
      return result;
    }
    if (rr == ReadResult::TooLarge) {
      result.error = kBodyTooLarge;
      return result;
    }
    result.ok = true;
    if (reusable && bodyFramed && serverKeepsAlive(result)) {
      poolStore(target, t.fd);
      t.fd = -1;  // keep it out of Transport's destructor
    }
    return result;
  }
  result.error = "write failed";
  return result;
}

}  // namespace http
}  // namespace cpilot
