// Minimal HTTP/1.1: a nonblocking server that runs on the reactor
// (serves the unix-socket control plane and the TCP telemetry endpoint)
// and a small blocking client (Consul API calls from worker threads, and
// the control-socket client used by subcommands).
// Connections are close-after-response; the reference also disables
// keep-alives (control/control.go:110).
#pragma once

#include <sys/socket.h>

#include <functional>
#include <map>
#include <mutex>
#include <memory>
#include <string>

#include "cpilot/loop.hpp"

namespace cpilot {
namespace http {

struct Request {
  std::string method;
  std::string path;
  std::string query;
  std::map<std::string, std::string> headers;  // lower-cased keys
  std::string body;
};

struct Response {
  int status = 200;
  std::string contentType = "text/plain; charset=utf-8";
  std::string body;
};

const char* statusText(int code);

using Handler = std::function<Response(const Request&)>;
using Headers = std::map<std::string, std::string>;

// ---- message-head parsing: pure functions shared by server and client ----

// Header lines of head[pos, end), where `end` is the offset of the
// CRLFCRLF that closes the head. Keys are lower-cased, only leading
// spaces are stripped from values, a repeated key keeps the last value
// and a line without ':' is skipped.
void parseHeaderLines(const std::string& head, size_t pos, size_t end,
                      Headers* out);
// "METHOD target VERSION": the target lies between the first and the last
// space and splits at the first '?'. False with fewer than two spaces.
bool parseRequestLine(const std::string& line, Request* req);
// Request line plus header lines; `headerEnd` is the offset just past
// the closing CRLFCRLF.
bool parseRequestHead(const std::string& buf, size_t headerEnd, Request* req);
// The integer after the first space of a response that starts with
// "HTTP/" (0 when it is not a number); -1 for anything else.
int parseStatus(const std::string& resp);
// 0 when absent or non-numeric; a negative value wraps to a huge size.
size_t contentLength(const Headers& headers);
// Transfer-Encoding contains "chunked" in any letter case.
bool isChunked(const Headers& headers);

class Server {
 public:
  Server(Loop& loop, Handler handler);
  ~Server();

  // Bind + listen on a unix socket path (unlinks nothing; caller manages
  // stale sockets) or a TCP port. Return false on bind/listen failure,
  // which includes a path too long for sockaddr_un.
  bool listenUnix(const std::string& path, std::string* err);
  bool listenTcp(const std::string& ip, int port, std::string* err);

  // Run `listen` (listenUnix or listenTcp bound to its address) now and,
  // while it fails, once a second on a loop timer, never by sleeping on
  // the reactor; the tenth failed attempt is fatal like the reference's
  // log.Fatal (control/control.go:125-140, telemetry/telemetry.go:77-91).
  // onBound runs once the listener is up. `name` prefixes the retry
  // warning, `addr` is the address as logged, and `attempt` is advanced
  // by the timer. Return whether this attempt bound.
  using ListenFn = std::function<bool(std::string* err)>;
  bool listenRetrying(ListenFn listen, const std::string& name,
                      const std::string& addr, std::function<void()> onBound,
                      int attempt = 1);

  void stop();  // close listener and all connections, drop a pending retry

 private:
  struct Conn;
  bool bindAndListen(int fd, const struct sockaddr* addr, socklen_t len,
                     std::string* err);
  void acceptReady();
  void armDeadline(const std::shared_ptr<Conn>& c);
  void connReadable(std::shared_ptr<Conn> c);
  void connWritable(std::shared_ptr<Conn> c);
  void beginWrite(const std::shared_ptr<Conn>& c, const Response& resp);
  void closeConn(const std::shared_ptr<Conn>& c);
  static Response errorResponse(int status);

  Loop& loop_;
  Handler handler_;
  int listenFd_ = -1;
  uint64_t retryTimer_ = 0;
  std::map<int, std::shared_ptr<Conn>> conns_;
};

// ---- blocking client ----

struct ClientResult {
  bool ok = false;
  int status = 0;
  std::string body;
  std::string error;
  Headers headers;  // lower-cased keys
};

// Cancellation for long-polling requests (Consul blocking queries):
// cancel() shuts the socket down from another thread so the blocked
// read returns immediately.
class CancelToken {
 public:
  void arm(int fd);     // called by request() once connected
  void disarm();        // called by request() before closing
  void cancel();        // any thread
  bool cancelled();

 private:
  std::mutex mu_;
  int fd_ = -1;
  bool cancelled_ = false;
};

// TLS options for https targets (OpenSSL; reference parity with the
// consul api.TLSConfig fields, discovery/config.go:29-61)
struct TlsOptions {
  bool enabled = false;
  std::string caFile;
  std::string caPath;
  std::string certFile;
  std::string keyFile;
  std::string serverName;          // SNI + hostname verification override
  bool insecureSkipVerify = false;
};

// ClientResult::error of a response whose body exceeds `maxBody`.
extern const char* const kBodyTooLarge;

// target: "unix:<path>" or "host:port". A unix path too long for
// sockaddr_un is an error, never truncated. maxBody > 0 caps the decoded
// body; a larger one fails with kBodyTooLarge instead of being buffered.
ClientResult request(const std::string& target, const std::string& method,
                     const std::string& path, const std::string& body,
                     const std::string& contentType = "application/json",
                     const std::map<std::string, std::string>& headers = {},
                     int timeoutMs = 10000,
                     const TlsOptions* tls = nullptr,
                     CancelToken* cancel = nullptr, size_t maxBody = 0);

}  // namespace http
}  // namespace cpilot
