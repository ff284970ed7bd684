// Native health probes: `health.tcp` and `health.http` run on the reactor
// itself — a non-blocking connect (plus, for http, one request and a
// status-line parse) driven by the loop's fd watchers and timer heap.
// No child process, no spawn-helper round trip, no log pipe, no PID
// overlay entry.
//
// A probe publishes the same verdict events an exec check does
// (ExitSuccess / ExitFailed + Error, source `check.<job>`), so Job,
// `when:` sources and the events counter need no new cases.
//
// The same engine runs http jobs (`jobs[].http`): a request that may carry
// a body, published from source `<job>`, which reads the response out
// instead of resetting the connection at the status line.
#pragma once

#include <sys/socket.h>

#include <memory>
#include <string>
#include <vector>

#include "cpilot/events.hpp"
#include "cpilot/json.hpp"
#include "cpilot/loop.hpp"
#include "cpilot/timing.hpp"

namespace cpilot {
// A namespace of its own: the native unit-test binary declares a global
// `Probe` event recorder next to `using namespace cpilot`, and it
// includes jobs.hpp, so the class cannot live in cpilot directly.
namespace health {

// Stable failure reasons (documented in docs/30-configuration.md).
// "malformed response"
extern const char* const kProbeMalformed;
// "connection closed before response"
extern const char* const kProbeClosedEarly;

// Response bytes accepted while looking for the status line's CRLF.
constexpr size_t kProbeMaxStatusLine = 8192;
// Longest `body` an http job may send.
constexpr size_t kActionMaxBody = 65536;
// Response bytes an http job reads and discards before it stops waiting
// for the peer to finish.
constexpr size_t kActionMaxDrain = 1024 * 1024;
// Response head an http job buffers while looking for a Content-Length.
constexpr size_t kActionMaxHead = 64 * 1024;

struct ProbeSpec {
  enum class Kind { Tcp, Http };
  Kind kind = Kind::Tcp;

  // resolved at validation: IP literals and `localhost` only, names are
  // never resolved on the reactor
  struct sockaddr_storage addr {};
  socklen_t addrLen = 0;
  std::string target;  // "host:port" as configured, for log lines

  // http only
  std::string method = "GET";
  std::string hostHeader;  // authority exactly as written in the URL
  std::string path = "/";  // path + query
  std::vector<std::pair<std::string, std::string>> headers;
  std::vector<int> expect;  // empty = any 2xx

  // http jobs only: the request is the job's action, not a check. It may
  // carry a body, it is logged as an action, and the response is read out
  // and discarded instead of reset at the status line.
  bool action = false;
  std::string url;  // as configured, for log lines
  bool hasBody = false;
  std::string body;

  Duration timeout{0};
};

// Parse `health.tcp` ("HOST:PORT"). On error returns false and sets err
// (without the job[...] prefix; the caller adds it).
bool parseTcpProbe(const std::string& hostPort, ProbeSpec* out,
                   std::string* err);

// Parse `health.http`: a URL string or {url, method, headers, expect}.
// errKey receives the sub-key the error is about ("", ".url", ".method",
// ".headers", ".expect") so the caller can name it.
bool parseHttpProbe(const Json& raw, ProbeSpec* out, std::string* errKey,
                    std::string* err);

// Parse `jobs[].http`: a URL string or {url, method, headers, expect,
// body}. The rules of `health.http` plus the methods that change state, a
// body for them, and a refusal of the headers the daemon sets itself.
bool parseHttpAction(const Json& raw, ProbeSpec* out, std::string* errKey,
                     std::string* err);

// The exact request bytes an http probe or an http job writes.
std::string buildProbeRequest(const ProbeSpec& spec);

// "1s", "250ms", "1500ms", "10us", "7ns": the largest unit that divides
// the duration exactly.
std::string probeDurationString(Duration d);

class Probe : public std::enable_shared_from_this<Probe> {
 public:
  Probe(ProbeSpec spec, std::string name);
  ~Probe();
  Probe(const Probe&) = delete;
  Probe& operator=(const Probe&) = delete;

  const std::string& name() const { return name_; }
  const ProbeSpec& spec() const { return spec_; }

  // Start one probe run (loop thread only). Publishes exactly one
  // verdict on `bus` unless cancel() intervenes. If the previous run is
  // still in flight the tick is skipped, not queued. The bus is held by
  // shared_ptr for the duration of the run so a probe from a drained
  // config generation can only publish to that generation's bus.
  void run(Loop& loop, std::shared_ptr<Bus> bus);

  // Abandon an in-flight run: unwatch, close, cancel the timer, publish
  // nothing.
  void cancel();

  bool running() const { return state_ != State::Idle; }

 private:
  enum class State { Idle, Connecting, Sending, Reading, Draining };

  void onIo(uint32_t events);
  void onConnected();
  void onWritable();
  void onReadable();
  void onTimeout();
  void judgeStatusLine(size_t crlf);
  // actions: hold the verdict and read the response out
  void beginDrain(size_t crlf);
  void onDrainReadable();
  bool drainComplete();
  void finishDrain(bool peerClosed);
  // release the socket and the timer; returns the bus of this run. The
  // close is abortive unless `orderly`.
  std::shared_ptr<Bus> teardown(bool orderly = false);
  void pass();
  void fail(const std::string& reason, bool timedOut = false);
  void failErrno(int err);

  ProbeSpec spec_;
  std::string name_;
  std::string request_;

  State state_ = State::Idle;
  Loop* loop_ = nullptr;
  std::shared_ptr<Bus> bus_;
  int fd_ = -1;
  uint64_t timer_ = 0;
  size_t sent_ = 0;
  std::string rbuf_;

  // the verdict of the status line, held while an action drains
  int code_ = 0;
  std::string verdict_;  // empty = passed
  size_t drained_ = 0;   // response bytes read so far
  bool headDone_ = false;
  bool bodyKnown_ = false;  // the head announced a length
  size_t bodyEnd_ = 0;      // drained_ at which that length has arrived
};

using ProbePtr = std::shared_ptr<Probe>;

}  // namespace health
}  // namespace cpilot
