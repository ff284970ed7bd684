// Control plane: HTTP server over a unix domain socket with the reference's
// five POST endpoints + GET ping, implementing the code's actual behavior
// (empty 200 body "\n", 422 on bad input, 405 on wrong method), plus
// POST /v3/signal (extension: signal a supervised job's process).
// Parity: /root/reference/control/{control,config,endpoints}.go.
#pragma once

#include <functional>
#include <memory>
#include <string>

#include "cpilot/command.hpp"
#include "cpilot/events.hpp"
#include "cpilot/http.hpp"
#include "cpilot/json.hpp"
#include "cpilot/metrics.hpp"

namespace cpilot {

extern const char* kDefaultControlSocket;  // /var/run/containerpilot.socket

struct ControlConfig {
  std::string socketPath = "/var/run/containerpilot.socket";
};

bool newControlConfig(const Json* raw, ControlConfig* out, std::string* err);

// The value text POST /v3/metric puts after "name|" for one JSON value
// (Go's fmt %v of the unmarshaled interface{}, endpoints.go:124-127): a
// number is spelled so that Metric::record reads back every bit of it.
std::string metricValueString(const Json& v);

class ControlServer {
 public:
  // reloadCb: invoked by POST /v3/reload after setting the bus reload flag
  ControlServer(Loop& loop, std::string socketPath);
  ~ControlServer();

  // Unlink stale socket (control/control.go:61-73), then bind through
  // http::Server::listenUnixRetrying, which owns the 10x1s retry on a
  // loop timer and the fatal exit after the last failed attempt. Returns
  // false only for unretryable config errors (missing path, unremovable
  // stale socket).
  bool start(std::shared_ptr<Bus> bus, std::string* err);
  void stop();  // also unlinks the socket

  const std::string& socketPath() const { return socketPath_; }

  // POST /v3/signal resolves job names through this callback, which the
  // App answers from the current generation's jobs. Returns false for an
  // unknown job; *exec stays null for a job without an `exec`.
  using JobLookup =
      std::function<bool(const std::string& job, CommandPtr* exec)>;
  void setJobLookup(JobLookup lookup) { jobLookup_ = std::move(lookup); }

 private:
  int postSignal(const std::string& body);

  http::Response handle(const http::Request& req);

  Loop& loop_;
  std::string socketPath_;
  std::shared_ptr<Bus> bus_;
  std::unique_ptr<http::Server> server_;
  std::shared_ptr<prom::Family> requestCounter_;
  JobLookup jobLookup_;
};

}  // namespace cpilot
