#include "cpilot/control.hpp"

#include <unistd.h>

#include <cstdio>
#include <thread>

#include "cpilot/command.hpp"
#include "cpilot/decode.hpp"
#include "cpilot/log.hpp"
#include "cpilot/signals.hpp"

namespace cpilot {

const char* kDefaultControlSocket = "/var/run/containerpilot.socket";

bool newControlConfig(const Json* raw, ControlConfig* out, std::string* err) {
  out->socketPath = kDefaultControlSocket;
  if (raw == nullptr || raw->isNull()) return true;
  if (!raw->isObject()) {
    *err = "control config parsing error: must be an object";
    return false;
  }
  if (!decode::checkKeys(*raw, {"socket"}, err)) {
    *err = "control config parsing error: " + *err;
    return false;
  }
  if (const Json* v = raw->find("socket")) decode::toString(*v, &out->socketPath);
  return true;
}

ControlServer::ControlServer(Loop& loop, std::string socketPath)
    : loop_(loop), socketPath_(std::move(socketPath)) {
  requestCounter_ = prom::Registry::global().registerFamily(
      "containerpilot_control_http_requests",
      "count of requests to control socket, partitioned by path and HTTP code",
      prom::MetricType::Counter, {"code", "path"});
}

ControlServer::~ControlServer() { stop(); }

bool ControlServer::start(std::shared_ptr<Bus> bus, std::string* err) {
  bus_ = std::move(bus);
  if (socketPath_.empty()) {
    *err = "control: validate failed with control server not loading due to "
           "missing config";
    return false;
  }
  // unlink stale socket (control/control.go:61-73)
  if (access(socketPath_.c_str(), F_OK) == 0) {
    LOG_DEBUG("control: unlinking previous socket at %s", socketPath_.c_str());
    if (unlink(socketPath_.c_str()) != 0) {
      *err = "could not remove stale socket";
      return false;
    }
  }
  server_ = std::make_unique<http::Server>(
      loop_, [this](const http::Request& req) { return handle(req); });
  // a contended socket is retried by the server on the reactor
  server_->listenRetrying(
      [this](std::string* e) { return server_->listenUnix(socketPath_, e); },
      "control", socketPath_, [this] {
        LOG_DEBUG("control: listening to %s", socketPath_.c_str());
        LOG_INFO("control: serving at %s", socketPath_.c_str());
      });
  return true;
}

void ControlServer::stop() {
  if (server_) {
    server_->stop();
    server_.reset();
    unlink(socketPath_.c_str());
    LOG_DEBUG("control: completed graceful shutdown of control server");
  }
}

namespace {

http::Response plainResponse(int status) {
  http::Response resp;
  resp.status = status;
  if (status == 200) {
    resp.body = "\n";  // io.WriteString(w, "\n") on empty 200
  } else {
    resp.body = std::string(http::statusText(status)) + "\n";  // http.Error
  }
  return resp;
}

}  // namespace

std::string metricValueString(const Json& v) {
  if (v.isString()) return v.str();
  if (v.isBool()) return v.boolean() ? "true" : "false";
  if (v.isInt()) return std::to_string(v.asInt());
  if (v.isDouble()) return prom::formatValue(v.asDouble());
  return v.dump();
}

http::Response ControlServer::handle(const http::Request& req) {
  http::Response resp;
  const std::string& path = req.path;

  if (path == "/v3/ping") {
    // GetPing has no method check (endpoints.go:133-138)
    resp = plainResponse(200);
    requestCounter_->inc({"200", path});
    return resp;
  }

  auto finish = [&](int status) {
    requestCounter_->inc({std::to_string(status), path});
    return plainResponse(status);
  };

  if (path != "/v3/environ" && path != "/v3/reload" && path != "/v3/metric" &&
      path != "/v3/signal" && path != "/v3/maintenance/enable" &&
      path != "/v3/maintenance/disable") {
    http::Response notFound;
    notFound.status = 404;
    notFound.body = "404 page not found\n";
    requestCounter_->inc({"404", path});
    return notFound;
  }
  if (req.method != "POST") return finish(405);

  if (path == "/v3/environ") {
    // PutEnviron (endpoints.go:57-72)
    try {
      Json doc = parseJson5(req.body);
      if (!doc.isObject()) return finish(422);
      for (auto& kv : doc.object()) {
        if (!kv.second.isString()) return finish(422);
        setenv(kv.first.c_str(), kv.second.str().c_str(), 1);
      }
      commandEnvInvalidate();  // future spawns see the new environ
    } catch (const std::exception&) {
      return finish(422);
    }
    return finish(200);
  }
  if (path == "/v3/reload") {
    LOG_DEBUG("control: reloading app via control plane");
    bus_->setReloadFlag();
    bus_->shutdown();
    LOG_DEBUG("control: reloaded app via control plane");
    return finish(200);
  }
  if (path == "/v3/metric") {
    // PostMetric (endpoints.go:111-129)
    try {
      Json doc = parseJson5(req.body);
      if (!doc.isObject()) return finish(422);
      for (auto& kv : doc.object()) {
        std::string eventVal = kv.first + "|" + metricValueString(kv.second);
        bus_->publish(Event{EventCode::Metric, eventVal});
      }
    } catch (const std::exception&) {
      return finish(422);
    }
    return finish(200);
  }
  if (path == "/v3/signal") return finish(postSignal(req.body));
  if (path == "/v3/maintenance/enable") {
    bus_->publish(GlobalEnterMaintenance);
    return finish(200);
  }
  if (path == "/v3/maintenance/disable") {
    bus_->publish(GlobalExitMaintenance);
    return finish(200);
  }
  return finish(404);
}

// PostSignal (extension): {"<job>": "<signal>", ...}. Everything is
// validated before anything is sent, so a 422 means no process was
// signalled; then every entry is delivered in order, to the process and
// not its group, and a target without a running process makes it a 409.
int ControlServer::postSignal(const std::string& body) {
  struct Target {
    std::string job, sigName;
    CommandPtr exec;
    int signo = 0;
  };
  std::vector<Target> targets;
  try {
    Json doc = parseJson5(body);
    if (!doc.isObject()) return 422;
    for (auto& kv : doc.object()) {
      Target t;
      t.job = kv.first;
      if (!kv.second.isString() ||
          !signals::fromName(kv.second.str(), &t.signo, &t.sigName))
        return 422;
      if (!jobLookup_ || !jobLookup_(t.job, &t.exec) || !t.exec) return 422;
      targets.push_back(std::move(t));
    }
  } catch (const std::exception&) {
    return 422;
  }
  int status = 200;
  for (auto& t : targets) {
    pid_t pid = t.exec->pid();
    std::string reason;
    if (signals::deliver(pid, t.signo, /*group=*/false, &reason)) {
      LOG_INFO("control: sent %s to job %s at pid %d", t.sigName.c_str(),
               t.job.c_str(), (int)pid);
    } else {
      LOG_WARN("control: %s not sent to job %s: %s", t.sigName.c_str(),
               t.job.c_str(), reason.c_str());
      status = 409;
    }
  }
  return status;
}

}  // namespace cpilot
