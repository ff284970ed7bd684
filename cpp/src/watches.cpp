#include "cpilot/watches.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <tuple>

#include "cpilot/decode.hpp"
#include "cpilot/ips.hpp"
#include "cpilot/log.hpp"

namespace cpilot {

namespace {

bool readWholeFile(const std::string& path, std::string* out) {
  std::ifstream f(path, std::ios::binary);
  if (!f) return false;
  std::stringstream ss;
  ss << f.rdbuf();
  if (f.bad()) return false;
  *out = ss.str();
  return true;
}

// watches[].render: shape only
bool newRenderConfig(const Json& raw, const std::string& watchName,
                     std::shared_ptr<RenderConfig>* out, std::string* err) {
  const std::string where = "watch[" + watchName + "].render";
  if (!raw.isObject()) {
    *err = where + " must be an object";
    return false;
  }
  if (!decode::checkKeys(raw, {"source", "dest", "mode"}, err)) {
    *err = where + ": " + *err;
    return false;
  }
  auto cfg = std::make_shared<RenderConfig>();
  struct {
    const char* key;
    std::string* field;
  } paths[] = {{"source", &cfg->source}, {"dest", &cfg->dest}};
  for (auto& p : paths) {
    const Json* v = raw.find(p.key);
    if (!v) {
      *err = where + "." + p.key + " is required";
      return false;
    }
    if (!v->isString() || v->str().empty()) {
      *err = where + "." + p.key + " must be a non-empty string";
      return false;
    }
    if (v->str()[0] != '/') {
      *err = where + "." + p.key + " must be an absolute path";
      return false;
    }
    *p.field = v->str();
  }
  if (cfg->source == cfg->dest) {
    *err = where + ".dest must differ from source";
    return false;
  }
  if (const Json* v = raw.find("mode")) {
    const std::string& m = v->str();
    bool octal = v->isString() && (m.size() == 3 || m.size() == 4) &&
                 m.find_first_not_of("01234567") == std::string::npos;
    long mode = octal ? strtol(m.c_str(), nullptr, 8) : -1;
    if (mode < 0 || mode > 0777) {
      *err = where + ".mode must be an octal string from \"0000\" to \"0777\"";
      return false;
    }
    cfg->mode = (mode_t)mode;
  }
  *out = std::move(cfg);
  return true;
}

}  // namespace

bool newWatchConfigs(const Json& rawWatches,
                     std::vector<std::shared_ptr<WatchConfig>>* out,
                     std::string* err) {
  out->clear();
  if (rawWatches.isNull()) return true;
  if (!rawWatches.isArray()) {
    *err = "Watch configuration error: watches must be an array";
    return false;
  }
  for (auto& raw : rawWatches.array()) {
    if (!raw.isObject()) {
      *err = "Watch configuration error: watch must be an object";
      return false;
    }
    if (!decode::checkKeys(
            raw,
            {"name", "interval", "tag", "dc", "blocking", "render", "key",
             "keyPrefix"},
            err)) {
      *err = "Watch configuration error: " + *err;
      return false;
    }
    auto cfg = std::make_shared<WatchConfig>();
    if (const Json* v = raw.find("name")) decode::toString(*v, &cfg->name);
    if (const Json* v = raw.find("interval")) decode::toInt(*v, &cfg->poll);
    if (const Json* v = raw.find("tag")) decode::toString(*v, &cfg->tag);
    if (const Json* v = raw.find("dc")) decode::toString(*v, &cfg->dc);
    if (const Json* v = raw.find("blocking")) {
      if (!decode::toBool(*v, &cfg->blocking)) {
        *err = "watch[" + cfg->name + "].blocking must be a bool";
        return false;
      }
    }

    if (!validateServiceName(cfg->name, err)) return false;
    cfg->serviceName = cfg->name;
    cfg->name = "watch." + cfg->name;  // watches/config.go:44-45
    // a key watch: `key` or `keyPrefix`, null counting as not given
    const Json* key = decode::given(raw, "key");
    const Json* keyPrefix = decode::given(raw, "keyPrefix");
    if (key && keyPrefix) {
      *err = "watch[" + cfg->serviceName +
             "]: key and keyPrefix are mutually exclusive";
      return false;
    }
    if (key || keyPrefix) {
      const char* field = key ? "key" : "keyPrefix";
      std::string why;
      if (!validateKVKey(key ? *key : *keyPrefix, &cfg->key, &why)) {
        *err = "watch[" + cfg->serviceName + "]." + field + " " + why;
        return false;
      }
      if (decode::given(raw, "tag")) {
        *err = "watch[" + cfg->serviceName +
               "].tag does not apply to a key watch";
        return false;
      }
      cfg->isKey = true;
      cfg->keyPrefix = keyPrefix != nullptr;
    }
    if (cfg->poll < 1) {
      *err = "watch[" + cfg->serviceName + "].interval must be > 0";
      return false;
    }
    if (const Json* v = raw.find("render")) {
      if (!v->isNull() &&
          !newRenderConfig(*v, cfg->serviceName, &cfg->render, err))
        return false;
    }
    out->push_back(cfg);
  }
  // a key watch's name is its cache key and its only identity: it must be
  // the only watch of that name. Service watches keep what they did.
  for (auto& a : *out) {
    if (!a->isKey) continue;
    for (auto& b : *out) {
      if (a != b && a->name == b->name) {
        *err = "watch[" + a->serviceName +
               "]: a key watch must not share its name with another watch";
        return false;
      }
    }
  }
  return true;
}

bool loadRenderTemplate(WatchConfig& cfg, std::string* err) {
  if (!cfg.render) return true;
  const std::string where = "watch[" + cfg.serviceName + "].render.source: ";
  std::string text;
  errno = 0;
  if (!readWholeFile(cfg.render->source, &text)) {
    *err = where + "open " + cfg.render->source + ": " +
           strerror(errno ? errno : EIO);
    return false;
  }
  try {
    cfg.render->tmpl = Template::parse(text);
  } catch (const std::exception& e) {
    *err = where + e.what();
    return false;
  }
  return true;
}

Json buildRenderData(const std::string& serviceName, const std::string& tag,
                     const std::string& dc,
                     const std::vector<ServiceEntry>& entries) {
  struct Row {
    std::string address;
    const ServiceEntry* e;
  };
  std::vector<Row> rows;
  for (auto& e : entries)
    rows.push_back({e.address.empty() ? e.nodeAddress : e.address, &e});
  std::sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) {
    return std::tie(a.address, a.e->port, a.e->id) <
           std::tie(b.address, b.e->port, b.e->id);
  });
  JsonArray services;
  for (auto& r : rows) {
    JsonArray tags;
    for (auto& t : r.e->tags) tags.push_back(Json(t));
    services.push_back(Json(JsonObject{
        {"ID", Json(r.e->id)},
        {"Name", Json(serviceName)},
        {"Address", Json(r.address)},
        {"Port", Json(r.e->port)},
        {"Tags", Json(std::move(tags))},
        {"Node", Json(r.e->node)},
        {"NodeAddress", Json(r.e->nodeAddress)},
    }));
  }
  return Json(JsonObject{
      {"Name", Json(serviceName)},
      {"Tag", Json(tag)},
      {"DC", Json(dc)},
      {"Healthy", Json(!entries.empty())},
      {"Services", Json(std::move(services))},
  });
}

bool writeFileAtomic(const std::string& dest, const std::string& bytes,
                     mode_t mode, std::string* err) {
  std::string current;
  if (readWholeFile(dest, &current) && current == bytes) return true;

  std::string tmp = dest + ".tmp.XXXXXX";
  int fd = mkostemp(&tmp[0], O_CLOEXEC);
  if (fd < 0) {
    *err = "create " + tmp + ": " + strerror(errno);
    return false;
  }
  auto fail = [&](const char* what) {
    *err = std::string(what) + " " + tmp + ": " + strerror(errno);
    if (fd >= 0) close(fd);
    unlink(tmp.c_str());
    return false;
  };
  // mkostemp creates 0600; fchmod sets the mode whatever the umask is
  if (fchmod(fd, mode) != 0) return fail("chmod");
  size_t off = 0;
  while (off < bytes.size()) {
    ssize_t n = write(fd, bytes.data() + off, bytes.size() - off);
    if (n < 0) {
      if (errno == EINTR) continue;
      return fail("write");
    }
    off += (size_t)n;
  }
  int rc = close(fd);
  fd = -1;
  if (rc != 0) return fail("close");
  if (rename(tmp.c_str(), dest.c_str()) != 0) return fail("rename");
  return true;
}

void Watch::run(Loop& loop, std::shared_ptr<Bus> bus, ConsulBackend* consul) {
  loop_ = &loop;
  bus_ = std::move(bus);
  consul_ = consul;
  auto self = shared_from_this();
  if (blocking_) {
    issueBlocking();
    return;
  }
  timer_ = loop.addInterval(std::chrono::seconds(poll_),
                            [this, self] { tick(); });
}

void Watch::stop(Loop& loop) {
  stopped_ = true;
  if (timer_) {
    loop.cancelTimer(timer_);
    timer_ = 0;
  }
}

void Watch::onResult(bool ok, std::vector<ServiceEntry> entries) {
  if (!ok) {
    LOG_WARN("failed to query %s", serviceName_.c_str());
    return;
  }
  consul_->watchGauge()->set({serviceName_}, (double)entries.size());
  bool isHealthy = !entries.empty();
  bool didChange = consul_->compareAndSwap(serviceName_, entries);
  publishResult(didChange, isHealthy, [&] {
    return buildRenderData(serviceName_, tag_, dc_, entries);
  });
}

void Watch::onKVResult(bool ok, std::vector<KVEntry> entries) {
  if (!ok) {
    LOG_WARN("failed to query key %s", key_.c_str());
    return;
  }
  // healthy: the key exists, or something lies under the prefix
  bool isHealthy = !entries.empty();
  bool didChange = consul_->compareAndSwapKV(serviceName_, entries);
  publishResult(didChange, isHealthy, [&] {
    return buildKVRenderData(serviceName_, key_, keyPrefix_, dc_, entries);
  });
}

void Watch::publishResult(bool didChange, bool isHealthy,
                          const std::function<Json()>& renderData) {
  // the file is in place before anything hears about this result; the
  // first result of a generation renders even when nothing changed, so
  // dest exists before anything depends on it
  if (render_ && (didChange || !rendered_)) {
    rendered_ = true;
    std::string err;
    if (!renderDest(renderData(), &err)) {
      LOG_ERROR("%s: render: %s", name_.c_str(), err.c_str());
      bus_->publish(Event{EventCode::Error, name_ + ": render: " + err});
    }
  }
  if (didChange) {
    bus_->publish(Event{EventCode::StatusChanged, name_});
    if (isHealthy)
      bus_->publish(Event{EventCode::StatusHealthy, name_});
    else
      bus_->publish(Event{EventCode::StatusUnhealthy, name_});
  }
}

bool Watch::renderDest(const Json& data, std::string* err) {
  std::string out;
  try {
    out = render_->tmpl.render(data);
  } catch (const std::exception& e) {
    *err = e.what();
    return false;
  }
  return writeFileAtomic(render_->dest, out, render_->mode, err);
}

void Watch::tick() {
  if (stopped_ || !consul_) return;
  if (inFlight_) return;  // one query at a time; skip this tick
  inFlight_ = true;
  auto self = shared_from_this();
  if (isKey_) {
    consul_->kvGet(key_, keyPrefix_, dc_,
                   [this, self](bool ok, std::vector<KVEntry> entries) {
                     inFlight_ = false;
                     if (stopped_) return;
                     onKVResult(ok, std::move(entries));
                   });
    return;
  }
  consul_->healthService(
      serviceName_, tag_, dc_,
      [this, self](bool ok, std::vector<ServiceEntry> entries) {
        inFlight_ = false;
        if (stopped_) return;
        onResult(ok, std::move(entries));
      });
}

void Watch::issueBlocking() {
  if (stopped_ || !consul_) return;
  auto self = shared_from_this();
  if (isKey_) {
    consul_->kvGetBlocking(
        key_, keyPrefix_, dc_, lastIndex_, 10,
        [this, self](bool ok, std::vector<KVEntry> entries, uint64_t index) {
          if (stopped_) return;
          onKVResult(ok, std::move(entries));
          afterBlocking(ok, index);
        });
    return;
  }
  consul_->healthServiceBlocking(
      serviceName_, tag_, dc_, lastIndex_, 10,
      [this, self](bool ok, std::vector<ServiceEntry> entries,
                   uint64_t index) {
        if (stopped_) return;
        onResult(ok, std::move(entries));
        afterBlocking(ok, index);
      });
}

void Watch::afterBlocking(bool ok, uint64_t index) {
  auto self = shared_from_this();
  if (ok) {
    // consul index contract: reset when it goes backwards
    lastIndex_ = (index > 0 && index >= lastIndex_) ? index : 0;
    // immediate re-issue with a tiny floor so a hot agent can't
    // spin us
    timer_ = loop_->addTimeout(std::chrono::milliseconds(50),
                               [this, self] { issueBlocking(); });
  } else {
    // error backoff: fall back to the configured interval
    timer_ = loop_->addTimeout(std::chrono::seconds(poll_),
                               [this, self] { issueBlocking(); });
  }
}

}  // namespace cpilot
