// Watches: poll Consul for healthy instances of a service every `interval`
// seconds; on membership/address change publish StatusChanged plus
// StatusHealthy/StatusUnhealthy from source "watch.<name>".
// Parity: /root/reference/watches/{watches,config}.go.
// extension: a watch with `key` or `keyPrefix` watches Consul's key/value
// store instead (cpilot/kv.hpp); events, render and scheduling are shared.
#pragma once

#include <sys/types.h>

#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "cpilot/discovery.hpp"
#include "cpilot/events.hpp"
#include "cpilot/json.hpp"
#include "cpilot/tmpl.hpp"

namespace cpilot {

// extension: `render` writes the watch's healthy set through a template
// file into `dest` before the change events are published, so an onChange
// job always finds the file for the set its event is about.
struct RenderConfig {
  std::string source;  // template file, absolute
  std::string dest;    // output file, absolute
  mode_t mode = 0644;
  Template tmpl;       // parsed by loadRenderTemplate, not by the decoder
};

struct WatchConfig {
  std::string name;         // "watch.<service>"
  std::string serviceName;  // original name
  int poll = 0;             // seconds
  std::string tag;
  std::string dc;
  // extension: blocking=true uses Consul blocking queries (long-poll on
  // the service's index) — changes propagate in milliseconds instead of
  // the poll interval, and idle traffic drops to one request per wait
  // window. `interval` becomes the error-backoff period.
  bool blocking = false;
  std::shared_ptr<RenderConfig> render;  // null when not configured
  // extension: a key watch. `key` holds watches[].key or, with keyPrefix
  // set, watches[].keyPrefix; serviceName is then only the event source.
  bool isKey = false;
  bool keyPrefix = false;
  std::string key;
};

// Decodes and validates shape only; never touches the filesystem.
bool newWatchConfigs(const Json& rawWatches,
                     std::vector<std::shared_ptr<WatchConfig>>* out,
                     std::string* err);

// Read and parse cfg.render->source (no-op without render). On failure
// sets err to "watch[<name>].render.source: <reason>".
bool loadRenderTemplate(WatchConfig& cfg, std::string* err);

// What a render template sees as ".": Name/Tag/DC as configured, Healthy,
// and Services sorted by (Address, Port, ID). An empty Service.Address
// falls back to Node.Address.
Json buildRenderData(const std::string& serviceName, const std::string& tag,
                     const std::string& dc,
                     const std::vector<ServiceEntry>& entries);

// Make `dest` hold exactly `bytes`: untouched when it already does, else
// a temporary file in dest's directory with `mode`, renamed over dest.
// No fsync. On failure returns false, removes the temporary file and
// leaves dest as it was.
bool writeFileAtomic(const std::string& dest, const std::string& bytes,
                     mode_t mode, std::string* err);

class Watch : public std::enable_shared_from_this<Watch> {
 public:
  explicit Watch(const std::shared_ptr<WatchConfig>& cfg)
      : name_(cfg->name),
        serviceName_(cfg->serviceName),
        tag_(cfg->tag),
        dc_(cfg->dc),
        poll_(cfg->poll),
        blocking_(cfg->blocking),
        render_(cfg->render),
        isKey_(cfg->isKey),
        keyPrefix_(cfg->keyPrefix),
        key_(cfg->key) {}

  const std::string& name() const { return name_; }
  const std::string& serviceName() const { return serviceName_; }

  void run(Loop& loop, std::shared_ptr<Bus> bus, ConsulBackend* consul);
  void stop(Loop& loop);

 private:
  void tick();
  void issueBlocking();
  void afterBlocking(bool ok, uint64_t index);
  void onResult(bool ok, std::vector<ServiceEntry> entries);
  void onKVResult(bool ok, std::vector<KVEntry> entries);
  // the part both kinds of watch share: render, then the events
  void publishResult(bool didChange, bool isHealthy,
                     const std::function<Json()>& renderData);
  bool renderDest(const Json& data, std::string* err);

  std::string name_, serviceName_, tag_, dc_;
  int poll_;
  bool blocking_ = false;
  std::shared_ptr<RenderConfig> render_;
  bool isKey_ = false;
  bool keyPrefix_ = false;
  std::string key_;
  bool rendered_ = false;  // first successful result seen this generation
  uint64_t lastIndex_ = 0;
  Loop* loop_ = nullptr;
  std::shared_ptr<Bus> bus_;
  ConsulBackend* consul_ = nullptr;
  uint64_t timer_ = 0;
  bool inFlight_ = false;
  bool stopped_ = false;
};

}  // namespace cpilot
