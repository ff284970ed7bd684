// Native telemetry sensors: `telemetry.sensors` samples a file or an HTTP
// endpoint on an interval, extracts numbers with line / field / JSON
// pointer selectors and publishes them as Metric events, the same events
// `-putmetric` produces. No shell, no second containerpilot process, no
// control-socket round trip per sample.
//
// Reads never run on the reactor: a small worker pool owned by the
// telemetry generation does the blocking work and posts the body back
// with Loop::postIfLive. Extraction, counter deltas and publishing happen
// on the loop thread.
#pragma once

#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "cpilot/events.hpp"
#include "cpilot/http.hpp"
#include "cpilot/json.hpp"
#include "cpilot/loop.hpp"
#include "cpilot/metrics.hpp"
#include "cpilot/probe.hpp"
#include "cpilot/timing.hpp"

namespace cpilot {
namespace sensor {

// A source larger than this fails the sample with "source too large".
constexpr size_t kMaxSourceBytes = 1 << 20;
// Worker threads per telemetry generation.
constexpr size_t kMaxWorkers = 4;
// Bytes of an offending token quoted in a "not a number" reason.
constexpr size_t kMaxQuotedToken = 64;

// Stable failure reasons (documented in docs/30-configuration.md).
extern const char* const kNotRegular;  // "not a regular file"
extern const char* const kTooLarge;    // "source too large"
extern const char* const kTimeout;     // "timeout"
extern const char* const kOutOfRange;  // "value out of range"

struct RecordSpec {
  enum class Selector { Whole, LinePrefix, LineNumber, JsonPointer };

  std::string metric;  // <namespace>_<subsystem>_<name>, the -putmetric key
  prom::MetricType type = prom::MetricType::Gauge;
  Selector selector = Selector::Whole;
  std::string linePrefix;
  int64_t lineNumber = 0;  // 1-based
  int64_t field = 1;       // 1-based
  std::string pointer;     // as written, for reasons
  std::vector<std::string> pointerTokens;  // unescaped reference tokens
  double scale = 1;
};

// Parse one `record` entry. errKey receives the key the error is about
// ("" for the record itself, else ".metric", ".line", ...). The metric is
// not looked up here; newSensorSpecs does that.
bool parseRecord(const Json& raw, RecordSpec* out, std::string* errKey,
                 std::string* err);

// A finite number in strtod's grammar, white space trimmed: sources write
// hex and the like, and what is found here is published through
// formatValue, whose text Metric::record always accepts.
bool parseNumber(const std::string& token, double* out);

// Extract the record's number from `body` and apply its scale. On failure
// returns false and sets *reason to a stable reason.
bool extract(const std::string& body, const RecordSpec& rec, double* out,
             std::string* reason);

// Shortest decimal text that strtod reads back as exactly `v`
// (prom::formatValue).
std::string formatValue(double v);

// Read a regular file to EOF without ever blocking on a FIFO or a tty.
bool readFileSource(const std::string& path, std::string* body,
                    std::string* reason);

// Running-total -> increase. The first value sets the baseline, a
// decrease is a reset of the source and publishes the new value.
class CounterBaseline {
 public:
  // true when *delta is to be published
  bool feed(double value, double* delta);
  void reset() { have_ = false; }

 private:
  bool have_ = false;
  double last_ = 0;
};

struct SensorSpec {
  std::string name;
  bool isHttp = false;
  std::string file;
  health::ProbeSpec http;   // address, path and headers of an http source
  std::string httpTarget;   // numeric "ip:port" for the blocking client
  Duration interval{0};
  Duration timeout{0};
  std::vector<RecordSpec> records;
};

// Parse `telemetry.sensors`. `metrics` maps each configured metric key to
// its collector type. Errors name their position:
// telemetry.sensors[<name>].record[<i>].<key> ...
bool newSensorSpecs(const Json& raw,
                    const std::map<std::string, prom::MetricType>& metrics,
                    std::vector<std::shared_ptr<SensorSpec>>* out,
                    std::string* err);

// Fixed pool of at most kMaxWorkers threads running blocking fetches.
class WorkerPool {
 public:
  explicit WorkerPool(size_t threads);
  ~WorkerPool();
  WorkerPool(const WorkerPool&) = delete;
  WorkerPool& operator=(const WorkerPool&) = delete;

  void submit(std::function<void()> fn);
  // drop queued work, wait for running work, join; idempotent
  void stop();

 private:
  void work();
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> queue_;
  bool stopping_ = false;
  std::vector<std::thread> threads_;
};

class Sensor : public std::enable_shared_from_this<Sensor> {
 public:
  Sensor(std::shared_ptr<const SensorSpec> spec,
         std::shared_ptr<prom::Family> samples);

  const std::string& name() const { return spec_->name; }

  // Arm the interval timer (loop thread only). The bus is held weakly: a
  // result that outlives its bus is dropped.
  void start(Loop& loop, const std::shared_ptr<Bus>& bus, WorkerPool* pool);
  // Cancel the timer and any in-flight fetch; nothing is published after
  // this returns. A later start() begins with fresh counter baselines.
  void stop();

  // One sample now, as the timer would (loop thread only). Skipped when
  // the previous sample is still in flight.
  void tick();

  bool inFlight() const { return inFlight_; }
  uint64_t okCount() const { return ok_; }
  uint64_t errorCount() const { return errors_; }
  uint64_t skippedTicks() const { return skipped_; }

 private:
  struct Fetched {
    bool ok = false;
    std::string body;
    std::string reason;
  };
  static Fetched fetch(const SensorSpec& spec, http::CancelToken* cancel);
  void onFetched(uint64_t run, Fetched result);
  void finish(bool good, const std::string& reason);

  std::shared_ptr<const SensorSpec> spec_;
  std::shared_ptr<prom::Family> samples_;
  std::vector<CounterBaseline> baselines_;  // one per record

  Loop* loop_ = nullptr;
  WorkerPool* pool_ = nullptr;
  std::weak_ptr<Bus> bus_;
  uint64_t timer_ = 0;
  uint64_t deadline_ = 0;
  uint64_t run_ = 0;  // bumped by stop(): results of older runs are dropped
  bool started_ = false;
  bool inFlight_ = false;
  bool timedOut_ = false;
  bool bad_ = false;  // last sample failed (log on transitions only)
  std::shared_ptr<http::CancelToken> cancel_;
  uint64_t ok_ = 0, errors_ = 0, skipped_ = 0;
};

// Everything `telemetry.sensors` runs in one config generation.
class Sensors {
 public:
  explicit Sensors(const std::vector<std::shared_ptr<SensorSpec>>& specs);
  ~Sensors();

  void start(Loop& loop, const std::shared_ptr<Bus>& bus);
  // cancel timers and in-flight http fetches, join the workers
  void stop();

  const std::vector<std::shared_ptr<Sensor>>& sensors() const {
    return sensors_;
  }

 private:
  std::vector<std::shared_ptr<Sensor>> sensors_;
  std::unique_ptr<WorkerPool> pool_;
};

}  // namespace sensor
}  // namespace cpilot
