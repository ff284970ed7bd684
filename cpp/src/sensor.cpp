#include "cpilot/sensor.hpp"

#include <arpa/inet.h>
#include <fcntl.h>
#include <netinet/in.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "cpilot/decode.hpp"
#include "cpilot/ips.hpp"
#include "cpilot/log.hpp"

namespace cpilot {
namespace sensor {

const char* const kNotRegular = "not a regular file";
const char* const kTooLarge = "source too large";
const char* const kTimeout = "timeout";
const char* const kOutOfRange = "value out of range";

namespace {

// white space of the "C" locale, whatever locale the process runs in
bool isSpace(char c) {
  return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' ||
         c == '\r';
}

// narrows [*a, *b) of s past the white space at either end
void trimRange(const std::string& s, size_t* a, size_t* b) {
  while (*a < *b && isSpace(s[*a])) (*a)++;
  while (*b > *a && isSpace(s[*b - 1])) (*b)--;
}

std::string notANumber(const std::string& token) {
  // a NUL would end the reason early in every C string it passes through
  std::string shown;
  for (char c : token.substr(0, kMaxQuotedToken)) {
    if (c == '\0') shown += "\\0";
    else shown += c;
  }
  if (token.size() > kMaxQuotedToken) shown += "...";
  return "not a number: \"" + shown + "\"";
}

// [begin, end) of line `want` (1-based), or of the first line that starts
// with `prefix` after leading white space when want == 0. A final piece
// without a newline is a line; the empty piece after a final newline is
// not.
bool findLine(const std::string& body, int64_t want, const std::string& prefix,
              size_t* begin, size_t* end) {
  size_t pos = 0;
  int64_t n = 0;
  while (pos < body.size()) {
    size_t nl = body.find('\n', pos);
    size_t stop = nl == std::string::npos ? body.size() : nl;
    n++;
    if (want > 0) {
      if (n == want) {
        *begin = pos;
        *end = stop;
        return true;
      }
    } else {
      size_t a = pos, b = stop;
      trimRange(body, &a, &b);
      if (stop - a >= prefix.size() &&
          body.compare(a, prefix.size(), prefix) == 0) {
        *begin = pos;
        *end = stop;
        return true;
      }
    }
    if (nl == std::string::npos) break;
    pos = nl + 1;
  }
  return false;
}

// token `field` (1-based) of body[begin, end); *count receives the number
// of tokens when there are fewer
bool findField(const std::string& body, size_t begin, size_t end,
               int64_t field, std::string* token, int64_t* count) {
  int64_t n = 0;
  size_t pos = begin;
  while (pos < end) {
    while (pos < end && isSpace(body[pos])) pos++;
    if (pos >= end) break;
    size_t start = pos;
    while (pos < end && !isSpace(body[pos])) pos++;
    if (++n == field) {
      token->assign(body, start, pos - start);
      return true;
    }
  }
  *count = n;
  return false;
}

bool isArrayIndex(const std::string& tok, size_t* out) {
  if (tok.empty() || tok.size() > 18) return false;
  if (tok.size() > 1 && tok[0] == '0') return false;
  size_t v = 0;
  for (char c : tok) {
    if (c < '0' || c > '9') return false;
    v = v * 10 + (size_t)(c - '0');
  }
  *out = v;
  return true;
}

bool parsePointer(const std::string& ptr, std::vector<std::string>* tokens,
                  std::string* err) {
  tokens->clear();
  if (ptr.empty()) return true;
  if (ptr[0] != '/') {
    *err = "must be an RFC 6901 pointer: empty or starting with '/'";
    return false;
  }
  std::string cur;
  for (size_t i = 1; i <= ptr.size(); i++) {
    if (i == ptr.size() || ptr[i] == '/') {
      tokens->push_back(cur);
      cur.clear();
      continue;
    }
    if (ptr[i] == '~') {
      char next = i + 1 < ptr.size() ? ptr[i + 1] : '\0';
      if (next != '0' && next != '1') {
        *err = "has a '~' that is not part of '~0' or '~1'";
        return false;
      }
      cur += next == '0' ? '~' : '/';
      i++;
      continue;
    }
    cur += ptr[i];
  }
  return true;
}

const char* jsonTypeName(const Json& v) {
  switch (v.type()) {
    case Json::Type::Null: return "null";
    case Json::Type::Bool: return "bool";
    case Json::Type::Array: return "array";
    case Json::Type::Object: return "object";
    default: return "value";
  }
}

bool extractJson(const std::string& body, const RecordSpec& rec, double* out,
                 std::string* reason) {
  Json doc;
  try {
    doc = parseJson5(body);
  } catch (const std::exception& e) {
    *reason = std::string("json: ") + e.what();
    return false;
  }
  const Json* cur = &doc;
  for (auto& tok : rec.pointerTokens) {
    const Json* next = nullptr;
    if (cur->isObject()) {
      next = cur->find(tok);
    } else if (cur->isArray()) {
      size_t idx = 0;
      if (isArrayIndex(tok, &idx) && idx < cur->array().size())
        next = &cur->array()[idx];
    }
    if (!next) {
      *reason = "json: no value at " + rec.pointer;
      return false;
    }
    cur = next;
  }
  if (cur->isNumber()) {
    *out = cur->asDouble();
    if (!std::isfinite(*out)) {
      *reason = notANumber(formatValue(*out));
      return false;
    }
    return true;
  }
  if (cur->isString()) {
    if (parseNumber(cur->str(), out)) return true;
    *reason = notANumber(cur->str());
    return false;
  }
  *reason = notANumber(jsonTypeName(*cur));
  return false;
}

std::string numericTarget(const health::ProbeSpec& spec) {
  char buf[INET6_ADDRSTRLEN] = {0};
  int port = 0;
  if (spec.addr.ss_family == AF_INET6) {
    auto* sa = reinterpret_cast<const struct sockaddr_in6*>(&spec.addr);
    inet_ntop(AF_INET6, &sa->sin6_addr, buf, sizeof(buf));
    port = ntohs(sa->sin6_port);
  } else {
    auto* sa = reinterpret_cast<const struct sockaddr_in*>(&spec.addr);
    inet_ntop(AF_INET, &sa->sin_addr, buf, sizeof(buf));
    port = ntohs(sa->sin_port);
  }
  return std::string(buf) + ":" + std::to_string(port);
}

}  // namespace

// ---------------- extraction ----------------

bool parseNumber(const std::string& token, double* out) {
  size_t a = 0, b = token.size();
  trimRange(token, &a, &b);
  if (a == b) return false;
  std::string v = token.substr(a, b - a);
  char* end = nullptr;
  double val = strtod(v.c_str(), &end);
  // compare against the real end: an embedded NUL must not pass
  if (end != v.c_str() + v.size()) return false;
  if (!std::isfinite(val)) return false;
  *out = val;
  return true;
}

bool extract(const std::string& body, const RecordSpec& rec, double* out,
             std::string* reason) {
  double value = 0;
  switch (rec.selector) {
    case RecordSpec::Selector::Whole: {
      if (!parseNumber(body, &value)) {
        size_t a = 0, b = body.size();
        trimRange(body, &a, &b);
        *reason = notANumber(body.substr(a, b - a));
        return false;
      }
      break;
    }
    case RecordSpec::Selector::LinePrefix:
    case RecordSpec::Selector::LineNumber: {
      bool byNumber = rec.selector == RecordSpec::Selector::LineNumber;
      size_t begin = 0, end = 0;
      if (!findLine(body, byNumber ? rec.lineNumber : 0, rec.linePrefix,
                    &begin, &end)) {
        *reason = byNumber
                      ? "no line " + std::to_string(rec.lineNumber)
                      : "no line starts with \"" + rec.linePrefix + "\"";
        return false;
      }
      std::string token;
      int64_t count = 0;
      if (!findField(body, begin, end, rec.field, &token, &count)) {
        *reason = "line has " + std::to_string(count) + " fields";
        return false;
      }
      if (!parseNumber(token, &value)) {
        *reason = notANumber(token);
        return false;
      }
      break;
    }
    case RecordSpec::Selector::JsonPointer:
      if (!extractJson(body, rec, &value, reason)) return false;
      break;
  }
  value *= rec.scale;
  if (!std::isfinite(value)) {
    *reason = kOutOfRange;
    return false;
  }
  *out = value;
  return true;
}

// the exposition's printer, so a sample reads the same on /metrics as in
// the event that carried it
std::string formatValue(double v) { return prom::formatValue(v); }

bool CounterBaseline::feed(double value, double* delta) {
  if (!have_) {
    have_ = true;
    last_ = value;
    return false;
  }
  *delta = value >= last_ ? value - last_ : value;
  last_ = value;
  return true;
}

// ---------------- file source ----------------

bool readFileSource(const std::string& path, std::string* body,
                    std::string* reason) {
  body->clear();
  int fd;
  do {
    fd = open(path.c_str(), O_RDONLY | O_NONBLOCK | O_CLOEXEC | O_NOCTTY);
  } while (fd < 0 && errno == EINTR);
  if (fd < 0) {
    *reason = std::string("open: ") + strerror(errno);
    return false;
  }
  struct stat st;
  if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) {
    close(fd);
    *reason = kNotRegular;
    return false;
  }
  // to EOF: procfs and sysfs report size 0 or a page
  char buf[16384];
  while (true) {
    ssize_t n = read(fd, buf, sizeof(buf));
    if (n > 0) {
      body->append(buf, (size_t)n);
      if (body->size() > kMaxSourceBytes) {
        close(fd);
        body->clear();
        *reason = kTooLarge;
        return false;
      }
    } else if (n == 0) {
      break;
    } else if (errno != EINTR) {
      *reason = std::string("read: ") + strerror(errno);
      close(fd);
      body->clear();
      return false;
    }
  }
  close(fd);
  return true;
}

// ---------------- config ----------------

bool parseRecord(const Json& raw, RecordSpec* out, std::string* errKey,
                 std::string* err) {
  errKey->clear();
  if (!raw.isObject()) {
    *err = "must be an object";
    return false;
  }
  if (!decode::checkKeys(
          raw, {"metric", "line", "lineNumber", "field", "json", "scale"}, err))
    return false;

  const Json* metric = raw.find("metric");
  if (!metric || !metric->isString() || metric->str().empty()) {
    *errKey = ".metric";
    *err = "is required and must be a string";
    return false;
  }
  out->metric = metric->str();

  const Json* line = decode::given(raw, "line");
  const Json* lineNumber = decode::given(raw, "lineNumber");
  const Json* field = decode::given(raw, "field");
  const Json* json = decode::given(raw, "json");
  if (json && (line || lineNumber || field)) {
    *errKey = ".json";
    *err = "cannot be combined with 'line', 'lineNumber' or 'field'";
    return false;
  }
  if (line && lineNumber) {
    *errKey = ".line";
    *err = "cannot be combined with 'lineNumber'";
    return false;
  }
  if (field && !line && !lineNumber) {
    *errKey = ".field";
    *err = "needs 'line' or 'lineNumber'";
    return false;
  }
  if (json) {
    if (!json->isString()) {
      *errKey = ".json";
      *err = "must be a string";
      return false;
    }
    out->pointer = json->str();
    if (!parsePointer(out->pointer, &out->pointerTokens, err)) {
      *errKey = ".json";
      return false;
    }
    out->selector = RecordSpec::Selector::JsonPointer;
  }
  if (line) {
    if (!line->isString() || line->str().empty() ||
        line->str().find('\n') != std::string::npos ||
        isSpace(line->str()[0])) {
      *errKey = ".line";
      *err = "must be a non-empty string without a newline that does not "
             "start with white space";
      return false;
    }
    out->linePrefix = line->str();
    out->selector = RecordSpec::Selector::LinePrefix;
  }
  if (lineNumber) {
    if (!lineNumber->isInt() || lineNumber->asInt() < 1) {
      *errKey = ".lineNumber";
      *err = "must be an int >= 1";
      return false;
    }
    out->lineNumber = lineNumber->asInt();
    out->selector = RecordSpec::Selector::LineNumber;
  }
  if (field) {
    if (!field->isInt() || field->asInt() < 1) {
      *errKey = ".field";
      *err = "must be an int >= 1";
      return false;
    }
    out->field = field->asInt();
  }
  if (const Json* scale = decode::given(raw, "scale")) {
    if (!scale->isNumber() || !std::isfinite(scale->asDouble())) {
      *errKey = ".scale";
      *err = "must be a finite number";
      return false;
    }
    out->scale = scale->asDouble();
  }
  return true;
}

bool newSensorSpecs(const Json& raw,
                    const std::map<std::string, prom::MetricType>& metrics,
                    std::vector<std::shared_ptr<SensorSpec>>* out,
                    std::string* err) {
  out->clear();
  if (raw.isNull()) return true;
  if (!raw.isArray()) {
    *err = "telemetry.sensors must be an array";
    return false;
  }
  std::set<std::string> names;
  size_t index = 0;
  for (auto& s : raw.array()) {
    std::string at = "telemetry.sensors[" + std::to_string(index++) + "]";
    if (!s.isObject()) {
      *err = at + " must be an object";
      return false;
    }
    auto spec = std::make_shared<SensorSpec>();
    const Json* name = s.find("name");
    if (!name || !name->isString() || name->str().empty()) {
      *err = at + ".name is required and must be a string";
      return false;
    }
    spec->name = name->str();
    at = "telemetry.sensors[" + spec->name + "]";
    std::string sub;
    if (!validateServiceName(spec->name, &sub)) {
      *err = at + ".name: " + sub;
      return false;
    }
    if (!names.insert(spec->name).second) {
      *err = at + ".name must be unique among sensors";
      return false;
    }
    if (!decode::checkKeys(
            s, {"name", "file", "http", "interval", "timeout", "record"},
            &sub)) {
      *err = at + ": " + sub;
      return false;
    }

    const Json* file = decode::given(s, "file");
    const Json* http = decode::given(s, "http");
    if ((file != nullptr) == (http != nullptr)) {
      *err = at + " needs exactly one of 'file' and 'http'";
      return false;
    }
    if (file) {
      if (!file->isString() || file->str().empty() || file->str()[0] != '/' ||
          file->str().find('\0') != std::string::npos) {
        *err = at + ".file must be an absolute path";
        return false;
      }
      spec->file = file->str();
    } else {
      for (const char* key : {"method", "expect"}) {
        if (http->isObject() && http->find(key)) {
          *err = at + ".http." + key +
                 " is not accepted for sensors: the method is GET and any "
                 "2xx status is success";
          return false;
        }
      }
      std::string key;
      if (!health::parseHttpProbe(*http, &spec->http, &key, &sub)) {
        *err = at + ".http" + key + ": " + sub;
        return false;
      }
      spec->isHttp = true;
      spec->httpTarget = numericTarget(spec->http);
    }

    const Json* interval = decode::given(s, "interval");
    if (!interval || !parsePositiveDuration(*interval, &spec->interval)) {
      *err = at + ".interval must be > 0";
      return false;
    }
    spec->timeout = spec->interval;
    if (const Json* timeout = decode::given(s, "timeout")) {
      if (!parsePositiveDuration(*timeout, &spec->timeout)) {
        *err = at + ".timeout must be > 0";
        return false;
      }
    }
    spec->http.timeout = spec->timeout;

    const Json* record = decode::given(s, "record");
    if (!record || !record->isArray() || record->array().empty()) {
      *err = at + ".record must be a non-empty array";
      return false;
    }
    size_t ri = 0;
    for (auto& r : record->array()) {
      std::string rat = at + ".record[" + std::to_string(ri++) + "]";
      RecordSpec rec;
      std::string key;
      if (!parseRecord(r, &rec, &key, &sub)) {
        *err = rat + key + (key.empty() ? ": " : " ") + sub;
        return false;
      }
      auto it = metrics.find(rec.metric);
      if (it == metrics.end()) {
        *err = rat + ".metric '" + rec.metric +
               "' is not the <namespace>_<subsystem>_<name> key of a metric "
               "in telemetry.metrics";
        return false;
      }
      rec.type = it->second;
      spec->records.push_back(std::move(rec));
    }
    out->push_back(spec);
  }
  return true;
}

// ---------------- worker pool ----------------

WorkerPool::WorkerPool(size_t threads) {
  if (threads > kMaxWorkers) threads = kMaxWorkers;
  for (size_t i = 0; i < threads; i++)
    threads_.emplace_back([this] {
      resetThreadScheduling();
      work();
    });
}

WorkerPool::~WorkerPool() { stop(); }

void WorkerPool::submit(std::function<void()> fn) {
  {
    std::lock_guard<std::mutex> l(mu_);
    if (stopping_) return;
    queue_.push_back(std::move(fn));
  }
  cv_.notify_one();
}

void WorkerPool::stop() {
  {
    std::lock_guard<std::mutex> l(mu_);
    stopping_ = true;
    queue_.clear();
  }
  cv_.notify_all();
  for (auto& t : threads_)
    if (t.joinable()) t.join();
  threads_.clear();
}

void WorkerPool::work() {
  while (true) {
    std::function<void()> fn;
    {
      std::unique_lock<std::mutex> l(mu_);
      cv_.wait(l, [this] { return stopping_ || !queue_.empty(); });
      if (stopping_) return;
      fn = std::move(queue_.front());
      queue_.pop_front();
    }
    fn();
  }
}

// ---------------- sensor runtime ----------------

Sensor::Sensor(std::shared_ptr<const SensorSpec> spec,
               std::shared_ptr<prom::Family> samples)
    : spec_(std::move(spec)),
      samples_(std::move(samples)),
      baselines_(spec_->records.size()) {}

void Sensor::start(Loop& loop, const std::shared_ptr<Bus>& bus,
                   WorkerPool* pool) {
  if (started_) stop();
  loop_ = &loop;
  pool_ = pool;
  bus_ = bus;
  started_ = true;
  bad_ = false;
  for (auto& b : baselines_) b.reset();
  if (samples_) {
    // both series exist from the start, so a scrape can tell "no errors"
    // from "no such sensor"
    samples_->inc({spec_->name, "ok"}, 0);
    samples_->inc({spec_->name, "error"}, 0);
  }
  // the per-name phase offset jobs use: N sensors created at the same
  // instant do not sample in one burst
  uint64_t h = std::hash<std::string>{}(spec_->name);
  Duration phase(spec_->interval.count() / 2 +
                 (Ns::rep)(h % 1000) * spec_->interval.count() / 2000);
  auto self = shared_from_this();
  timer_ = loop.addInterval(spec_->interval, [this, self] { tick(); }, phase);
}

void Sensor::stop() {
  if (!started_) return;
  started_ = false;
  run_++;
  if (timer_) loop_->cancelTimer(timer_);
  if (deadline_) loop_->cancelTimer(deadline_);
  timer_ = deadline_ = 0;
  if (cancel_) cancel_->cancel();
  cancel_.reset();
  inFlight_ = false;
  timedOut_ = false;
  bus_.reset();
}

void Sensor::tick() {
  if (!started_) return;
  if (inFlight_) {
    // single-instance skip, as Probe::run: never queued
    skipped_++;
    LOG_DEBUG("sensor %s still in flight, skipping this tick",
              spec_->name.c_str());
    return;
  }
  inFlight_ = true;
  timedOut_ = false;
  auto self = shared_from_this();
  std::shared_ptr<http::CancelToken> cancel;
  if (spec_->isHttp) {
    cancel = cancel_ = std::make_shared<http::CancelToken>();
    // a deadline for the whole fetch: the client's own timeout bounds
    // each read, not their sum
    deadline_ = loop_->addTimeout(spec_->timeout, [this, self] {
      deadline_ = 0;
      timedOut_ = true;
      if (cancel_) cancel_->cancel();
    });
  }
  Loop* loop = loop_;
  uint64_t loopId = loop_->id();
  uint64_t run = run_;
  auto spec = spec_;
  pool_->submit([self, spec, cancel, loop, loopId, run] {
    Fetched result = fetch(*spec, cancel.get());
    auto boxed = std::make_shared<Fetched>(std::move(result));
    Loop::postIfLive(loop, loopId, [self, run, boxed] {
      self->onFetched(run, std::move(*boxed));
    });
  });
}

Sensor::Fetched Sensor::fetch(const SensorSpec& spec,
                              http::CancelToken* cancel) {
  Fetched out;
  if (!spec.isHttp) {
    out.ok = readFileSource(spec.file, &out.body, &out.reason);
    return out;
  }
  http::Headers headers;
  for (auto& kv : spec.http.headers) headers[kv.first] = kv.second;
  auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(spec.timeout)
                .count();
  TimePoint began = Clock::now();
  http::ClientResult res = http::request(
      spec.httpTarget, "GET", spec.http.path, "", "application/json", headers,
      (int)std::min<long long>(ms, 3600 * 1000), nullptr, cancel,
      kMaxSourceBytes);
  if (!res.ok) {
    if (res.error == http::kBodyTooLarge) out.reason = kTooLarge;
    else if (Clock::now() - began >= spec.timeout) out.reason = kTimeout;
    else out.reason = res.error;
    return out;
  }
  if (res.status < 200 || res.status > 299) {
    out.reason = "status " + std::to_string(res.status);
    return out;
  }
  out.ok = true;
  out.body = std::move(res.body);
  return out;
}

void Sensor::onFetched(uint64_t run, Fetched result) {
  // a result of a run that stop() ended belongs to a drained generation
  if (run != run_ || !started_) return;
  inFlight_ = false;
  if (deadline_) {
    loop_->cancelTimer(deadline_);
    deadline_ = 0;
  }
  cancel_.reset();
  auto bus = bus_.lock();
  if (!bus) return;  // the bus was dropped under us: nothing to record into
  if (!result.ok) {
    finish(false, timedOut_ ? kTimeout : result.reason);
    return;
  }
  bool good = true;
  std::string firstReason;
  for (size_t i = 0; i < spec_->records.size(); i++) {
    const RecordSpec& rec = spec_->records[i];
    double value = 0;
    std::string reason;
    if (!extract(result.body, rec, &value, &reason)) {
      if (good)
        firstReason = "record[" + std::to_string(i) + "] " + rec.metric +
                      ": " + reason;
      good = false;
      continue;
    }
    if (rec.type == prom::MetricType::Counter) {
      double delta = 0;
      if (!baselines_[i].feed(value, &delta)) continue;
      value = delta;
    }
    bus->publish(
        Event{EventCode::Metric, rec.metric + "|" + formatValue(value)});
  }
  finish(good, firstReason);
}

void Sensor::finish(bool good, const std::string& reason) {
  if (good) {
    ok_++;
    if (samples_) samples_->inc({spec_->name, "ok"});
    if (bad_) LOG_INFO("sensor %s: recovered", spec_->name.c_str());
  } else {
    errors_++;
    if (samples_) samples_->inc({spec_->name, "error"});
    if (!bad_)
      LOG_WARN("sensor %s: sample failed: %s", spec_->name.c_str(),
               reason.c_str());
  }
  bad_ = !good;
}

// ---------------- the generation's set ----------------

Sensors::Sensors(const std::vector<std::shared_ptr<SensorSpec>>& specs) {
  if (specs.empty()) return;
  // internal collector: lives across reloads like the bus's own, and is
  // registered only here so a config without sensors exposes no new family
  auto samples = prom::Registry::global().registerFamily(
      "containerpilot_sensor_samples",
      "count of telemetry sensor samples, partitioned by sensor and result",
      prom::MetricType::Counter, {"sensor", "result"});
  for (auto& spec : specs)
    sensors_.push_back(std::make_shared<Sensor>(spec, samples));
}

Sensors::~Sensors() { stop(); }

void Sensors::start(Loop& loop, const std::shared_ptr<Bus>& bus) {
  if (sensors_.empty()) return;
  if (!pool_)
    pool_ = std::make_unique<WorkerPool>(
        std::min(sensors_.size(), kMaxWorkers));
  for (auto& s : sensors_) s->start(loop, bus, pool_.get());
}

void Sensors::stop() {
  for (auto& s : sensors_) s->stop();
  // in-flight http fetches were shut down above; a file read in flight is
  // waited for
  if (pool_) pool_->stop();
  pool_.reset();
}

}  // namespace sensor
}  // namespace cpilot
