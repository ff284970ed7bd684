// C API for the Python harness (loaded with ctypes as
// containerpilot_amd/_native.so). Exposes the pure config-pipeline
// components so Python tests exercise the same native code paths the
// daemon runs.
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "cpilot/config.hpp"
#include "cpilot/control.hpp"
#include "cpilot/discovery.hpp"
#include "cpilot/jobs.hpp"
#include "cpilot/json.hpp"
#include "cpilot/sensor.hpp"
#include "cpilot/signals.hpp"
#include "cpilot/telemetry.hpp"
#include "cpilot/timing.hpp"
#include "cpilot/tmpl.hpp"
#include "cpilot/version.hpp"
#include "cpilot/watches.hpp"

using namespace cpilot;

namespace {
char* dupString(const std::string& s) {
  char* out = (char*)malloc(s.size() + 1);
  memcpy(out, s.c_str(), s.size() + 1);
  return out;
}
}  // namespace

extern "C" {

const char* cp_version() { return kVersion; }

void cp_free(char* p) { free(p); }

// Render a config template against the current environment.
// Returns malloc'd result; on error returns nullptr and fills *errOut.
char* cp_render_template(const char* text, char** errOut) {
  try {
    return dupString(renderTemplate(text));
  } catch (const std::exception& e) {
    if (errOut) *errOut = dupString(e.what());
    return nullptr;
  }
}

// Render a data template (the language of a watch's `render` file) against
// an arbitrary JSON value: "." and "$" start as that value.
// Returns nullptr + *errOut on a bad document or a template error.
char* cp_render_data(const char* templateText, const char* dataJson,
                     char** errOut) {
  try {
    Json data = parseJson5(dataJson);
    return dupString(Template::parse(templateText).render(data));
  } catch (const std::exception& e) {
    if (errOut) *errOut = dupString(e.what());
    return nullptr;
  }
}

// Parse a duration (JSON5 value text: bare int or quoted string).
// Returns nanoseconds, or -1 on error.
long long cp_parse_duration_ns(const char* text) {
  try {
    Json v = parseJson5(text);
    return (long long)parseDuration(v).count();
  } catch (const std::exception&) {
    return -1;
  }
}

// Same input as cp_parse_duration_ns, but a negative duration and an error
// stay apart: returns 1 and fills *outNs, or returns 0 on error.
int cp_parse_duration(const char* text, long long* outNs) {
  try {
    Json v = parseJson5(text);
    long long ns = (long long)parseDuration(v).count();
    if (outNs) *outNs = ns;
    return 1;
  } catch (const std::exception&) {
    return 0;
  }
}

// Convert JSON5 text to strict JSON. nullptr + *errOut on parse error.
char* cp_json5_to_json(const char* text, char** errOut) {
  try {
    return dupString(parseJson5(text).dump());
  } catch (const JsonParseError& e) {
    if (errOut) *errOut = dupString(formatParseError(text, e));
    return nullptr;
  } catch (const std::exception& e) {
    if (errOut) *errOut = dupString(e.what());
    return nullptr;
  }
}

// Validate a full (already rendered) config. Returns nullptr when valid,
// else a malloc'd error message.
char* cp_validate_config(const char* text) {
  std::string err;
  auto cfg = newConfig(text, &err);
  if (cfg) return nullptr;
  return dupString(err);
}

// Resolve the consul endpoint ("scheme://host:port") that the given
// `consul` config value + the current CONSUL_* environment produce
// (discovery/config.go:29-61 + api.DefaultConfig env handling).
// Returns nullptr + *errOut on config error.
char* cp_consul_endpoint(const char* consulJson, char** errOut) {
  try {
    Json raw = parseJson5(consulJson);
    std::string err;
    auto backend = ConsulBackend::create(&raw, &err);
    if (!backend) {
      if (errOut) *errOut = dupString(err);
      return nullptr;
    }
    return dupString(backend->scheme() + "://" + backend->address());
  } catch (const std::exception& e) {
    if (errOut) *errOut = dupString(e.what());
    return nullptr;
  }
}

// Dry-run of a watch's `render`: parse a raw /v1/health/service response
// body the way the daemon does, build the watch data model for service
// `name` (+tag, +dc) and render `templateText` against it.
// Returns nullptr + *errOut on a bad body or a template error.
char* cp_watch_render(const char* templateText, const char* healthBodyJson,
                      const char* name, const char* tag, const char* dc,
                      char** errOut) {
  try {
    bool ok = true;
    auto entries = parseHealthEntries(healthBodyJson, &ok);
    if (!ok) {
      if (errOut) *errOut = dupString("could not parse health response body");
      return nullptr;
    }
    Template tmpl = Template::parse(templateText);
    return dupString(tmpl.render(
        buildRenderData(name, tag ? tag : "", dc ? dc : "", entries)));
  } catch (const std::exception& e) {
    if (errOut) *errOut = dupString(e.what());
    return nullptr;
  }
}

// Decode a /v1/kv response body (bodyLen bytes) the way a key watch does.
// Returns a JSON list of {"Key", "ValueHex", "Flags"} sorted by key, the
// value as lower-case hex so it stays byte-exact; nullptr + *errOut on
// what the daemon treats as a failed query.
char* cp_kv_decode(const char* body, size_t bodyLen, char** errOut) {
  try {
    std::vector<KVEntry> entries;
    if (!parseKVEntries(std::string(body, bodyLen), &entries)) {
      if (errOut) *errOut = dupString("could not parse kv response body");
      return nullptr;
    }
    JsonArray rows;
    for (auto& e : entries) {
      std::string hex;
      for (unsigned char c : e.value) {
        const char* digits = "0123456789abcdef";
        hex += digits[c >> 4];
        hex += digits[c & 15];
      }
      rows.push_back(Json(JsonObject{{"Key", Json(e.key)},
                                     {"ValueHex", Json(std::move(hex))},
                                     {"Flags", Json((int64_t)e.flags)}}));
    }
    return dupString(Json(std::move(rows)).dump());
  } catch (const std::exception& e) {
    if (errOut) *errOut = dupString(e.what());
    return nullptr;
  }
}

// Dry-run of a key watch's `render`: decode `body` (bodyLen bytes; nullptr
// stands for the 404 of a missing key) the way the daemon does, build the
// data model of watch `name` on `key` (a prefix when `prefix` is non-zero)
// and render `templateText` against it. The rendering may hold any byte:
// returns a malloc'd buffer of *outLen bytes; nullptr + *errOut on a bad
// body or a template error.
char* cp_kv_render(const char* templateText, const char* body, size_t bodyLen,
                   const char* name, const char* key, int prefix,
                   const char* dc, size_t* outLen, char** errOut) {
  try {
    std::vector<KVEntry> entries;
    if (body && !parseKVEntries(std::string(body, bodyLen), &entries)) {
      if (errOut) *errOut = dupString("could not parse kv response body");
      return nullptr;
    }
    Template tmpl = Template::parse(templateText);
    std::string out = tmpl.render(
        buildKVRenderData(name, key, prefix != 0, dc ? dc : "", entries));
    char* buf = (char*)malloc(out.size() + 1);
    memcpy(buf, out.data(), out.size());
    buf[out.size()] = '\0';
    if (outLen) *outLen = out.size();
    return buf;
  } catch (const std::exception& e) {
    if (errOut) *errOut = dupString(e.what());
    return nullptr;
  }
}

// Dry-run of one sensor `record`: extract the number from `body` (bodyLen
// bytes, NULs allowed) the way the daemon does and apply the scale. The
// metric named by the record is not looked up.
// Returns 1 and fills *out, or 0 and fills *errOut with the stable reason
// (or the config error of a bad record).
int cp_sensor_extract(const char* body, size_t bodyLen, const char* recordJson,
                      double* out, char** errOut) {
  try {
    sensor::RecordSpec rec;
    std::string key, err;
    if (!sensor::parseRecord(parseJson5(recordJson), &rec, &key, &err)) {
      if (errOut)
        *errOut = dupString("record" + key + (key.empty() ? ": " : " ") + err);
      return 0;
    }
    double value = 0;
    if (!sensor::extract(std::string(body, bodyLen), rec, &value, &err)) {
      if (errOut) *errOut = dupString(err);
      return 0;
    }
    if (out) *out = value;
    return 1;
  } catch (const std::exception& e) {
    if (errOut) *errOut = dupString(e.what());
    return 0;
  }
}

// The number of a signal that `jobs[].signal.send`, POST /v3/signal and
// `-signal` accept, or -1 for a refused name (*errOut lists the accepted
// names).
int cp_signal_number(const char* name, char** errOut) {
  int signo = 0;
  if (signals::fromName(name, &signo, nullptr)) return signo;
  if (errOut)
    *errOut = dupString(std::string("'") + name +
                        "' is not accepted: must be one of " +
                        signals::acceptedNames());
  return -1;
}

// The exact bytes the http job `jobJson` (one entry of `jobs`) would write
// to its target: a malloc'd buffer of *outLen bytes, since a body may hold
// any byte. nullptr + *errOut with the config error of a refused job, or
// for a job without `http`.
char* cp_http_action_request(const char* jobJson, size_t* outLen,
                             char** errOut) {
  try {
    std::shared_ptr<JobConfig> cfg;
    std::string err;
    if (!validateJobConfig(parseJson5(jobJson), nullptr, &cfg, &err)) {
      if (errOut) *errOut = dupString(err);
      return nullptr;
    }
    if (!cfg->http) {
      if (errOut) *errOut = dupString("job[" + cfg->name + "] has no 'http'");
      return nullptr;
    }
    std::string out = health::buildProbeRequest(cfg->http->spec());
    char* buf = (char*)malloc(out.size() + 1);
    memcpy(buf, out.data(), out.size());
    buf[out.size()] = '\0';
    if (outLen) *outLen = out.size();
    return buf;
  } catch (const std::exception& e) {
    if (errOut) *errOut = dupString(e.what());
    return nullptr;
  }
}

// Replay a script against the daemon's own metrics path, in a registry of
// its own, and return the exposition:
//   {metrics:  [<telemetry.metrics entry>, ...],
//    events:   ["name|value", ...],
//    families: [{name, help, type, labels: [..], buckets: [..]}, ...],
//    ops:      [{family, op: "inc"|"set"|"observe"|"setBuckets",
//                labels: [..], value, bounds: [..]}, ...]}
// `metrics` go through newMetricConfigs and every event through each
// Metric::onEvent, in order; then `ops` run on the `families` (the
// internal-collector path). Returns nullptr + *errOut on a config error or
// a malformed script.
char* cp_metrics_replay(const char* scriptJson, char** errOut) {
  try {
    Json script = parseJson5(scriptJson);
    prom::Registry registry;
    std::string err;
    std::vector<std::shared_ptr<MetricConfig>> cfgs;
    if (const Json* m = script.find("metrics")) {
      if (!newMetricConfigs(*m, &cfgs, &err, &registry)) {
        if (errOut) *errOut = dupString(err);
        return nullptr;
      }
    }
    std::vector<std::shared_ptr<Metric>> metrics;
    for (auto& cfg : cfgs) metrics.push_back(std::make_shared<Metric>(cfg));
    if (const Json* events = script.find("events")) {
      for (auto& e : events->array())
        for (auto& metric : metrics)
          metric->onEvent(Event{EventCode::Metric, e.str()});
    }

    auto need = [](const Json& obj, const char* key) -> const Json& {
      const Json* v = obj.find(key);
      if (!v) throw std::runtime_error(std::string("script: missing ") + key);
      return *v;
    };
    auto strings = [](const Json* v) {
      std::vector<std::string> out;
      if (v)
        for (auto& s : v->array()) out.push_back(s.str());
      return out;
    };
    auto doubles = [](const Json* v) {
      std::vector<double> out;
      if (v)
        for (auto& d : v->array()) out.push_back(d.asDouble());
      return out;
    };
    std::map<std::string, std::shared_ptr<prom::Family>> families;
    if (const Json* fams = script.find("families")) {
      for (auto& f : fams->array()) {
        std::string name = need(f, "name").str();
        std::string type = need(f, "type").str();
        prom::MetricType mt;
        if (type == "counter") mt = prom::MetricType::Counter;
        else if (type == "gauge") mt = prom::MetricType::Gauge;
        else if (type == "histogram") mt = prom::MetricType::Histogram;
        else if (type == "summary") mt = prom::MetricType::Summary;
        else throw std::runtime_error("invalid metric type: " + type);
        const Json* help = f.find("help");
        auto fam = registry.registerFamily(name, help ? help->str() : "", mt,
                                           strings(f.find("labels")));
        if (const Json* b = f.find("buckets")) fam->setBuckets(doubles(b));
        families[name] = fam;
      }
    }
    if (const Json* ops = script.find("ops")) {
      for (auto& o : ops->array()) {
        auto it = families.find(need(o, "family").str());
        if (it == families.end())
          throw std::runtime_error("op on an undeclared family");
        std::string op = need(o, "op").str();
        auto labels = strings(o.find("labels"));
        const Json* value = o.find("value");
        double v = value ? value->asDouble() : 0;
        if (op == "inc") it->second->inc(labels, v);
        else if (op == "set") it->second->set(labels, v);
        else if (op == "observe") it->second->observe(labels, v);
        else if (op == "setBuckets")
          it->second->setBuckets(doubles(o.find("bounds")));
        else throw std::runtime_error("unknown op: " + op);
      }
    }
    return dupString(registry.expose());
  } catch (const std::exception& e) {
    if (errOut) *errOut = dupString(e.what());
    return nullptr;
  }
}

// What POST /v3/metric puts after "name|" for one JSON value.
char* cp_metric_value_string(const char* jsonText, char** errOut) {
  try {
    return dupString(metricValueString(parseJson5(jsonText)));
  } catch (const std::exception& e) {
    if (errOut) *errOut = dupString(e.what());
    return nullptr;
  }
}

}  // extern "C"
