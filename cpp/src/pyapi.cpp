// C API for the Python harness (loaded with ctypes as
// containerpilot_amd/_native.so). Exposes the pure config-pipeline
// components so Python tests exercise the same native code paths the
// daemon runs.
#include <cstdlib>
#include <cstring>
#include <string>

#include "cpilot/config.hpp"
#include "cpilot/discovery.hpp"
#include "cpilot/json.hpp"
#include "cpilot/sensor.hpp"
#include "cpilot/signals.hpp"
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

}  // extern "C"
