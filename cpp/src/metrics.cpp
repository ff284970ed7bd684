#include "cpilot/metrics.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace cpilot {
namespace prom {

namespace {
std::string escapeLabel(const std::string& s) {
  std::string out;
  for (char c : s) {
    if (c == '\\') out += "\\\\";
    else if (c == '"') out += "\\\"";
    else if (c == '\n') out += "\\n";
    else out += c;
  }
  return out;
}

// HELP text escapes backslash and newline (text format 0.0.4)
std::string escapeHelp(const std::string& s) {
  std::string out;
  for (char c : s) {
    if (c == '\\') out += "\\\\";
    else if (c == '\n') out += "\\n";
    else out += c;
  }
  return out;
}

// the objectives every summary exposes, as exact fractions
struct Quantile {
  uint64_t num, den;
};
const Quantile kQuantiles[] = {{1, 2}, {9, 10}, {99, 100}};

std::string labelString(const std::vector<std::string>& names,
                        const std::vector<std::string>& values,
                        const std::string& extraName = "",
                        const std::string& extraValue = "") {
  std::string out;
  bool any = false;
  for (size_t i = 0; i < names.size() && i < values.size(); i++) {
    if (any) out += ",";
    out += names[i] + "=\"" + escapeLabel(values[i]) + "\"";
    any = true;
  }
  if (!extraName.empty()) {
    if (any) out += ",";
    out += extraName + "=\"" + extraValue + "\"";
    any = true;
  }
  if (!any) return "";
  return "{" + out + "}";
}
}  // namespace

std::string formatValue(double v) {
  if (std::isnan(v)) return "NaN";
  if (std::isinf(v)) return v > 0 ? "+Inf" : "-Inf";
  char buf[40];
  // whole numbers read better as digits than as "4e+01"
  // (most of a scrape is event counts, so this path stays an integer print;
  // the value is finite and in range here, so the cast is defined)
  if (std::fabs(v) < 1e15 && v == std::floor(v)) {
    if (v == 0 && std::signbit(v)) return "-0";
    snprintf(buf, sizeof(buf), "%lld", (long long)v);
    return buf;
  }
  for (int prec = 1; prec <= 17; prec++) {
    snprintf(buf, sizeof(buf), "%.*g", prec, v);
    if (strtod(buf, nullptr) == v) break;
  }
  return buf;
}

bool validMetricName(const std::string& name) {
  if (name.empty()) return false;
  for (size_t i = 0; i < name.size(); i++) {
    char c = name[i];
    bool ok = (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_' ||
              c == ':' || (i > 0 && c >= '0' && c <= '9');
    if (!ok) return false;
  }
  return true;
}

bool isInternalName(const std::string& name) {
  for (const char* internal :
       {"containerpilot_events", "containerpilot_event_dispatch_seconds",
        "containerpilot_event_deliveries",
        "containerpilot_control_http_requests",
        "containerpilot_watch_instances", "containerpilot_sensor_samples"})
    if (name == internal) return true;
  return false;
}

void Family::expose(std::string& out) const {
  std::lock_guard<std::mutex> l(mu_);
  const char* typeName;
  switch (type_) {
    case MetricType::Counter: typeName = "counter"; break;
    case MetricType::Gauge: typeName = "gauge"; break;
    case MetricType::Histogram: typeName = "histogram"; break;
    case MetricType::Summary: typeName = "summary"; break;
  }
  out += "# HELP " + name_ + " " + escapeHelp(help_) + "\n";
  out += "# TYPE " + name_ + " " + std::string(typeName) + "\n";
  // a family with no children still exposes one zero-value child for
  // unlabeled collectors (prometheus exposes e.g. user metrics at 0, a
  // histogram with zero buckets, a summary with NaN quantiles)
  std::map<std::vector<std::string>, Child> unobserved;
  if (children_.empty() && labelNames_.empty()) {
    Child& c = unobserved[{}];
    if (!bucketBounds_.empty()) c.hist.setBounds(bucketBounds_);
  }
  for (auto& kv : children_.empty() ? unobserved : children_) {
    const auto& labels = kv.first;
    const Child& c = kv.second;
    switch (type_) {
      case MetricType::Counter:
      case MetricType::Gauge:
        out += name_ + labelString(labelNames_, labels) + " " +
               formatValue(c.value) + "\n";
        break;
      case MetricType::Histogram: {
        uint64_t cumulative = 0;
        for (size_t i = 0; i < c.hist.bounds.size(); i++) {
          cumulative = c.hist.counts[i];
          out += name_ + "_bucket" +
                 labelString(labelNames_, labels, "le",
                             formatValue(c.hist.bounds[i])) +
                 " " + std::to_string(cumulative) + "\n";
        }
        out += name_ + "_bucket" +
               labelString(labelNames_, labels, "le", "+Inf") + " " +
               std::to_string(c.hist.count) + "\n";
        out += name_ + "_sum" + labelString(labelNames_, labels) + " " +
               formatValue(c.hist.sum) + "\n";
        out += name_ + "_count" + labelString(labelNames_, labels) + " " +
               std::to_string(c.hist.count) + "\n";
        break;
      }
      case MetricType::Summary: {
        for (const Quantile& q : kQuantiles) {
          out += name_ +
                 labelString(labelNames_, labels, "quantile",
                             formatValue((double)q.num / (double)q.den)) +
                 " " + formatValue(c.summ.quantile(q.num, q.den)) + "\n";
        }
        out += name_ + "_sum" + labelString(labelNames_, labels) + " " +
               formatValue(c.summ.sum) + "\n";
        out += name_ + "_count" + labelString(labelNames_, labels) + " " +
               std::to_string(c.summ.count) + "\n";
        break;
      }
    }
  }
}

Registry& Registry::global() {
  static Registry r;
  return r;
}

std::shared_ptr<Family> Registry::registerFamily(
    const std::string& name, const std::string& help, MetricType type,
    std::vector<std::string> labelNames, bool keepExisting) {
  std::lock_guard<std::mutex> l(mu_);
  for (auto it = families_.begin(); it != families_.end(); ++it) {
    if ((*it)->name() == name) {
      if (keepExisting && (*it)->type() == type) return *it;
      families_.erase(it);
      break;
    }
  }
  auto fam = std::make_shared<Family>(name, help, type, std::move(labelNames));
  families_.push_back(fam);
  return fam;
}

std::string Registry::expose() const {
  std::lock_guard<std::mutex> l(mu_);
  std::string out;
  for (auto& f : families_) f->expose(out);
  return out;
}

}  // namespace prom
}  // namespace cpilot
