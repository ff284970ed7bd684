#include "cpilot/signals.hpp"

#include <signal.h>

#include <cerrno>
#include <cstring>

#include "cpilot/decode.hpp"

namespace cpilot {
namespace signals {

namespace {

constexpr auto kMinWait = std::chrono::milliseconds(1);

struct Entry {
  const char* name;  // without the prefix
  int signo;
};
const Entry kTable[] = {
    {"HUP", SIGHUP},   {"INT", SIGINT},   {"QUIT", SIGQUIT},
    {"TERM", SIGTERM}, {"USR1", SIGUSR1}, {"USR2", SIGUSR2},
    {"WINCH", SIGWINCH}, {"CONT", SIGCONT},
};

}  // namespace

const char* kNoProcess = "no running process";

bool fromName(const std::string& name, int* signo, std::string* canonical) {
  std::string bare = name.compare(0, 3, "SIG") == 0 ? name.substr(3) : name;
  for (const Entry& e : kTable) {
    if (bare == e.name) {
      if (signo) *signo = e.signo;
      if (canonical) *canonical = std::string("SIG") + e.name;
      return true;
    }
  }
  return false;
}

std::string acceptedNames() {
  std::string out;
  for (const Entry& e : kTable) {
    if (!out.empty()) out += ", ";
    out += std::string("SIG") + e.name;
  }
  return out;
}

bool parseSpec(const Json& raw, Spec* out, std::string* key,
               std::string* err) {
  key->clear();
  if (!raw.isObject()) {
    *err = "must be an object";
    return false;
  }
  if (!decode::checkKeys(raw, {"job", "send", "group", "wait"}, err))
    return false;

  const Json* job = raw.find("job");
  if (!job || !job->isString() || job->str().empty()) {
    *key = ".job";
    *err = "must be the name of a job with an 'exec'";
    return false;
  }
  out->job = job->str();

  const Json* send = raw.find("send");
  if (!send || !send->isString() ||
      !fromName(send->str(), &out->signo, &out->name)) {
    *key = ".send";
    if (!send || send->isNull()) {
      *err = "is required: must be one of " + acceptedNames();
    } else {
      *err = "'" + (send->isString() ? send->str() : send->dump()) +
             "' is not accepted: must be one of " + acceptedNames();
    }
    return false;
  }

  out->group = false;
  if (const Json* group = raw.find("group")) {
    if (!decode::toBool(*group, &out->group)) {
      *key = ".group";
      *err = "cannot parse 'group' as bool";
      return false;
    }
  }

  out->wait = Duration(0);
  const Json* wait = raw.find("wait");
  if (wait && !wait->isNull()) {
    *key = ".wait";
    std::string text;
    decode::toString(*wait, &text);
    try {
      out->wait = getTimeout(text);
    } catch (const std::exception& e) {
      *err = "'" + text + "': " + e.what();
      return false;
    }
    if (out->wait < kMinWait) {
      *err = "'" + text + "' cannot be less than 1ms";
      return false;
    }
    key->clear();
  }
  return true;
}

bool deliver(pid_t pid, int signo, bool group, std::string* reason) {
  if (pid <= 0) {
    *reason = kNoProcess;
    return false;
  }
  if (::kill(group ? -pid : pid, signo) != 0) {
    *reason = strerror(errno);
    return false;
  }
  return true;
}

}  // namespace signals
}  // namespace cpilot
