// Signal actions: the name table, the `jobs[].signal` spec parser and the
// deliver function behind signal jobs, POST /v3/signal and `-signal`.
// Everything here is pure (no loop, no bus), so it is tested without a
// daemon. This is an extension: the reference needs a shell, `kill` and
// $CONTAINERPILOT_<NAME>_PID to signal a process it supervises.
#pragma once

#include <sys/types.h>

#include <string>

#include "cpilot/json.hpp"
#include "cpilot/timing.hpp"

namespace cpilot {
namespace signals {

// Accepts SIGHUP SIGINT SIGQUIT SIGTERM SIGUSR1 SIGUSR2 SIGWINCH SIGCONT,
// upper case, with or without the "SIG" prefix. Numbers, SIGKILL and
// SIGSTOP are refused: killing belongs to timeouts and the stop sweep,
// and a stopped child would wedge supervision.
// On success fills *signo and *canonical (always with the prefix).
bool fromName(const std::string& name, int* signo, std::string* canonical);

// "SIGHUP, SIGINT, ..." for error messages
std::string acceptedNames();

struct Spec {
  std::string job;   // name of the target job
  int signo = 0;
  std::string name;  // canonical signal name
  bool group = false;
  Duration wait{0};  // 0: the action finishes at delivery
};

// Parse a `signal` object. On error returns false, sets *key to the
// offending key path under `signal` ("", ".job", ".send", ".group",
// ".wait") and *err to the reason.
bool parseSpec(const Json& raw, Spec* out, std::string* key, std::string* err);

// kill(pid, sig), or kill(-pid, sig) for the process group. A pid <= 0
// means "no running process" and nothing is sent. Returns false and sets
// *reason when nothing was delivered.
bool deliver(pid_t pid, int signo, bool group, std::string* reason);

extern const char* kNoProcess;  // deliver()'s reason for a pid <= 0

}  // namespace signals
}  // namespace cpilot
