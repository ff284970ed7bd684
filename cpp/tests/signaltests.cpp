// Tests for signal jobs (cpilot/signals.hpp, the `signal` action in
// cpilot/jobs.hpp): the name table, the spec parser and the config rules
// including target resolution in newJobConfigs, and a Job with a signal
// action driven on a real Loop and Bus against a real child.
// Run via `bin/cpilot_signaltests`; exits non-zero if any check failed.
#include <signal.h>
#include <sys/epoll.h>
#include <sys/signalfd.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <sstream>
#include <string>
#include <vector>

#include "cpilot/events.hpp"
#include "cpilot/jobs.hpp"
#include "cpilot/json.hpp"
#include "cpilot/log.hpp"
#include "cpilot/loop.hpp"
#include "cpilot/signals.hpp"

using namespace cpilot;
using std::chrono::milliseconds;

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                         \
    }                                                                     \
  } while (0)
#define CHECK_EQ(a, b)                                                    \
  do {                                                                    \
    auto va = (a);                                                        \
    auto vb = (b);                                                        \
    if (!(va == vb)) {                                                    \
      fprintf(stderr, "FAIL %s:%d: %s != %s\n", __FILE__, __LINE__, #a,   \
              #b);                                                        \
      failures++;                                                         \
    }                                                                     \
  } while (0)

namespace {

// ---------------- name table ----------------

void testNameTable() {
  struct Row {
    const char* bare;
    int signo;
  };
  const Row rows[] = {{"HUP", SIGHUP},     {"INT", SIGINT},   {"QUIT", SIGQUIT},
                      {"TERM", SIGTERM},   {"USR1", SIGUSR1}, {"USR2", SIGUSR2},
                      {"WINCH", SIGWINCH}, {"CONT", SIGCONT}};
  for (const Row& row : rows) {
    for (std::string name : {std::string(row.bare),
                             std::string("SIG") + row.bare}) {
      int signo = 0;
      std::string canonical;
      CHECK(signals::fromName(name, &signo, &canonical));
      CHECK_EQ(signo, row.signo);
      CHECK_EQ(canonical, std::string("SIG") + row.bare);
    }
  }
  for (const char* bad : {"SIGKILL", "KILL", "SIGSTOP", "STOP", "1", "15", "",
                          "SIG", "sighup", "hup", "SigHup", "SIGSIGHUP",
                          "SIGHUP ", " SIGHUP", "SIGTSTP", "SIGRTMIN"}) {
    int signo = -5;
    std::string canonical = "untouched";
    CHECK(!signals::fromName(bad, &signo, &canonical));
    CHECK_EQ(signo, -5);
    CHECK_EQ(canonical, std::string("untouched"));
  }
  CHECK_EQ(signals::acceptedNames(),
           std::string("SIGHUP, SIGINT, SIGQUIT, SIGTERM, SIGUSR1, SIGUSR2, "
                       "SIGWINCH, SIGCONT"));
  // null outputs are allowed
  CHECK(signals::fromName("HUP", nullptr, nullptr));
}

// ---------------- spec parser ----------------

void testSpecParser() {
  signals::Spec spec;
  std::string key, err;
  CHECK(signals::parseSpec(parseJson5("{job: 'app', send: 'SIGHUP'}"), &spec,
                           &key, &err));
  CHECK_EQ(spec.job, std::string("app"));
  CHECK_EQ(spec.signo, SIGHUP);
  CHECK_EQ(spec.name, std::string("SIGHUP"));
  CHECK(!spec.group);
  CHECK(spec.wait == Duration(0));

  CHECK(signals::parseSpec(
      parseJson5("{job: 'app', send: 'QUIT', group: true, wait: '1500ms'}"),
      &spec, &key, &err));
  CHECK_EQ(spec.signo, SIGQUIT);
  CHECK_EQ(spec.name, std::string("SIGQUIT"));
  CHECK(spec.group);
  CHECK(spec.wait == Duration(milliseconds(1500)));
  // a bare number is seconds, as for stopTimeout
  CHECK(signals::parseSpec(parseJson5("{job: 'app', send: 'HUP', wait: 2}"),
                           &spec, &key, &err));
  CHECK(spec.wait == Duration(std::chrono::seconds(2)));

  auto bad = [](const std::string& json5, const std::string& wantKey,
                const std::string& wantErr, int line) {
    signals::Spec s;
    std::string k, e;
    bool ok = signals::parseSpec(parseJson5(json5), &s, &k, &e);
    if (ok || k != wantKey || e.find(wantErr) == std::string::npos) {
      fprintf(stderr, "FAIL %s:%d: %s -> %s key '%s' err '%s'\n", __FILE__,
              line, json5.c_str(), ok ? "accepted" : "refused", k.c_str(),
              e.c_str());
      failures++;
    }
  };
  const std::string names = signals::acceptedNames();
  bad("'SIGHUP'", "", "must be an object", __LINE__);
  bad("{job: 'app', send: 'HUP', pid: 3}", "", "invalid keys: pid", __LINE__);
  bad("{send: 'HUP'}", ".job", "must be the name of a job", __LINE__);
  bad("{job: '', send: 'HUP'}", ".job", "must be the name of a job", __LINE__);
  bad("{job: 3, send: 'HUP'}", ".job", "must be the name of a job", __LINE__);
  bad("{job: 'app'}", ".send", "is required: must be one of " + names,
      __LINE__);
  bad("{job: 'app', send: 'SIGKILL'}", ".send",
      "'SIGKILL' is not accepted: must be one of " + names, __LINE__);
  bad("{job: 'app', send: 'STOP'}", ".send", "'STOP' is not accepted",
      __LINE__);
  bad("{job: 'app', send: 1}", ".send", "'1' is not accepted", __LINE__);
  bad("{job: 'app', send: '1'}", ".send", "'1' is not accepted", __LINE__);
  bad("{job: 'app', send: 'sighup'}", ".send", "'sighup' is not accepted",
      __LINE__);
  bad("{job: 'app', send: 'HUP', group: 'maybe'}", ".group",
      "cannot parse 'group' as bool", __LINE__);
  bad("{job: 'app', send: 'HUP', wait: 'soon'}", ".wait", "'soon'", __LINE__);
  bad("{job: 'app', send: 'HUP', wait: 0}", ".wait",
      "'0' cannot be less than 1ms", __LINE__);
  bad("{job: 'app', send: 'HUP', wait: '999us'}", ".wait",
      "'999us' cannot be less than 1ms", __LINE__);
  bad("{job: 'app', send: 'HUP', wait: '-1s'}", ".wait",
      "cannot be less than 1ms", __LINE__);
}

// ---------------- config rules ----------------

const char* kTarget = "{name: 'app', exec: 'sleep 1'}, ";

bool jobsOk(const std::string& jobs, std::string* err,
            std::vector<std::shared_ptr<JobConfig>>* out = nullptr) {
  std::vector<std::shared_ptr<JobConfig>> cfgs;
  bool ok = newJobConfigs(parseJson5("[" + jobs + "]"), nullptr, &cfgs, err);
  if (out) *out = cfgs;
  return ok;
}

void expectRefused(const std::string& jobs, const std::string& want,
                   int line) {
  std::string err;
  if (jobsOk(jobs, &err) || err != want) {
    fprintf(stderr, "FAIL %s:%d: %s -> '%s', want '%s'\n", __FILE__, line,
            jobs.c_str(), err.c_str(), want.c_str());
    failures++;
  }
}
#define REFUSED(jobs, want) expectRefused(jobs, want, __LINE__)

void testConfigRules() {
  const std::string t = kTarget;
  std::string err;
  std::vector<std::shared_ptr<JobConfig>> cfgs;

  CHECK(jobsOk(t + "{name: 'r', signal: {job: 'app', send: 'SIGHUP'}, "
                   "when: {source: 'watch.b', each: 'changed'}}",
               &err, &cfgs));
  CHECK_EQ(cfgs.size(), (size_t)2);
  if (cfgs.size() == 2) {
    CHECK(cfgs[1]->signal != nullptr);
    CHECK(cfgs[1]->exec == nullptr);
    // wired to the target's own Command, not a copy
    CHECK(cfgs[1]->signal && cfgs[1]->signal->target == cfgs[0]->exec);
    CHECK(cfgs[0]->signal == nullptr);
    CHECK_EQ(cfgs[1]->restartLimit, 0);
  }
  // the target may come later in the list
  CHECK(jobsOk("{name: 'r', signal: {job: 'app', send: 'HUP'}}, " +
                   std::string("{name: 'app', exec: 'sleep 1'}"),
               &err, &cfgs));
  CHECK(cfgs.size() == 2 && cfgs[0]->signal->target == cfgs[1]->exec);
  // validated alone, the target stays unresolved
  std::shared_ptr<JobConfig> one;
  CHECK(validateJobConfig(
      parseJson5("{name: 'r', signal: {job: 'app', send: 'HUP'}}"), nullptr,
      &one, &err));
  CHECK(one && one->signal && one->signal->target == nullptr);

  // restarts: only with when.interval
  CHECK(jobsOk(t + "{name: 'r', signal: {job: 'app', send: 'HUP'}, "
                   "restarts: 'never'}", &err));
  CHECK(jobsOk(t + "{name: 'r', signal: {job: 'app', send: 'HUP'}, "
                   "restarts: 0}", &err));
  CHECK(jobsOk(t + "{name: 'r', signal: {job: 'app', send: 'HUP'}, "
                   "when: {interval: '1s'}, restarts: 3}", &err, &cfgs));
  CHECK(cfgs.size() == 2 && cfgs[1]->restartLimit == 3);
  CHECK(jobsOk(t + "{name: 'r', signal: {job: 'app', send: 'HUP'}, "
                   "when: {interval: '1s'}}", &err, &cfgs));
  CHECK(cfgs.size() == 2 && cfgs[1]->restartLimit == kUnlimited);
  CHECK(jobsOk(t + "{name: 'r', signal: {job: 'app', send: 'HUP'}, "
                   "when: {interval: '1s'}, restarts: 'unlimited'}", &err));
  REFUSED(t + "{name: 'r', signal: {job: 'app', send: 'HUP'}, restarts: 3}",
          "job[r].signal cannot be combined with restarts '3' unless "
          "'when.interval' is set");
  REFUSED(t + "{name: 'r', signal: {job: 'app', send: 'HUP'}, "
              "restarts: 'unlimited'}",
          "job[r].signal cannot be combined with restarts 'unlimited' unless "
          "'when.interval' is set");
  REFUSED(t + "{name: 'r', signal: {job: 'app', send: 'HUP'}, "
              "when: {source: 'app', each: 'healthy'}, restarts: 1}",
          "job[r].signal cannot be combined with restarts '1' unless "
          "'when.interval' is set");

  // stopTimeout and when keep their meaning
  CHECK(jobsOk(t + "{name: 'pre-stop', stopTimeout: '3s', "
                   "signal: {job: 'app', send: 'QUIT', wait: '10s'}, "
                   "when: {source: 'app', once: 'stopping'}}",
               &err, &cfgs));
  if (cfgs.size() == 2) {
    CHECK(cfgs[1]->stoppingTimeout == Duration(std::chrono::seconds(3)));
    CHECK(cfgs[1]->whenEvent == (Event{EventCode::Stopping, "app"}));
    CHECK(cfgs[0]->stoppingWaitEvent ==
          (Event{EventCode::Stopped, "pre-stop"}));
  }

  // exclusions
  REFUSED(t + "{name: 'r', exec: 'true', signal: {job: 'app', send: 'HUP'}}",
          "job[r].signal cannot be combined with 'exec'");
  for (std::string extra :
       {"port: 80", "health: {exec: 'true', interval: 1, ttl: 2}",
        "timeout: '1s'", "logging: {raw: true}"}) {
    std::string key = extra.substr(0, extra.find(':'));
    REFUSED(t + "{name: 'r', signal: {job: 'app', send: 'HUP'}, " + extra +
                "}",
            "job[r].signal cannot be combined with '" + key +
                "': a signal job starts no process");
  }

  // the spec's own errors carry the job[<name>].signal prefix
  REFUSED(t + "{name: 'r', signal: 'SIGHUP'}",
          "job[r].signal: must be an object");
  REFUSED(t + "{name: 'r', signal: {job: 'app', send: 'HUP', to: 1}}",
          "job[r].signal: invalid keys: to");
  REFUSED(t + "{name: 'r', signal: {job: 'app', send: 'SIGSTOP'}}",
          "job[r].signal.send 'SIGSTOP' is not accepted: must be one of " +
              signals::acceptedNames());
  REFUSED(t + "{name: 'r', signal: {job: 'app', send: 'HUP', wait: '0s'}}",
          "job[r].signal.wait '0s' cannot be less than 1ms");

  // target resolution
  REFUSED("{name: 'r', signal: {job: 'r', send: 'HUP'}}",
          "job[r].signal.job 'r' is the job itself");
  REFUSED(t + "{name: 'r', signal: {job: 'nginx', send: 'HUP'}}",
          "job[r].signal.job 'nginx' is not a job in this config");
  REFUSED(t + "{name: 'idle'}, {name: 'r', signal: {job: 'idle', "
              "send: 'HUP'}}",
          "job[r].signal.job 'idle' has no 'exec' to signal");
  REFUSED(t + "{name: 'r', signal: {job: 'app', send: 'HUP'}}, "
              "{name: 'rr', signal: {job: 'r', send: 'HUP'}}",
          "job[rr].signal.job 'r' has no 'exec' to signal");

  // a job without `signal` is parsed as before
  CHECK(jobsOk("{name: 'app', exec: 'sleep 1', signal: null}", &err, &cfgs));
  CHECK(cfgs.size() == 1 && cfgs[0]->signal == nullptr && cfgs[0]->exec);
}

// ---------------- deliver ----------------

void testDeliver() {
  std::string reason;
  CHECK(!signals::deliver(-1, SIGHUP, false, &reason));
  CHECK_EQ(reason, std::string(signals::kNoProcess));
  CHECK(!signals::deliver(0, SIGHUP, true, &reason));
  CHECK_EQ(reason, std::string(signals::kNoProcess));
  // a pid that cannot exist: kill(2) itself fails
  reason.clear();
  CHECK(!signals::deliver(0x7ffffff0, SIGCONT, false, &reason));
  CHECK_EQ(reason, std::string(strerror(ESRCH)));
  // SIGCONT to ourselves is harmless and goes through
  CHECK(signals::deliver(getpid(), SIGCONT, false, &reason));
}

// ---------------- a Job on a real Loop and Bus ----------------

std::string tmpDir;

std::string readAll(const std::string& path) {
  std::ifstream in(path);
  std::stringstream ss;
  ss << in.rdbuf();
  return ss.str();
}

struct Recorder : Subscriber {
  std::vector<Event> events;
  void onEvent(const Event& e) override { events.push_back(e); }
  int count(EventCode code, const std::string& source) const {
    int n = 0;
    for (auto& e : events)
      if (e.code == code && e.source == source) n++;
    return n;
  }
  int indexOf(EventCode code, const std::string& source) const {
    for (size_t i = 0; i < events.size(); i++)
      if (events[i].code == code && events[i].source == source) return (int)i;
    return -1;
  }
  // the Error event published right after events[i], or ""
  std::string errorAfter(int i) const {
    if (i < 0 || (size_t)i + 1 >= events.size() ||
        events[i + 1].code != EventCode::Error)
      return "";
    return events[i + 1].source;
  }
};

struct Rig {
  Loop loop;
  std::shared_ptr<Bus> bus = std::make_shared<Bus>(loop);
  Recorder rec;
  std::vector<std::shared_ptr<JobConfig>> cfgs;
  std::vector<std::shared_ptr<Job>> jobs;
  int sigfd = -1;

  explicit Rig(const std::string& jobsJson) {
    sigset_t mask;
    sigemptyset(&mask);
    sigaddset(&mask, SIGCHLD);
    sigprocmask(SIG_BLOCK, &mask, nullptr);
    sigfd = signalfd(-1, &mask, SFD_NONBLOCK | SFD_CLOEXEC);
    loop.watchFd(sigfd, EPOLLIN, [this](uint32_t) {
      struct signalfd_siginfo si;
      while (read(sigfd, &si, sizeof(si)) == sizeof(si)) {
      }
      loop.reapChildren();
    });
    bus->subscribe(&rec);
    std::string err;
    if (!newJobConfigs(parseJson5(jobsJson), nullptr, &cfgs, &err)) {
      fprintf(stderr, "job config error: %s\n", err.c_str());
      exit(1);
    }
    for (auto& cfg : cfgs) {
      jobs.push_back(std::make_shared<Job>(cfg));
      bus->subscribe(jobs.back().get());
    }
    for (auto& job : jobs) job->run(loop, bus, [] {});
    bus->publish(GlobalStartup);
  }

  ~Rig() {
    // leave no child behind, whatever the test did
    bus->shutdown();
    spin(5000, [this] { return allDone(); });
    for (auto& cfg : cfgs)
      if (cfg->exec && cfg->exec->running()) cfg->exec->kill();
    spin(2000, [this] { return allDone(); });
    CHECK(allDone());
    bus->unsubscribe(&rec);
    loop.unwatchFd(sigfd);
    close(sigfd);
  }

  bool allDone() const {
    for (auto& job : jobs)
      if (!job->isComplete()) return false;
    for (auto& cfg : cfgs)
      if (cfg->exec && cfg->exec->running()) return false;
    return true;
  }

  // run the loop until done() holds, for ms at the most; returns done()
  bool spin(int ms, std::function<bool()> done = nullptr) {
    uint64_t deadline = loop.addTimeout(milliseconds(ms), [&] { loop.stop(); });
    uint64_t poll = 0;
    if (done)
      poll = loop.addInterval(milliseconds(2), [&] {
        if (done()) loop.stop();
      });
    loop.run();
    loop.cancelTimer(deadline);
    if (poll) loop.cancelTimer(poll);
    return done ? done() : true;
  }

  void trigger() { bus->publish(Event{EventCode::StatusChanged, "watch.t"}); }
};

// A target that records signals: it writes `ready` once its traps are
// set, and polls in short sleeps so a trap runs within a few ms.
int targetSeq = 0;  // one `ready` file per target made

std::string readyFile(const std::string& name) {
  return tmpDir + "/" + name + "." + std::to_string(targetSeq) + ".ready";
}

std::string target(const std::string& name, const std::string& traps,
                   const std::string& rest = "") {
  targetSeq++;
  std::string script = traps + " echo ready > " + readyFile(name) +
                       "; while :; do sleep 0.02; done";
  return "{name: '" + name + "', exec: ['/bin/sh', '-c', \"" + script +
         "\"]" + rest + "}";
}

bool isReady(const std::string& name) {
  return !readAll(readyFile(name)).empty();
}

// The target (always the first job) can be signalled: its traps are set
// AND the spawner's completion has handed its pid to the Command. The
// child may well write `ready` first; until the pid has landed the launch
// is still in flight by the feature's own rule.
bool targetUp(const Rig& rig) {
  return isReady("app") && rig.cfgs[0]->exec->pid() > 0;
}

const char* kWhen = "when: {source: 'watch.t', each: 'changed'}";

void testDelivered() {
  std::string out = tmpDir + "/delivered.out";
  Rig rig("[" + target("app", "trap 'echo usr1 >> " + out + "' USR1;") +
          ", {name: 'sig', signal: {job: 'app', send: 'SIGUSR1'}, " + kWhen +
          "}]");
  CHECK(rig.spin(5000, [&] { return targetUp(rig); }));
  pid_t pid = rig.cfgs[0]->exec->pid();
  CHECK(pid > 0);
  rig.trigger();
  CHECK(rig.spin(5000, [&] { return readAll(out) == "usr1\n"; }));
  CHECK_EQ(rig.rec.count(EventCode::ExitSuccess, "sig"), 1);
  CHECK_EQ(rig.rec.count(EventCode::ExitFailed, "sig"), 0);
  // `each`: the job is still there for the next change
  CHECK(!rig.jobs[1]->isComplete());
  rig.trigger();
  CHECK(rig.spin(5000, [&] { return readAll(out) == "usr1\nusr1\n"; }));
  CHECK_EQ(rig.rec.count(EventCode::ExitSuccess, "sig"), 2);
  // the target was signalled, not replaced
  CHECK_EQ(rig.cfgs[0]->exec->pid(), pid);
  for (auto& e : rig.rec.events) CHECK(e.code != EventCode::Error);
}

void testNoPid() {
  // never started: its `when` never fires
  Rig rig("[{name: 'app', exec: 'sleep 30', "
          "when: {source: 'never', once: 'changed'}}, "
          "{name: 'sig', signal: {job: 'app', send: 'HUP'}, " +
          std::string(kWhen) + "}]");
  rig.trigger();
  CHECK(rig.spin(2000, [&] {
    return rig.rec.count(EventCode::ExitFailed, "sig") == 1 &&
           !rig.rec.errorAfter(rig.rec.indexOf(EventCode::ExitFailed, "sig"))
                .empty();
  }));
  CHECK_EQ(rig.rec.errorAfter(rig.rec.indexOf(EventCode::ExitFailed, "sig")),
           std::string("sig: SIGHUP not sent: job 'app' has no running "
                       "process"));
  CHECK_EQ(rig.rec.count(EventCode::ExitSuccess, "sig"), 0);
  CHECK(!rig.jobs[1]->isComplete());
}

void testNoPidAfterExit() {
  Rig rig("[{name: 'app', exec: 'true'}, "
          "{name: 'sig', signal: {job: 'app', send: 'HUP', wait: '5s'}, " +
          std::string(kWhen) + "}]");
  CHECK(rig.spin(5000, [&] {
    return rig.rec.count(EventCode::ExitSuccess, "app") == 1;
  }));
  rig.trigger();
  CHECK(rig.spin(2000, [&] {
    return rig.rec.count(EventCode::ExitFailed, "sig") == 1;
  }));
  rig.spin(30);
  // it failed at once: the `wait` never started
  CHECK_EQ(rig.rec.count(EventCode::ExitFailed, "sig"), 1);
  CHECK_EQ(rig.rec.count(EventCode::ExitSuccess, "sig"), 0);
}

void testWaitSatisfied() {
  // the target takes 150 ms to leave, and leaves with a failure: how it
  // exits does not matter
  Rig rig("[" + target("app", "trap 'sleep 0.15; exit 3' QUIT;") +
          ", {name: 'sig', signal: {job: 'app', send: 'QUIT', wait: '5s'}, " +
          kWhen + "}]");
  CHECK(rig.spin(5000, [&] { return targetUp(rig); }));
  rig.trigger();
  rig.trigger();  // arrives during the wait: ignored
  TimePoint t0 = Clock::now();
  CHECK(rig.spin(5000, [&] {
    return rig.rec.count(EventCode::ExitSuccess, "sig") == 1;
  }));
  CHECK(Clock::now() - t0 < milliseconds(3000));
  int iTarget = rig.rec.indexOf(EventCode::ExitFailed, "app");
  int iSig = rig.rec.indexOf(EventCode::ExitSuccess, "sig");
  CHECK(iTarget >= 0 && iTarget < iSig);
  rig.spin(50);
  CHECK_EQ(rig.rec.count(EventCode::ExitSuccess, "sig"), 1);
  CHECK_EQ(rig.rec.count(EventCode::ExitFailed, "sig"), 0);
}

void testWaitTimedOut() {
  Rig rig("[" + target("app", "trap '' QUIT;") +
          ", {name: 'sig', signal: {job: 'app', send: 'QUIT', wait: '100ms'}, " +
          kWhen + "}]");
  CHECK(rig.spin(5000, [&] { return targetUp(rig); }));
  TimePoint t0 = Clock::now();
  rig.trigger();
  CHECK(rig.spin(3000, [&] {
    return rig.rec.count(EventCode::ExitFailed, "sig") == 1;
  }));
  CHECK(Clock::now() - t0 >= milliseconds(100));
  CHECK_EQ(rig.rec.count(EventCode::ExitSuccess, "sig"), 0);
  // nothing was killed
  CHECK(rig.cfgs[0]->exec->pid() > 0);
  CHECK_EQ(rig.rec.count(EventCode::ExitFailed, "app"), 0);
  // and the job can go again
  rig.trigger();
  CHECK(rig.spin(3000, [&] {
    return rig.rec.count(EventCode::ExitFailed, "sig") == 2;
  }));
}

void testIgnoredStartsUseNoRestart() {
  // interval 60 ms, wait 150 ms: two ticks fall into every wait. They are
  // ignored and must not count against `restarts: 2`, so the job runs
  // three times (start-up + 2): each run ends in ExitFailed, either at
  // once (start-up: the launch is in flight) or when its wait runs out.
  Rig rig("[" + target("app", "trap '' QUIT;") +
          ", {name: 'sig', when: {interval: '60ms'}, restarts: 2, "
          "signal: {job: 'app', send: 'QUIT', wait: '150ms'}}]");
  CHECK(rig.spin(5000, [&] {
    return rig.rec.count(EventCode::Stopped, "sig") == 1;
  }));
  CHECK_EQ(rig.rec.count(EventCode::ExitFailed, "sig"), 3);
  CHECK_EQ(rig.rec.count(EventCode::ExitSuccess, "sig"), 0);
  CHECK(rig.cfgs[0]->exec->pid() > 0);
}

void testCleanupDuringWait() {
  Rig rig("[" + target("app", "trap '' QUIT;") +
          ", {name: 'sig', signal: {job: 'app', send: 'QUIT', wait: '400ms'}, " +
          kWhen + "}]");
  CHECK(rig.spin(5000, [&] { return targetUp(rig); }));
  rig.trigger();
  rig.spin(30);
  rig.bus->publish(Event{EventCode::Quit, "sig"});
  CHECK(rig.spin(2000, [&] { return rig.jobs[1]->isComplete(); }));
  CHECK_EQ(rig.rec.count(EventCode::Stopped, "sig"), 1);
  // past the wait: its timer was cancelled, so the finished job says
  // nothing more
  rig.spin(500);
  CHECK_EQ(rig.rec.count(EventCode::ExitFailed, "sig"), 0);
  CHECK_EQ(rig.rec.count(EventCode::ExitSuccess, "sig"), 0);
  CHECK(rig.cfgs[0]->exec->pid() > 0);
}

void testPreStopDrain() {
  // shutdown: Stopping{app} starts pre-stop, which asks app to drain and
  // waits; app leaves by itself (exit 0: it never saw a SIGTERM)
  std::string out = tmpDir + "/drain.out";
  Rig rig("[" +
          target("app",
                 "trap 'sleep 0.15; echo drained > " + out + "; exit 0' QUIT;",
                 ", stopTimeout: '5s'") +
          ", {name: 'pre-stop', "
          "signal: {job: 'app', send: 'SIGQUIT', wait: '5s'}, "
          "when: {source: 'app', once: 'stopping'}}]");
  CHECK(rig.spin(5000, [&] { return targetUp(rig); }));
  rig.bus->shutdown();
  CHECK(rig.spin(5000, [&] { return rig.allDone(); }));
  CHECK_EQ(readAll(out), std::string("drained\n"));
  int iStopping = rig.rec.indexOf(EventCode::Stopping, "app");
  int iExit = rig.rec.indexOf(EventCode::ExitSuccess, "app");
  int iPre = rig.rec.indexOf(EventCode::ExitSuccess, "pre-stop");
  int iPreStopped = rig.rec.indexOf(EventCode::Stopped, "pre-stop");
  int iStopped = rig.rec.indexOf(EventCode::Stopped, "app");
  CHECK(iStopping >= 0 && iStopping < iExit && iExit < iPre &&
        iPre < iPreStopped && iPreStopped < iStopped);
  CHECK_EQ(rig.rec.count(EventCode::ExitFailed, "app"), 0);
  CHECK_EQ(rig.rec.count(EventCode::ExitFailed, "pre-stop"), 0);
}

void testSubscription() {
  std::vector<std::shared_ptr<JobConfig>> cfgs;
  std::string err;
  CHECK(jobsOk(std::string(kTarget) +
                   "{name: 'a', signal: {job: 'app', send: 'HUP'}, " + kWhen +
                   "}, {name: 'b', signal: {job: 'app', send: 'HUP', "
                   "wait: '1s'}, " + kWhen + "}",
               &err, &cfgs));
  if (cfgs.size() != 3) return;
  auto has = [](const Subscription& sub, const std::string& source) {
    for (auto& s : sub.sources)
      if (s == source) return true;
    return false;
  };
  Subscription a = Job(cfgs[1]).subscription();
  Subscription b = Job(cfgs[2]).subscription();
  CHECK(!a.all && !has(a, "app"));  // as narrow as before
  CHECK(!b.all && has(b, "app"));
  CHECK_EQ(b.sources.size(), a.sources.size() + 1);
}

}  // namespace

int main() {
  logging::setLevel(logging::Level::Fatal);  // failures here are scripted
  char tmpl[] = "/tmp/cpilot-signaltests-XXXXXX";
  if (!mkdtemp(tmpl)) {
    perror("mkdtemp");
    return 1;
  }
  tmpDir = tmpl;

  testNameTable();
  testSpecParser();
  testConfigRules();
  testDeliver();
  testSubscription();
  testDelivered();
  testNoPid();
  testNoPidAfterExit();
  testWaitSatisfied();
  testWaitTimedOut();
  testIgnoredStartsUseNoRestart();
  testCleanupDuringWait();
  testPreStopDrain();

  std::string cleanup = "rm -rf '" + tmpDir + "'";
  if (system(cleanup.c_str()) != 0) perror("cleanup");

  if (failures) {
    fprintf(stderr, "%d signal test failure(s)\n", failures);
    return 1;
  }
  printf("all signal tests passed\n");
  return 0;
}
