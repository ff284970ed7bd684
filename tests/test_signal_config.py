"""Config rules of `jobs[].signal`, one row per rule: each refusal with its
message, each accepted spelling, and the name table behind
native.signal_number against Python's signal.Signals."""

import json
import signal

import pytest

from containerpilot_amd import native

ACCEPTED = ["SIGHUP", "SIGINT", "SIGQUIT", "SIGTERM", "SIGUSR1", "SIGUSR2",
            "SIGWINCH", "SIGCONT"]
NAMES = ", ".join(ACCEPTED)
TARGET = {"name": "nginx", "exec": "sleep 1"}


def validate(*jobs):
    config = {"consul": "localhost:8500", "jobs": list(jobs)}
    return native.validate_config(json.dumps(config))


def signal_job(spec=None, **extra):
    job = {"name": "reload",
           "signal": {"job": "nginx", "send": "SIGHUP"} if spec is None
           else spec}
    job.update(extra)
    return job


ACCEPTED_JOBS = [
    ("plain", signal_job()),
    ("bare name", signal_job({"job": "nginx", "send": "HUP"})),
    ("group", signal_job({"job": "nginx", "send": "USR1", "group": True})),
    ("group false", signal_job({"job": "nginx", "send": "USR1",
                                "group": False})),
    ("wait", signal_job({"job": "nginx", "send": "SIGQUIT", "wait": "10s"})),
    ("wait 1ms", signal_job({"job": "nginx", "send": "QUIT", "wait": "1ms"})),
    ("wait in seconds", signal_job({"job": "nginx", "send": "QUIT",
                                    "wait": 10})),
    ("when each", signal_job(when={"source": "watch.backend",
                                   "each": "changed"})),
    ("when once stopping", signal_job(when={"source": "nginx",
                                            "once": "stopping"})),
    ("when signal", signal_job(when={"source": "SIGHUP"})),
    ("stopTimeout", signal_job(stopTimeout="5s")),
    ("restarts never", signal_job(restarts="never")),
    ("restarts 0", signal_job(restarts=0)),
    ("restarts '0'", signal_job(restarts="0")),
    ("interval", signal_job(when={"interval": "1s"})),
    ("interval restarts", signal_job(when={"interval": "1s"}, restarts=3)),
    ("interval unlimited", signal_job(when={"interval": "1s"},
                                      restarts="unlimited")),
    ("exec null", signal_job(exec=None)),
] + [("send " + name, signal_job({"job": "nginx", "send": name}))
     for name in ACCEPTED] + [
    ("send " + name[3:], signal_job({"job": "nginx", "send": name[3:]}))
    for name in ACCEPTED]


@pytest.mark.parametrize("job", [j for _, j in ACCEPTED_JOBS],
                         ids=[i for i, _ in ACCEPTED_JOBS])
def test_accepted(job):
    assert validate(TARGET, job) is None
    # the target may also come after the job that signals it
    assert validate(job, TARGET) is None


def send_error(value):
    return ("job[reload].signal.send '%s' is not accepted: must be one of %s"
            % (value, NAMES))


def no_process(key):
    return ("job[reload].signal cannot be combined with '%s': a signal job "
            "starts no process" % key)


def restarts_error(value):
    return ("job[reload].signal cannot be combined with restarts '%s' unless "
            "'when.interval' is set" % value)


REFUSED_JOBS = [
    ("not an object", [TARGET, signal_job("SIGHUP")],
     "job[reload].signal: must be an object"),
    ("unknown key", [TARGET, signal_job({"job": "nginx", "send": "HUP",
                                         "pid": 1})],
     "job[reload].signal: invalid keys: pid"),
    ("no job", [TARGET, signal_job({"send": "HUP"})],
     "job[reload].signal.job must be the name of a job with an 'exec'"),
    ("no send", [TARGET, signal_job({"job": "nginx"})],
     "job[reload].signal.send is required: must be one of " + NAMES),
    ("SIGKILL", [TARGET, signal_job({"job": "nginx", "send": "SIGKILL"})],
     send_error("SIGKILL")),
    ("KILL", [TARGET, signal_job({"job": "nginx", "send": "KILL"})],
     send_error("KILL")),
    ("SIGSTOP", [TARGET, signal_job({"job": "nginx", "send": "SIGSTOP"})],
     send_error("SIGSTOP")),
    ("number", [TARGET, signal_job({"job": "nginx", "send": 1})],
     send_error("1")),
    ("number as text", [TARGET, signal_job({"job": "nginx", "send": "15"})],
     send_error("15")),
    ("lower case", [TARGET, signal_job({"job": "nginx", "send": "sighup"})],
     send_error("sighup")),
    ("bad group", [TARGET, signal_job({"job": "nginx", "send": "HUP",
                                       "group": "maybe"})],
     "job[reload].signal.group cannot parse 'group' as bool"),
    ("wait zero", [TARGET, signal_job({"job": "nginx", "send": "HUP",
                                       "wait": "0s"})],
     "job[reload].signal.wait '0s' cannot be less than 1ms"),
    ("wait below 1ms", [TARGET, signal_job({"job": "nginx", "send": "HUP",
                                            "wait": "999us"})],
     "job[reload].signal.wait '999us' cannot be less than 1ms"),
    ("with exec", [TARGET, signal_job(exec="true")],
     "job[reload].signal cannot be combined with 'exec'"),
    ("with port", [TARGET, signal_job(port=80)], no_process("port")),
    ("with health", [TARGET, signal_job(health={"exec": "true", "interval": 1,
                                                "ttl": 2})],
     no_process("health")),
    ("with timeout", [TARGET, signal_job(timeout="1s")],
     no_process("timeout")),
    ("with logging", [TARGET, signal_job(logging={"raw": True})],
     no_process("logging")),
    ("restarts", [TARGET, signal_job(restarts=3)], restarts_error("3")),
    ("restarts unlimited", [TARGET, signal_job(restarts="unlimited")],
     restarts_error("unlimited")),
    ("restarts with each", [TARGET, signal_job(
        restarts=1, when={"source": "nginx", "each": "healthy"})],
     restarts_error("1")),
    ("itself", [TARGET, signal_job({"job": "reload", "send": "HUP"})],
     "job[reload].signal.job 'reload' is the job itself"),
    ("unknown job", [TARGET, signal_job({"job": "apache", "send": "HUP"})],
     "job[reload].signal.job 'apache' is not a job in this config"),
    ("job without exec", [TARGET, {"name": "idle"},
                          signal_job({"job": "idle", "send": "HUP"})],
     "job[reload].signal.job 'idle' has no 'exec' to signal"),
    ("another signal job", [TARGET, {"name": "other",
                                     "signal": {"job": "nginx",
                                                "send": "HUP"}},
                            signal_job({"job": "other", "send": "HUP"})],
     "job[reload].signal.job 'other' has no 'exec' to signal"),
]


@pytest.mark.parametrize("jobs,message",
                         [(j, m) for _, j, m in REFUSED_JOBS],
                         ids=[i for i, _, _ in REFUSED_JOBS])
def test_refused(jobs, message):
    assert validate(*jobs) == "unable to parse jobs: " + message


def test_wait_that_does_not_parse():
    err = validate(TARGET, signal_job({"job": "nginx", "send": "HUP",
                                       "wait": "soon"}))
    assert err.startswith(
        "unable to parse jobs: job[reload].signal.wait 'soon': "), err


def test_telemetry_job_is_no_target():
    # the synthetic telemetry job has no process
    config = {"consul": "localhost:8500",
              "telemetry": {"port": 9090, "interfaces": ["static:127.0.0.1"]},
              "jobs": [signal_job({"job": "containerpilot", "send": "HUP"})]}
    assert native.validate_config(json.dumps(config)) == (
        "unable to parse jobs: job[reload].signal.job 'containerpilot' is "
        "not a job in this config")


@pytest.mark.parametrize("name", ACCEPTED)
def test_signal_number_matches_python(name):
    assert native.signal_number(name) == int(signal.Signals[name])
    assert native.signal_number(name[3:]) == int(signal.Signals[name])


@pytest.mark.parametrize("name", ["SIGKILL", "KILL", "SIGSTOP", "STOP", "9",
                                  "1", "", "SIG", "sighup", "hup", "SIGTSTP",
                                  "SIGSEGV", "SIGHUP ", "SIGSIGHUP"])
def test_signal_number_refuses(name):
    with pytest.raises(ValueError) as e:
        native.signal_number(name)
    assert str(e.value) == ("'%s' is not accepted: must be one of %s"
                            % (name, NAMES))
