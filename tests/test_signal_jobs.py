"""Signal jobs end to end (`jobs[].signal`, POST /v3/signal, `-signal`): the
daemon signals a process it supervises itself, on the reactor, without
launching a shell or a helper to do it.

Targets are tiny shell scripts that trap a signal and append to a file;
tests/fixtures/proxy.py reloads its upstream list on SIGHUP."""

import json
import os
import signal
import socket
import subprocess
import time
import urllib.request

from containerpilot_amd import BINARY

from test_watch_render import ONE, TWO, read_file, wait_until

HERE = os.path.dirname(os.path.abspath(__file__))
PROXY = os.path.join(HERE, "fixtures", "proxy.py")
UPSTREAMS = "{{ range .Services }}{{ .Address }}:{{ .Port }}\n{{ end }}"
# how long a signal that must NOT arrive is given to arrive
WINDOW_S = 0.3


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def lines(path):
    return (read_file(str(path)) or "").splitlines()


def trap_target(name, out, sig="USR1", on_signal=None, **extra):
    """A job that appends its pid to `<out>.ready` once its trap is set and
    then, on `sig`, appends its pid to `out` (or runs `on_signal`). It polls
    in short sleeps, so a trap runs within some 20 ms."""
    action = on_signal if on_signal is not None else "echo $$ >> %s" % out
    script = ("trap '%s' %s; echo $$ >> %s.ready; "
              "while :; do sleep 0.02; done" % (action, sig, out))
    job = {"name": name, "exec": ["/bin/sh", "-c", script]}
    job.update(extra)
    return job


def ready(out, count=1):
    return lambda: len(lines(str(out) + ".ready")) >= count


def wait_running(d, *jobs):
    """Wait until the daemon holds a pid for each of `jobs`. A child can
    write its `.ready` file before the daemon has been handed its pid; until
    then the launch is in flight and a signal for it is dropped. SIGCONT
    through the control socket is harmless and answers 200 only once every
    target has a process."""
    body = json.dumps({job: "SIGCONT" for job in jobs})
    assert wait_until(
        lambda: d.control("POST", "/v3/signal", body)[0] == 200), \
        d.log()[-3000:]


def base_config(jobs, consul="localhost:8500", **extra):
    config = {"consul": consul, "stopTimeout": 1,
              "logging": {"level": "DEBUG"}, "jobs": jobs}
    config.update(extra)
    return config


def finish(d, timeout=30):
    d.terminate()
    assert d.wait(timeout=timeout) == 0, d.log()[-3000:]


def upstreams(entries):
    rows = sorted(entries, key=lambda e: (e["Address"], e["Port"], e["ID"]))
    return ["%s:%d" % (e["Address"], e["Port"]) for e in rows]


def run_render_reload(daemon_factory, mock_consul, tmp_path, **kwargs):
    """A blocking watch renders the upstream file and a signal job SIGHUPs
    the proxy: after each of three changes the proxy, which reads the file
    only on SIGHUP, must serve exactly that set. Returns the daemon."""
    source = tmp_path / "upstreams.ctmpl"
    source.write_text(UPSTREAMS)
    dest = str(tmp_path / "upstreams.conf")
    port = free_port()
    mock_consul.set_health("backend", [])
    d = daemon_factory(base_config([
        {"name": "nginx", "exec": [PROXY, str(port), dest]},
        {"name": "onchange-backend",
         "signal": {"job": "nginx", "send": "SIGHUP"},
         "when": {"source": "watch.backend", "each": "changed"}},
    ], consul=mock_consul.address, watches=[
        {"name": "backend", "interval": 30, "blocking": True,
         "render": {"source": str(source), "dest": dest}}]),
        **kwargs).start()
    d.wait_for_socket()

    def proxy_state():
        try:
            with urllib.request.urlopen("http://127.0.0.1:%d/" % port,
                                        timeout=2) as resp:
                return json.load(resp)
        except (OSError, ValueError):
            return None

    # serving means its SIGHUP handler is installed; the first result (the
    # empty set) is rendered without a change event
    assert wait_until(lambda: proxy_state() is not None), d.log()[-3000:]
    wait_running(d, "nginx")
    assert wait_until(lambda: read_file(dest) is not None), d.log()[-3000:]
    assert proxy_state()["reloads"] == 1

    for n, entries in enumerate([ONE, TWO, []], start=1):
        mock_consul.set_health("backend", entries)
        assert wait_until(lambda: proxy_state()["reloads"] >= 1 + n), \
            (n, proxy_state(), d.log()[-3000:])
        # one reload per change, and it read the file of exactly this set:
        # a signal sent before the rendering would have loaded the old one
        state = proxy_state()
        assert state == {"upstreams": upstreams(entries), "reloads": 1 + n}, \
            (n, state, d.log()[-3000:])
    log = d.log()
    assert log.count("onchange-backend: sent SIGHUP to job nginx at pid") == 3
    assert log.count("{ExitSuccess onchange-backend}") == 3
    assert "{Error" not in log
    return d


def test_render_then_reload_without_a_launch(daemon_factory, mock_consul,
                                             tmp_path):
    d = run_render_reload(daemon_factory, mock_consul, tmp_path)
    log = d.log()
    # nothing was launched for the reloads
    assert "nginx.Run start" in log
    assert "onchange-backend.Run start" not in log
    finish(d)


def test_target_without_a_running_process(daemon_factory, tmp_path):
    # `never`: its `when` never fires. `gone`: it has exited by the time
    # its own exit event starts the signal job.
    d = daemon_factory(base_config([
        {"name": "main-app", "exec": "sleep 60"},
        {"name": "never", "exec": "sleep 60",
         "when": {"source": "nobody", "once": "healthy"}},
        {"name": "gone", "exec": "true"},
        {"name": "sig-never", "signal": {"job": "never", "send": "HUP"},
         "when": {"source": "gone", "once": "exitSuccess"}},
        {"name": "sig-gone",
         "signal": {"job": "gone", "send": "SIGUSR1", "wait": "5s"},
         "when": {"source": "gone", "once": "exitSuccess"}},
    ])).start()
    d.wait_for_socket()
    assert wait_until(lambda: "{ExitFailed sig-never}" in d.log() and
                      "{ExitFailed sig-gone}" in d.log()), d.log()
    assert wait_until(lambda: "{Stopped sig-gone}" in d.log()), d.log()
    log = d.log()
    for name, sig, target in (("sig-never", "SIGHUP", "never"),
                              ("sig-gone", "SIGUSR1", "gone")):
        reason = "%s: %s not sent: job '%s' has no running process" % (
            name, sig, target)
        assert "{Error %s}" % reason in log, log
        # published right after the ExitFailed, and logged once as a warning
        assert log.index("{ExitFailed %s}" % name) < \
            log.index("{Error %s}" % reason)
        assert len([ln for ln in log.splitlines()
                    if reason in ln and "event:" not in ln]) == 1, log
    assert "{ExitSuccess sig-" not in log
    status, _ = d.control("GET", "/v3/ping")
    assert status == 200
    finish(d)


def drain_config(tmp_path, on_quit, wait):
    out = tmp_path / "app.out"
    return out, base_config([
        trap_target("app", out, sig="QUIT", on_signal=on_quit,
                    stopTimeout="5s"),
        {"name": "pre-stop",
         "signal": {"job": "app", "send": "SIGQUIT", "wait": wait},
         "when": {"source": "app", "once": "stopping"}},
    ])


def test_drain_that_finishes(daemon_factory, tmp_path):
    drained = tmp_path / "drained"
    out, config = drain_config(
        tmp_path, "sleep 0.3; echo drained > %s; exit 0" % drained, "5s")
    d = daemon_factory(config).start()
    d.wait_for_socket()
    assert wait_until(ready(out)), d.log()
    wait_running(d, "app")
    t0 = time.monotonic()
    d.terminate()
    assert d.wait(timeout=30) == 0, d.log()[-3000:]
    # well inside the wait: the chain moved on when the target left
    assert time.monotonic() - t0 < 4
    assert lines(drained) == ["drained"]
    log = d.log()
    assert "terminating command 'app'" not in log
    order = [log.index(text) for text in (
        "{Stopping app}", "pre-stop: sent SIGQUIT to job app at pid",
        "{ExitSuccess app}", "{ExitSuccess pre-stop}", "{Stopped pre-stop}",
        "{Stopped app}")]
    assert order == sorted(order), log
    assert "{ExitFailed" not in log


def test_drain_that_times_out(daemon_factory, tmp_path):
    out, config = drain_config(tmp_path, "", "300ms")  # QUIT is ignored
    d = daemon_factory(config).start()
    d.wait_for_socket()
    assert wait_until(ready(out)), d.log()
    wait_running(d, "app")
    t0 = time.monotonic()
    d.terminate()
    assert d.wait(timeout=30) == 0, d.log()[-3000:]
    assert time.monotonic() - t0 < 5  # the target's stopTimeout
    log = d.log()
    order = [log.index(text) for text in (
        "pre-stop: sent SIGQUIT to job app at pid", "{ExitFailed pre-stop}",
        "{Stopped pre-stop}", "terminating command 'app'", "{Stopped app}")]
    assert order == sorted(order), log
    assert "{ExitSuccess pre-stop}" not in log


def group_target(name, tmp_path):
    """A shell that records USR1 itself and has a child, in its process
    group, that records USR1 too."""
    parent_out = tmp_path / (name + ".parent")
    child_out = tmp_path / (name + ".child")
    child = tmp_path / (name + "-child.sh")
    child.write_text("trap 'echo usr1 >> %s' USR1\necho $$ >> %s.ready\n"
                     "while :; do sleep 0.02; done\n"
                     % (child_out, child_out))
    script = ("trap 'echo usr1 >> %s' USR1; /bin/sh %s & "
              "while :; do sleep 0.02; done" % (parent_out, child))
    return ({"name": name, "exec": ["/bin/sh", "-c", script]},
            parent_out, child_out)


def test_group_reaches_the_targets_children(daemon_factory, tmp_path):
    grouped, grouped_parent, grouped_child = group_target("grouped", tmp_path)
    single, single_parent, single_child = group_target("single", tmp_path)
    d = daemon_factory(base_config([
        grouped, single,
        {"name": "sig-grouped", "when": {"source": "SIGUSR2"},
         "signal": {"job": "grouped", "send": "USR1", "group": True}},
        {"name": "sig-single", "when": {"source": "SIGUSR2"},
         "signal": {"job": "single", "send": "USR1", "group": False}},
    ])).start()
    d.wait_for_socket()
    assert wait_until(lambda: ready(grouped_child)() and
                      ready(single_child)()), d.log()
    wait_running(d, "grouped", "single")
    d.signal(signal.SIGUSR2)
    # both parents have handled theirs: both deliveries are done
    assert wait_until(lambda: lines(grouped_parent) == ["usr1"] and
                      lines(single_parent) == ["usr1"]), d.log()
    assert wait_until(lambda: lines(grouped_child) == ["usr1"]), d.log()
    time.sleep(WINDOW_S)
    assert lines(single_child) == []
    assert lines(grouped_child) == ["usr1"]
    assert "(process group)" in d.log()
    finish(d)


def test_forwarding_a_daemon_signal(daemon_factory, tmp_path):
    out = tmp_path / "app.out"
    d = daemon_factory(base_config([
        trap_target("app", out, sig="USR1"),
        {"name": "forward-hup", "when": {"source": "SIGHUP"},
         "signal": {"job": "app", "send": "SIGUSR1"}},
    ])).start()
    d.wait_for_socket()
    assert wait_until(ready(out)), d.log()
    wait_running(d, "app")
    pid = lines(str(out) + ".ready")[0]
    for n in (1, 2):
        d.signal(signal.SIGHUP)
        assert wait_until(lambda: lines(out) == [pid] * n), (n, d.log())
    assert d.log().count("{ExitSuccess forward-hup}") == 2
    finish(d)


def test_interval_with_restarts_runs_as_often_as_an_exec_job(daemon_factory,
                                                             tmp_path):
    """The exec job is the only way there was: a shell that runs `kill`
    with the pid variable. Both jobs have the same `when` and `restarts`,
    so they run, deliver and fail equally often: the start-up run finds the
    target's launch still in flight (no pid, no pid variable), and the
    three restarts deliver."""
    out = tmp_path / "app.out"
    when = {"interval": "200ms"}
    d = daemon_factory(base_config([
        trap_target("app", out, sig="USR1"),
        {"name": "tick-exec", "when": when, "restarts": 3,
         "exec": ["/bin/sh", "-c", "kill -USR1 $CONTAINERPILOT_APP_PID"]},
        {"name": "tick-signal", "when": when, "restarts": 3,
         "signal": {"job": "app", "send": "SIGUSR1"}},
    ])).start()
    d.wait_for_socket()
    assert wait_until(lambda: "{Stopped tick-exec}" in d.log() and
                      "{Stopped tick-signal}" in d.log()), d.log()[-3000:]
    log = d.log()
    counts = {}
    for name in ("tick-exec", "tick-signal"):
        counts[name] = (log.count("event: {ExitSuccess %s}" % name),
                        log.count("event: {ExitFailed %s}" % name))
    print("runs (delivered, failed): %s" % counts)
    assert counts["tick-signal"] == counts["tick-exec"], log
    assert sum(counts["tick-exec"]) == 4  # the start-up run and 3 restarts
    assert counts["tick-signal"][0] == 3
    assert log.count("tick-signal: sent SIGUSR1 to job app") == 3
    assert lines(out), "no signal reached the target"
    finish(d)


def test_reloaded_config_signals_the_new_process(daemon_factory, tmp_path):
    out = tmp_path / "app.out"
    d = daemon_factory(base_config([
        trap_target("app", out, sig="USR1"),
        {"name": "poke", "when": {"source": "SIGUSR2"},
         "signal": {"job": "app", "send": "SIGUSR1"}},
    ])).start()
    d.wait_for_socket()
    assert wait_until(ready(out)), d.log()
    wait_running(d, "app")
    first = lines(str(out) + ".ready")[0]
    d.signal(signal.SIGUSR2)
    assert wait_until(lambda: lines(out) == [first]), d.log()

    status, _ = d.control("POST", "/v3/reload")
    assert status == 200
    assert wait_until(ready(out, count=2)), d.log()[-3000:]
    d.wait_for_socket(timeout=15)
    wait_running(d, "app")
    second = lines(str(out) + ".ready")[1]
    assert second != first
    d.signal(signal.SIGUSR2)
    assert wait_until(lambda: lines(out) == [first, second]), d.log()[-3000:]
    assert "poke: sent SIGUSR1 to job app at pid %s" % second in d.log()
    finish(d)


def cli(d, *args):
    return subprocess.run([BINARY, "-config", d.config_path, *args],
                          capture_output=True, text=True, timeout=30)


def test_control_endpoint_and_flag(daemon_factory, tmp_path):
    one, two = tmp_path / "one.out", tmp_path / "two.out"
    d = daemon_factory(base_config([
        trap_target("one", one, sig="USR1"),
        trap_target("two", two, sig="HUP"),
        {"name": "gone", "exec": "true"},
        {"name": "idle", "when": {"source": "nobody", "once": "healthy"}},
        {"name": "poke", "when": {"source": "nobody", "once": "healthy"},
         "signal": {"job": "one", "send": "USR1"}},
    ])).start()
    d.wait_for_socket()
    assert wait_until(lambda: ready(one)() and ready(two)() and
                      "{ExitSuccess gone}" in d.log()), d.log()
    wait_running(d, "one", "two")
    pid_one = lines(str(one) + ".ready")[0]
    pid_two = lines(str(two) + ".ready")[0]

    def post(body):
        return d.control("POST", "/v3/signal", json.dumps(body)
                         if not isinstance(body, str) else body)

    # 200 with delivery
    assert post({"one": "SIGUSR1"}) == (200, "\n")
    assert wait_until(lambda: lines(one) == [pid_one]), d.log()
    assert "control: sent SIGUSR1 to job one at pid %s" % pid_one in d.log()

    # two flags in one call
    result = cli(d, "-signal", "one=USR1", "-signal", "two=SIGHUP")
    assert result.returncode == 0, result.stderr
    assert wait_until(lambda: lines(one) == [pid_one] * 2 and
                      lines(two) == [pid_two]), d.log()

    # 405
    status, body = d.control("GET", "/v3/signal")
    assert (status, body) == (405, "Method Not Allowed\n")

    # each 422: nothing is delivered to anyone, not even to the valid entry
    for body in ("not json", "[]", '"SIGHUP"', {"one": 10}, {"one": ["USR1"]},
                 {"one": "USR1", "nobody": "HUP"},      # unknown job
                 {"one": "USR1", "idle": "HUP"},        # no exec
                 {"one": "USR1", "poke": "HUP"},        # a signal job
                 {"one": "USR1", "two": "SIGKILL"},     # refused signals
                 {"one": "USR1", "two": "SIGSTOP"},
                 {"one": "USR1", "two": "1"},
                 {"one": "USR1", "two": "hup"}):
        status, text = post(body)
        assert (status, text) == (422, "Unprocessable Entity\n"), body
    result = cli(d, "-signal", "nobody=HUP")
    assert result.returncode == 1
    assert result.stderr == \
        "-signal: failed to run subcommand: HTTP 422\n"
    time.sleep(WINDOW_S)
    assert lines(one) == [pid_one] * 2
    assert lines(two) == [pid_two]

    # 409: the stopped target gets nothing, the other entry gets its signal
    status, text = post({"gone": "HUP", "one": "USR1"})
    assert (status, text) == (409, "Conflict\n")
    assert wait_until(lambda: lines(one) == [pid_one] * 3), d.log()
    assert "control: SIGHUP not sent to job gone: no running process" \
        in d.log()
    assert lines(two) == [pid_two]

    # still serving, and nothing here went through a job
    status, _ = d.control("GET", "/v3/ping")
    assert status == 200
    assert "{ExitSuccess poke}" not in d.log()
    finish(d)


def test_usage_lists_the_flag():
    result = subprocess.run([BINARY, "-help"], capture_output=True, text=True,
                            timeout=30)
    assert result.returncode == 2
    assert "  -signal value\n" in result.stderr
