"""Http jobs end to end (`jobs[].http`): the daemon makes the request on its
reactor, without launching a `curl` to do it, and the job walks the state
machine as an exec job does whose process runs for the duration of the
request.

The peer is a recording `ThreadingHTTPServer` in this file; what a path does
is decided by its first segment (`/ok`, `/fail`, `/slow`, `/hang`, ...)."""

import http.server
import json
import signal
import socket
import threading
import time

import pytest

from containerpilot_amd import native

from test_watch_render import ONE, read_file, wait_until

UPSTREAMS = "{{ range .Services }}{{ .Address }}:{{ .Port }}\n{{ end }}"


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


class Recording(http.server.ThreadingHTTPServer):
    daemon_threads = True
    request_queue_size = 64

    def __init__(self):
        super().__init__(("127.0.0.1", 0), Handler)
        self.port = self.server_address[1]
        self.lock = threading.Lock()
        self.requests = []      # dicts, in order of arrival
        self.release = threading.Event()  # lets go of /hang and /slow
        self.slow_s = 0.4
        self.on_request = None  # called with the recorded dict

    def url(self, path):
        return "http://127.0.0.1:%d%s" % (self.port, path)

    def seen(self, path=None):
        with self.lock:
            return [r for r in self.requests
                    if path is None or r["path"] == path]


class Handler(http.server.BaseHTTPRequestHandler):
    protocol_version = "HTTP/1.1"

    def log_message(self, *args):
        pass

    def handle_any(self):
        length = int(self.headers.get("Content-Length") or 0)
        seen = {"method": self.command, "path": self.path,
                "headers": self.headers.items(),
                "body": self.rfile.read(length), "at": time.monotonic()}
        if self.server.on_request:
            self.server.on_request(seen)
        with self.server.lock:
            self.server.requests.append(seen)
        kind = self.path.split("?")[0].split("/")[1]
        if kind == "hang":
            self.server.release.wait(30)
            return
        if kind in ("slow", "drain"):
            self.server.release.wait(self.server.slow_s)
        seen["answered"] = time.time()
        seen["waited"] = time.monotonic() - seen["at"]
        status = 503 if kind == "fail" else 200
        body = b"done\n"
        self.send_response(status)
        self.send_header("Content-Type", "text/plain")
        self.send_header("Content-Length", str(len(body)))
        self.end_headers()
        if self.command != "HEAD":
            self.wfile.write(body)

    do_GET = do_HEAD = do_POST = do_PUT = do_PATCH = do_DELETE = handle_any


@pytest.fixture
def server():
    srv = Recording()
    thread = threading.Thread(target=srv.serve_forever, daemon=True,
                              kwargs={"poll_interval": 0.05})
    thread.start()
    yield srv
    srv.release.set()
    srv.shutdown()
    srv.server_close()


# the `text` log format names each line's level
TEXT_LOG = {"level": "DEBUG", "format": "text"}


def base_config(jobs, consul="localhost:8500", **extra):
    config = {"consul": consul, "stopTimeout": 1,
              "logging": {"level": "DEBUG"}, "jobs": jobs}
    config.update(extra)
    return config


def finish(d, timeout=30):
    d.terminate()
    assert d.wait(timeout=timeout) == 0, d.log()[-3000:]


def said(log, text):
    """Log lines that hold `text` and are not the bus's own event trace."""
    return [ln for ln in log.splitlines() if text in ln and "event:" not in ln]


def test_the_server_gets_the_request_exactly(daemon_factory, server):
    body = "{\"grace\": 10, \"why\": \"grüße\"}"
    url = server.url("/ok/drain?now=1&x=a%20b")
    d = daemon_factory(base_config([
        {"name": "main-app", "exec": "sleep 60"},
        {"name": "act",
         "http": {"url": url, "method": "POST",
                  "headers": {"Content-Type": "application/json",
                              "X-Token": "s3cret", "accept": "text/plain"},
                  "body": body}},
        {"name": "poke", "http": server.url("/ok/poke")},
    ], logging=TEXT_LOG)).start()
    d.wait_for_socket()
    assert wait_until(lambda: "{ExitSuccess act}" in d.log() and
                      "{ExitSuccess poke}" in d.log()), d.log()[-3000:]
    (got,) = server.seen("/ok/drain?now=1&x=a%20b")
    assert got["method"] == "POST"
    assert got["body"] == body.encode()
    assert got["headers"] == [
        ("Host", "127.0.0.1:%d" % server.port),
        ("User-Agent", "containerpilot/" + native.version()),
        ("Accept", "*/*"),
        ("Connection", "close"),
        ("Content-Length", str(len(body.encode()))),
        ("Content-Type", "application/json"),
        ("X-Token", "s3cret"),
        ("accept", "text/plain"),
    ]
    (poke,) = server.seen("/ok/poke")
    assert poke["method"] == "GET" and poke["body"] == b""
    assert [k for k, _ in poke["headers"]] == \
        ["Host", "User-Agent", "Accept", "Connection"]
    log = d.log()
    # one INFO line per request: job, method, URL as configured, status
    (line,) = said(log, "act: POST %s answered 200" % url)
    assert " level=info " in line, line
    assert len(said(log, "poke: GET %s answered 200"
                    % server.url("/ok/poke"))) == 1, log
    # no start limit left and no restarts: the jobs are done
    assert wait_until(lambda: "{Stopped act}" in d.log()), d.log()[-3000:]
    assert "act.Run start" not in log  # nothing was launched
    assert "{ExitFailed" not in log and "{Error" not in log
    status, text = d.control("GET", "/v3/ping")
    assert status == 200
    finish(d)


def test_failures_publish_exit_failed_and_error(daemon_factory, server):
    closed = free_port()
    d = daemon_factory(base_config([
        {"name": "main-app", "exec": "sleep 60"},
        {"name": "bad", "http": server.url("/fail")},
        {"name": "nobody", "http": "http://127.0.0.1:%d/" % closed},
        {"name": "picky", "http": {"url": server.url("/ok"), "expect": 204}},
        {"name": "alarm", "http": {"url": server.url("/ok/alarm"),
                                   "method": "POST", "body": "bad failed"},
         "when": {"source": "bad", "each": "exitFailed"}},
    ], logging=TEXT_LOG)).start()
    d.wait_for_socket()
    assert wait_until(lambda: all(
        "{ExitFailed %s}" % name in d.log()
        for name in ("bad", "nobody", "picky")) and
        "{ExitSuccess alarm}" in d.log()), d.log()[-3000:]
    log = d.log()
    for name, reason in (("bad", "unexpected status 503"),
                         ("nobody", "Connection refused"),
                         ("picky", "unexpected status 200")):
        error = "{Error %s: %s}" % (name, reason)
        assert error in log, log
        assert log.index("{ExitFailed %s}" % name) < log.index(error)
        # one WARN line
        (line,) = said(log, "%s: %s" % (name, reason))
        assert " level=warning " in line, line
        assert "{ExitSuccess %s}" % name not in log
    # the reference's own periodic-tasks example: an alarm on a failure
    (alarm,) = server.seen("/ok/alarm")
    assert alarm["body"] == b"bad failed"
    finish(d)


def test_timeout_is_the_deadline_of_the_request(daemon_factory, server):
    d = daemon_factory(base_config([
        {"name": "main-app", "exec": "sleep 60"},
        {"name": "stuck", "http": server.url("/hang"), "timeout": "300ms"},
    ], logging=TEXT_LOG)).start()
    d.wait_for_socket()
    assert wait_until(lambda: "{ExitFailed stuck}" in d.log()), \
        d.log()[-3000:]
    assert wait_until(lambda: "{Stopped stuck}" in d.log()), d.log()[-3000:]
    log = d.log()
    assert "{Error stuck: timeout after 300ms}" in log
    (line,) = said(log, "stuck: timeout after 300ms")
    assert " level=warning " in line, line
    assert len(server.seen("/hang")) == 1
    finish(d)


def test_render_then_reload_over_http(daemon_factory, mock_consul, tmp_path,
                                      server):
    """The watch renders the file before it publishes the change, so the
    server's handler finds the new rendering in place when the request
    arrives."""
    source = tmp_path / "upstreams.ctmpl"
    source.write_text(UPSTREAMS)
    dest = str(tmp_path / "upstreams.conf")
    found = []
    server.on_request = lambda seen: found.append(read_file(dest))
    mock_consul.set_health("backend", [])
    d = daemon_factory(base_config([
        {"name": "main-app", "exec": "sleep 60"},
        {"name": "reload",
         "http": {"url": server.url("/ok/-/reload"), "method": "POST"},
         "when": {"source": "watch.backend", "each": "changed"}},
    ], consul=mock_consul.address, watches=[
        {"name": "backend", "interval": 30, "blocking": True,
         "render": {"source": str(source), "dest": dest}}])).start()
    d.wait_for_socket()
    # the first result (the empty set) is rendered without a change event
    assert wait_until(lambda: read_file(dest) == ""), d.log()[-3000:]
    assert found == []
    mock_consul.set_health("backend", ONE)
    assert wait_until(lambda: len(found) == 1), d.log()[-3000:]
    assert found == ["10.0.0.1:9000\n"]
    mock_consul.set_health("backend", [])
    assert wait_until(lambda: len(found) == 2), d.log()[-3000:]
    assert found == ["10.0.0.1:9000\n", ""]
    assert wait_until(lambda: d.log().count("{ExitSuccess reload}") == 2)
    (first, second) = server.seen("/ok/-/reload")
    assert first["method"] == "POST" and first["body"] == b""
    assert ("Content-Length", "0") in first["headers"]
    assert "reload.Run start" not in d.log()
    finish(d)


def test_pre_stop_drain(daemon_factory, tmp_path, server):
    """On SIGTERM the server gets /drain and answers after 300 ms; only
    then does the app get its SIGTERM."""
    out = tmp_path / "app.term"
    server.slow_s = 0.3
    script = ("trap 'date +%%s.%%N > %s; exit 0' TERM; echo up > %s.ready; "
              "while :; do sleep 0.02; done" % (out, out))
    d = daemon_factory(base_config([
        {"name": "app", "exec": ["/bin/sh", "-c", script],
         "stopTimeout": "5s"},
        {"name": "pre-stop",
         "http": {"url": server.url("/drain"), "method": "POST",
                  "headers": {"Content-Type": "application/json"},
                  "body": "{\"grace\": 10}", "expect": [200, 202]},
         "timeout": "5s", "when": {"source": "app", "once": "stopping"}},
    ])).start()
    d.wait_for_socket()
    assert wait_until(lambda: read_file(str(out) + ".ready")), d.log()
    assert server.seen() == []
    t0 = time.monotonic()
    d.terminate()
    assert d.wait(timeout=30) == 0, d.log()[-3000:]
    assert time.monotonic() - t0 < 4
    (drain,) = server.seen("/drain")
    assert drain["body"] == b"{\"grace\": 10}"
    assert drain["at"] - t0 < 1.0
    # the app was terminated, and only after the drain was answered
    termed = float(read_file(str(out)))
    print("drain answered %.3f s before the app's SIGTERM"
          % (termed - drain["answered"]))
    assert termed >= drain["answered"]
    assert drain["waited"] >= 0.29
    log = d.log()
    order = [log.index(text) for text in (
        "{Stopping app}", "{ExitSuccess pre-stop}", "{Stopped pre-stop}",
        "terminating command 'app'", "{Stopped app}")]
    assert order == sorted(order), log
    assert "{ExitFailed pre-stop}" not in log


def test_reload_with_a_request_in_flight(daemon_factory, server):
    """The request's deadline is 4 s; the reload must be through within 1 s.
    That the cancelled request's timer says nothing once its deadline has
    passed is checked in the native tests, which can spin past it without
    making this suite wait."""
    d = daemon_factory(base_config([
        {"name": "main-app", "exec": "echo generation-up; sleep 60"},
        {"name": "stuck", "http": server.url("/hang"), "timeout": "4s",
         "when": {"source": "SIGUSR2"}},
    ])).start()
    d.wait_for_socket()
    assert wait_until(lambda: "generation-up" in d.log()), d.log()
    d.signal(signal.SIGUSR2)
    assert wait_until(lambda: len(server.seen("/hang")) == 1), d.log()
    t0 = time.monotonic()
    status, _ = d.control("POST", "/v3/reload")
    assert status == 200
    assert wait_until(lambda: d.log().count("generation-up") == 2,
                      timeout=5), d.log()[-3000:]
    took = time.monotonic() - t0
    print("reload with a request in flight took %.3f s" % took)
    assert took < 1.0
    d.wait_for_socket(timeout=15)
    log = d.log()
    assert len(said(log, "stuck canceled in flight")) == 1, log
    after = log[log.index("stuck canceled in flight"):]
    assert "{ExitFailed stuck}" not in log and "{ExitSuccess stuck}" not in log
    assert "stuck: " not in after, after
    # the new generation's job works
    d.signal(signal.SIGUSR2)
    assert wait_until(lambda: len(server.seen("/hang")) == 2), d.log()[-3000:]
    finish(d)
    assert "timeout after" not in d.log()


def test_a_start_during_a_slow_request_is_ignored(daemon_factory, server):
    server.slow_s = 0.5
    d = daemon_factory(base_config([
        {"name": "main-app", "exec": "sleep 60"},
        {"name": "slow", "http": server.url("/slow"),
         "when": {"source": "SIGUSR2"}},
    ])).start()
    d.wait_for_socket()
    d.signal(signal.SIGUSR2)
    assert wait_until(lambda: len(server.seen("/slow")) == 1), d.log()
    d.signal(signal.SIGUSR2)
    assert wait_until(lambda: "slow: start ignored, request still in flight"
                      in d.log()), d.log()[-3000:]
    assert wait_until(lambda: "{ExitSuccess slow}" in d.log()), \
        d.log()[-3000:]
    assert len(server.seen("/slow")) == 1
    assert d.log().count("{ExitSuccess slow}") == 1
    # and the job is still there for the next one
    d.signal(signal.SIGUSR2)
    assert wait_until(lambda: len(server.seen("/slow")) == 2), d.log()[-3000:]
    server.release.set()
    assert wait_until(lambda: d.log().count("{ExitSuccess slow}") == 2)
    finish(d)


def test_status_lists_the_job_like_any_other(daemon_factory, server):
    port = free_port()
    d = daemon_factory(base_config([
        {"name": "main-app", "exec": "sleep 60"},
        {"name": "tick", "http": server.url("/ok/tick"),
         "when": {"interval": "100ms"}},
    ], telemetry={"port": port, "interfaces": ["static:127.0.0.1"]})).start()
    d.wait_for_socket()
    assert wait_until(lambda: len(server.seen("/ok/tick")) >= 3), \
        d.log()[-3000:]
    import urllib.request
    with urllib.request.urlopen("http://127.0.0.1:%d/status" % port,
                                timeout=5) as resp:
        status = json.load(resp)
    assert "tick" in [j["Name"] for j in status["Jobs"]]
    with urllib.request.urlopen("http://127.0.0.1:%d/metrics" % port,
                                timeout=5) as resp:
        metrics = resp.read().decode()
    assert 'containerpilot_events{code="ExitSuccess",source="tick"}' in metrics
    finish(d)
