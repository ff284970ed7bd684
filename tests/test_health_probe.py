"""Native health checks end to end: the daemon binary probing a Python
HTTP fixture whose status the test flips, registering and heartbeating
against the mock Consul, with /status, `when:` sources, maintenance and
reload behaving exactly as they do for exec checks, and no process
launched per check."""

import json
import socket
import threading
import time
import urllib.request
from http.server import BaseHTTPRequestHandler, ThreadingHTTPServer

import pytest

from containerpilot_amd import harness


def wait_until(predicate, timeout=10.0, interval=0.05):
    deadline = time.time() + timeout
    while time.time() < deadline:
        if predicate():
            return True
        time.sleep(interval)
    return False


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


class HealthFixture:
    """An HTTP server answering every GET with `self.status`."""

    def __init__(self):
        self.status = 200
        self.requests = 0
        self.user_agents = set()
        self.paths = set()
        fixture = self

        class Handler(BaseHTTPRequestHandler):
            def log_message(self, fmt, *args):
                pass

            def do_GET(self):
                fixture.requests += 1
                fixture.user_agents.add(self.headers.get("User-Agent"))
                fixture.paths.add(self.path)
                body = b"status %d\n" % fixture.status
                try:
                    self.send_response(fixture.status)
                    self.send_header("Content-Length", str(len(body)))
                    self.end_headers()
                    self.wfile.write(body)
                except OSError:
                    pass  # the probe resets once it has the status line

        class Server(ThreadingHTTPServer):
            daemon_threads = True

            def handle_error(self, request, client_address):
                pass  # resets from the probe's abortive close

        self.server = Server(("127.0.0.1", 0), Handler)
        self.port = self.server.server_address[1]
        self.thread = threading.Thread(target=self.server.serve_forever,
                                       daemon=True)

    def start(self):
        self.thread.start()
        return self

    def stop(self):
        self.server.shutdown()
        self.server.server_close()


@pytest.fixture
def health_fixture():
    fixture = HealthFixture().start()
    yield fixture
    fixture.stop()


@pytest.fixture
def sink():
    """Start bin/cpilot_probesink in a mode; yields start(mode) -> port."""
    sinks = []

    def start(mode):
        sinks.append(harness.ProbeSink(mode).start())
        return sinks[-1].port

    yield start
    for s in sinks:
        s.stop()


def service_status(telemetry_port, name):
    url = "http://127.0.0.1:%d/status" % telemetry_port
    try:
        with urllib.request.urlopen(url, timeout=2) as resp:
            doc = json.loads(resp.read().decode())
    except OSError:
        return None
    for svc in doc["Services"]:
        if svc["Name"] == name:
            return svc["Status"]
    return None


def test_http_check_follows_the_fixture(daemon_factory, mock_consul,
                                        health_fixture):
    telemetry_port = free_port()
    d = daemon_factory({
        "consul": mock_consul.address,
        "stopTimeout": 1,
        "logging": {"level": "DEBUG"},
        "jobs": [
            {"name": "web", "exec": "sleep 60", "port": 8000,
             "interfaces": ["static:10.1.2.3"],
             "health": {
                 "http": "http://localhost:%d/health" % health_fixture.port,
                 "interval": "100ms", "ttl": 5}},
            {"name": "on-healthy", "exec": "echo web-became-healthy",
             "when": {"source": "web", "once": "healthy"}},
        ],
        "telemetry": {"port": telemetry_port,
                      "interfaces": ["static:127.0.0.1"]},
    }).start()
    d.wait_for_socket()

    def status():
        return service_status(telemetry_port, "web")

    # 200: registers, receives TTL passes, reports healthy
    svc_id = "web-%s" % socket.gethostname()
    assert wait_until(lambda: svc_id in mock_consul.services), d.log()
    assert wait_until(lambda: len([u for u in mock_consul.ttl_updates
                                   if u[0] == "service:" + svc_id]) >= 2)
    assert all(u[1]["Status"] == "passing" for u in mock_consul.ttl_updates
               if u[0] == "service:" + svc_id)
    assert wait_until(lambda: status() == "healthy"), d.log()
    # ... and a job waiting on the service's health fires, once
    assert wait_until(lambda: "web-became-healthy" in d.log()), d.log()

    # 500: unhealthy, with the documented reason in the log
    health_fixture.status = 500
    assert wait_until(lambda: status() == "unhealthy"), d.log()
    assert wait_until(
        lambda: "check.web: unexpected status 500" in d.log()), d.log()
    assert "{ExitFailed check.web}" in d.log()
    assert "{StatusUnhealthy web}" in d.log()

    # back to 200: recovers
    health_fixture.status = 200
    assert wait_until(lambda: status() == "healthy"), d.log()

    # maintenance stops the probing itself, not just the verdicts
    code, _ = d.control("POST", "/v3/maintenance/enable")
    assert code == 200
    assert wait_until(lambda: status() == "maintenance")
    time.sleep(0.25)  # one interval plus the probe already in flight
    seen = health_fixture.requests
    time.sleep(0.5)  # five intervals
    assert health_fixture.requests == seen
    code, _ = d.control("POST", "/v3/maintenance/disable")
    assert code == 200
    assert wait_until(lambda: health_fixture.requests > seen)
    assert wait_until(lambda: status() == "healthy"), d.log()

    d.terminate()
    assert d.wait(timeout=30) == 0, d.log()
    log = d.log()

    # the request the fixture saw
    assert health_fixture.paths == {"/health"}
    assert len(health_fixture.user_agents) == 1
    agent = health_fixture.user_agents.pop()
    assert agent.startswith("containerpilot/") and len(agent) > 15, agent

    # no process was launched for any check; the job itself still ran one
    assert "check.web.Run start" not in log
    assert "web.Run start" in log
    assert log.count("web-became-healthy") == 1
    assert svc_id in mock_consul.deregistered


def test_tcp_check_closed_port_is_unhealthy(daemon_factory, mock_consul):
    telemetry_port = free_port()
    closed = free_port()  # bound, read, closed: nothing listens there
    d = daemon_factory({
        "consul": mock_consul.address,
        "stopTimeout": 1,
        "logging": {"level": "DEBUG"},
        "jobs": [{"name": "db", "exec": "sleep 60", "port": 5432,
                  "interfaces": ["static:10.1.2.3"],
                  "health": {"tcp": "127.0.0.1:%d" % closed,
                             "interval": "100ms", "ttl": 5}}],
        "telemetry": {"port": telemetry_port,
                      "interfaces": ["static:127.0.0.1"]},
    }).start()
    d.wait_for_socket()
    assert wait_until(
        lambda: service_status(telemetry_port, "db") == "unhealthy"), d.log()
    assert "check.db: Connection refused" in d.log()
    assert not [u for u in mock_consul.ttl_updates
                if u[0].startswith("service:db-")]
    d.terminate()
    assert d.wait(timeout=30) == 0, d.log()
    assert "check.db.Run start" not in d.log()


def test_tcp_check_open_port_is_healthy(daemon_factory, mock_consul, sink):
    telemetry_port = free_port()
    d = daemon_factory({
        "consul": mock_consul.address,
        "stopTimeout": 1,
        "jobs": [{"name": "db", "exec": "sleep 60", "port": 5432,
                  "interfaces": ["static:10.1.2.3"],
                  "health": {"tcp": "127.0.0.1:%d" % sink("accept"),
                             "interval": "100ms", "ttl": 5}}],
        "telemetry": {"port": telemetry_port,
                      "interfaces": ["static:127.0.0.1"]},
    }).start()
    d.wait_for_socket()
    assert wait_until(
        lambda: service_status(telemetry_port, "db") == "healthy"), d.log()
    d.terminate()
    assert d.wait(timeout=30) == 0, d.log()


def test_reload_hammering_with_probes_in_flight(daemon_factory, sink):
    """Every reload tears a generation down while its probes hang on a
    peer that never answers; each must be canceled with its job, and the
    drain must not need the kill sweep."""
    port = sink("hang")
    d = daemon_factory({
        "consul": "localhost:8500",
        "stopTimeout": 1,
        "logging": {"level": "DEBUG"},
        "jobs": [{"name": "svc-%d" % i, "exec": "sleep 60",
                  "health": {"http": "http://127.0.0.1:%d/" % port,
                             "interval": "100ms", "timeout": "30s",
                             "ttl": 5}}
                 for i in range(8)],
    }).start()
    d.wait_for_socket()
    assert wait_until(lambda: d.log().count("still in flight") >= 8), d.log()
    ok = 0
    for _ in range(8):
        try:
            code, _ = d.control("POST", "/v3/reload")
            ok += code == 200
        except OSError:
            pass  # socket mid-flip between generations
        time.sleep(0.1)
        d.wait_for_socket(timeout=10)
    assert ok >= 3
    d.wait_for_socket(timeout=10)
    d.terminate()
    assert d.wait(timeout=30) == 0, d.log()
    log = d.log()
    assert "canceled in flight" in log
    assert "stop timeout exceeded" not in log
    # hung probes never produced a verdict, in any generation
    assert "{ExitFailed check.svc-" not in log
    assert "{ExitSuccess check.svc-" not in log
