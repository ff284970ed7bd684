"""Native telemetry sensors end to end: a daemon samples files and HTTP
endpoints itself and the values show up on /metrics. No job is configured
in any of these, so nothing is ever spawned."""

import http.client
import http.server
import json
import os
import re
import signal
import socket
import subprocess
import threading
import time
import urllib.request

from containerpilot_amd import BINARY

INTERVAL_MS = 100
INTERVAL = INTERVAL_MS / 1000.0


def wait_until(predicate, timeout=10.0, interval=0.02):
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


def write_atomic(path, text):
    tmp = str(path) + ".tmp"
    with open(tmp, "w") as f:
        f.write(text)
    os.rename(tmp, str(path))


class Scraper:
    def __init__(self, port):
        self.url = "http://127.0.0.1:%d/metrics" % port

    def text(self):
        with urllib.request.urlopen(self.url, timeout=5) as resp:
            return resp.read().decode()

    def up(self):
        try:
            self.text()
            return True
        except (OSError, http.client.HTTPException):
            return False

    def value(self, series):
        """The value of an exact series (name plus labels), or None (also
        while the endpoint is down between two config generations)."""
        try:
            text = self.text()
        except (OSError, http.client.HTTPException):
            return None
        m = re.search(r"^%s ([^ \n]+)$" % re.escape(series), text, re.M)
        return float(m.group(1)) if m else None

    def samples(self, sensor, result):
        return self.value('containerpilot_sensor_samples{sensor="%s",'
                          'result="%s"}' % (sensor, result))


def metric(key, kind):
    ns, sub, name = key.split("_", 2)
    return {"namespace": ns, "subsystem": sub, "name": name, "type": kind,
            "help": key}


def start(daemon_factory, mock_consul, metrics, sensors, log_format="default"):
    port = free_port()
    d = daemon_factory({
        "consul": mock_consul.address,
        "stopTimeout": 1,
        "logging": {"level": "INFO", "format": log_format},
        "telemetry": {"port": port, "interfaces": ["static:127.0.0.1"],
                      "metrics": metrics, "sensors": sensors},
    }).start()
    d.wait_for_socket()
    scraper = Scraper(port)
    assert wait_until(scraper.up), d.log()
    return d, scraper


def file_sensor(name, path, records):
    return {"name": name, "file": str(path),
            "interval": "%dms" % INTERVAL_MS, "record": records}


def finish(d):
    d.terminate()
    assert d.wait(timeout=30) == 0, d.log()[-4000:]


def test_file_gauge_follows_the_file(daemon_factory, mock_consul, tmp_path):
    path = tmp_path / "value"
    write_atomic(path, "MemAvailable:   100 kB\n")
    d, scrape = start(
        daemon_factory, mock_consul, [metric("t_mem_avail", "gauge")],
        [file_sensor("mem", path, [{"metric": "t_mem_avail", "scale": 1024,
                                    "line": "MemAvailable:", "field": 2}])])
    assert wait_until(lambda: scrape.value("t_mem_avail") == 102400.0), \
        d.log()
    ok0 = scrape.samples("mem", "ok")
    for kb in (250, 7):
        write_atomic(path, "MemAvailable:   %d kB\n" % kb)
        t0 = time.monotonic()
        # within two intervals, plus the scrape's own round trips
        assert wait_until(lambda: scrape.value("t_mem_avail") == kb * 1024.0,
                          timeout=2 * INTERVAL + 0.3), scrape.text()
        assert time.monotonic() - t0 < 2 * INTERVAL + 0.4
    assert wait_until(lambda: scrape.samples("mem", "ok") >= ok0 + 3)
    assert scrape.samples("mem", "error") == 0
    finish(d)


def test_counter_publishes_increases(daemon_factory, mock_consul, tmp_path):
    path = tmp_path / "total"
    write_atomic(path, "10\n")
    d, scrape = start(
        daemon_factory, mock_consul, [metric("t_req_total", "counter")],
        [file_sensor("total", path, [{"metric": "t_req_total"}])])
    # the first good sample only sets the baseline
    assert wait_until(lambda: scrape.samples("total", "ok") >= 2)
    assert scrape.value("t_req_total") == 0
    write_atomic(path, "15\n")
    assert wait_until(lambda: scrape.value("t_req_total") == 5), scrape.text()
    write_atomic(path, "3\n")  # the source restarted
    assert wait_until(lambda: scrape.value("t_req_total") == 8), scrape.text()
    ok = scrape.samples("total", "ok")
    assert wait_until(lambda: scrape.samples("total", "ok") >= ok + 2)
    assert scrape.value("t_req_total") == 8
    finish(d)


STUB = ("Active connections: 291 \n"
        "server accepts handled requests\n"
        " %d 16630948 31070465 \n"
        "Reading: 6 Writing: 179 Waiting: 106 \n")


class StatsServer:
    """An http.server thread that counts the requests per path."""

    def __init__(self):
        self.hits = {}
        self.accepts = 1000
        self.lock = threading.Lock()
        outer = self

        class Handler(http.server.BaseHTTPRequestHandler):
            def do_GET(self):
                with outer.lock:
                    outer.hits[self.path] = outer.hits.get(self.path, 0) + 1
                    accepts = outer.accepts
                    if self.path == "/stub_status":
                        outer.accepts += 7
                if self.path == "/stub_status":
                    body, code = STUB % accepts, 200
                elif self.path == "/stats":
                    body = json.dumps({"queue": {"depth": 12, "lag": "0.25"},
                                       "token": self.headers.get("X-Token")})
                    code = 200
                else:
                    body, code = "no", 404
                data = body.encode()
                self.send_response(code)
                self.send_header("Content-Length", str(len(data)))
                self.end_headers()
                self.wfile.write(data)

            def log_message(self, *args):
                pass

        self.httpd = http.server.ThreadingHTTPServer(("127.0.0.1", 0), Handler)
        self.port = self.httpd.server_address[1]
        self.thread = threading.Thread(target=self.httpd.serve_forever,
                                       daemon=True)
        self.thread.start()

    def count(self, path):
        with self.lock:
            return self.hits.get(path, 0)

    def stop(self):
        self.httpd.shutdown()
        self.httpd.server_close()


def test_http_source_one_fetch_feeds_every_record(daemon_factory,
                                                  mock_consul):
    srv = StatsServer()
    try:
        base = "http://127.0.0.1:%d" % srv.port
        d, scrape = start(
            daemon_factory, mock_consul,
            [metric("t_ngx_accepts", "counter"),
             metric("t_ngx_active", "gauge"),
             metric("t_app_depth", "gauge"), metric("t_app_lag", "gauge"),
             metric("t_app_missing", "gauge")],
            [{"name": "nginx", "http": base + "/stub_status",
              "interval": "%dms" % INTERVAL_MS,
              "record": [
                  {"metric": "t_ngx_accepts", "lineNumber": 3, "field": 1},
                  {"metric": "t_ngx_active", "line": "Active", "field": 3}]},
             {"name": "app", "http": {"url": base + "/stats",
                                      "headers": {"X-Token": "tok"}},
              "interval": "%dms" % INTERVAL_MS, "timeout": "1s",
              "record": [{"metric": "t_app_depth", "json": "/queue/depth"},
                         {"metric": "t_app_lag", "json": "/queue/lag",
                          "scale": 4}]},
             {"name": "gone", "http": base + "/nope",
              "interval": "%dms" % INTERVAL_MS,
              "record": [{"metric": "t_app_missing"}]}])
        assert wait_until(lambda: (scrape.samples("nginx", "ok") or 0) >= 5
                          and (scrape.samples("app", "ok") or 0) >= 5), \
            d.log()
        assert scrape.value("t_ngx_active") == 291
        assert scrape.value("t_app_depth") == 12
        assert scrape.value("t_app_lag") == 1.0
        # every fetch adds 7 to the running total; the first is the baseline
        for name, path in (("nginx", "/stub_status"), ("app", "/stats")):
            r0 = srv.count(path)
            text = scrape.text()
            r1 = srv.count(path)
            got = {}
            for result in ("ok", "error"):
                m = re.search(r'^containerpilot_sensor_samples\{sensor="%s",'
                              r'result="%s"\} (\S+)$' % (name, result), text,
                              re.M)
                got[result] = float(m.group(1))
            assert got["error"] == 0
            # one request per sample (at most one in flight), not one per
            # record, which would be twice as many
            assert r0 - 1 <= got["ok"] <= r1, (name, r0, got, r1)
        text = scrape.text()
        ok = float(re.search(r'sensor="nginx",result="ok"\} (\S+)',
                             text).group(1))
        accepts = float(re.search(r"^t_ngx_accepts (\S+)$", text,
                                  re.M).group(1))
        assert accepts in (7 * (ok - 1), 7 * ok), (accepts, ok)
        # a 404 is a failed sample and leaves the gauge alone
        assert scrape.samples("gone", "ok") == 0
        assert scrape.samples("gone", "error") >= 1
        assert scrape.value("t_app_missing") == 0
        assert "sensor gone: sample failed: status 404" in d.log()
        finish(d)
    finally:
        srv.stop()


def test_failure_keeps_the_value_and_logs_once(daemon_factory, mock_consul,
                                               tmp_path):
    path = tmp_path / "value"
    write_atomic(path, "41\n")
    d, scrape = start(
        daemon_factory, mock_consul, [metric("t_file_value", "gauge")],
        [file_sensor("flaky", path, [{"metric": "t_file_value"}])],
        log_format="text")  # the text format shows each line's level
    assert wait_until(lambda: scrape.value("t_file_value") == 41)
    os.unlink(str(path))
    assert wait_until(lambda: scrape.samples("flaky", "error") >= 3), d.log()
    assert scrape.value("t_file_value") == 41
    write_atomic(path, "oops\n")  # a second kind of failure, same outage
    e = scrape.samples("flaky", "error")
    assert wait_until(lambda: scrape.samples("flaky", "error") >= e + 2)
    assert scrape.value("t_file_value") == 41
    write_atomic(path, "42\n")
    assert wait_until(lambda: scrape.value("t_file_value") == 42)
    ok = scrape.samples("flaky", "ok")
    assert wait_until(lambda: scrape.samples("flaky", "ok") >= ok + 2)
    log = d.log()
    warns = [l for l in log.splitlines() if "sensor flaky: sample failed" in l]
    infos = [l for l in log.splitlines() if "sensor flaky: recovered" in l]
    assert len(warns) == 1, log
    assert "open: No such file or directory" in warns[0]
    assert "level=warn" in warns[0].lower()
    assert len(infos) == 1, log
    assert "level=info" in infos[0].lower()
    # nothing in the state machine reacts to a sensor
    assert 'code="Error"' not in scrape.text()
    finish(d)


def test_putmetric_next_to_a_sensor(daemon_factory, mock_consul, tmp_path):
    path = tmp_path / "total"
    write_atomic(path, "10\n")
    d, scrape = start(
        daemon_factory, mock_consul,
        [metric("t_req_total", "counter"), metric("t_other_gauge", "gauge")],
        [file_sensor("total", path, [{"metric": "t_req_total"}])])
    assert wait_until(lambda: scrape.samples("total", "ok") >= 2)
    out = subprocess.run(
        [BINARY, "-config", d.config_path, "-putmetric", "t_req_total=100",
         "-putmetric", "t_other_gauge=2.5"],
        capture_output=True, text=True, timeout=10)
    assert out.returncode == 0, out.stderr
    assert wait_until(lambda: scrape.value("t_req_total") == 100)
    assert scrape.value("t_other_gauge") == 2.5
    write_atomic(path, "14\n")
    assert wait_until(lambda: scrape.value("t_req_total") == 104), \
        scrape.text()
    finish(d)


def test_reload_restarts_the_baseline(daemon_factory, mock_consul, tmp_path):
    path = tmp_path / "total"
    write_atomic(path, "10\n")
    d, scrape = start(
        daemon_factory, mock_consul,
        [metric("t_req_total", "counter"), metric("t_req_level", "gauge")],
        [file_sensor("total", path, [{"metric": "t_req_total"},
                                     {"metric": "t_req_level"}])])
    assert wait_until(lambda: scrape.samples("total", "ok") >= 2)
    write_atomic(path, "15\n")
    assert wait_until(lambda: scrape.value("t_req_total") == 5)
    before = scrape.samples("total", "ok")
    pid = d.proc.pid

    status, _ = d.control("POST", "/v3/reload")
    assert status == 200
    # the sample counter lives across generations; user collectors restart
    assert wait_until(lambda: scrape.up() and
                      (scrape.samples("total", "ok") or 0) >= before + 3), \
        d.log()
    d.wait_for_socket(timeout=15)
    assert d.proc.poll() is None and d.proc.pid == pid
    # the new generation's first sample of 15 is a baseline, not +15
    assert scrape.value("t_req_total") == 0, scrape.text()
    assert scrape.value("t_req_level") == 15
    write_atomic(path, "18\n")
    assert wait_until(lambda: scrape.value("t_req_total") == 3), scrape.text()
    assert scrape.samples("total", "error") == 0
    finish(d)


def test_shutdown_with_a_hung_http_source(daemon_factory, mock_consul):
    # accepts (through the backlog) and never answers
    hung = socket.socket()
    hung.bind(("127.0.0.1", 0))
    hung.listen(8)
    try:
        d, scrape = start(
            daemon_factory, mock_consul, [metric("t_hung_value", "gauge")],
            [{"name": "hung", "interval": "%dms" % INTERVAL_MS,
              "timeout": "30s",
              "http": "http://127.0.0.1:%d/" % hung.getsockname()[1],
              "record": [{"metric": "t_hung_value"}]}])
        conn, _ = hung.accept()  # the fetch is in flight now
        assert scrape.samples("hung", "ok") == 0
        assert scrape.samples("hung", "error") == 0
        t0 = time.monotonic()
        d.signal(signal.SIGTERM)
        assert d.wait(timeout=30) == 0, d.log()[-4000:]
        assert time.monotonic() - t0 < 1 + 5  # stopTimeout + 5 s
        conn.close()
    finally:
        hung.close()


def test_reload_with_a_hung_http_source(daemon_factory, mock_consul):
    hung = socket.socket()
    hung.bind(("127.0.0.1", 0))
    hung.listen(8)
    try:
        d, scrape = start(
            daemon_factory, mock_consul, [metric("t_hung_value", "gauge")],
            [{"name": "hung", "interval": "%dms" % INTERVAL_MS,
              "timeout": "30s",
              "http": "http://127.0.0.1:%d/" % hung.getsockname()[1],
              "record": [{"metric": "t_hung_value"}]}])
        first, _ = hung.accept()
        t0 = time.monotonic()
        status, _ = d.control("POST", "/v3/reload")
        assert status == 200
        hung.settimeout(5)
        second, _ = hung.accept()  # the new generation samples again
        assert time.monotonic() - t0 < 5
        assert first.recv(65536).startswith(b"GET / HTTP/1.1\r\n")
        first.settimeout(5)
        assert first.recv(1) == b""  # the old fetch was shut down
        first.close()
        second.close()
        d.wait_for_socket(timeout=15)
        finish(d)
    finally:
        hung.close()


def test_no_process_is_launched(daemon_factory, mock_consul, tmp_path):
    path = tmp_path / "value"
    write_atomic(path, "5\n")
    d, scrape = start(
        daemon_factory, mock_consul, [metric("t_file_value", "gauge")],
        [file_sensor("quiet", path, [{"metric": "t_file_value"}])])
    assert wait_until(lambda: scrape.samples("quiet", "ok") >= 10), d.log()
    text = scrape.text()
    assert "containerpilot_events" in text
    assert "ExitSuccess" not in text
    assert "ExitFailed" not in text
    finish(d)


def test_metrics_unchanged_without_sensors(daemon_factory, mock_consul):
    port = free_port()
    d = daemon_factory({
        "consul": mock_consul.address, "stopTimeout": 1,
        "telemetry": {"port": port, "interfaces": ["static:127.0.0.1"],
                      "metrics": [metric("t_file_value", "gauge")],
                      "sensors": []},
    }).start()
    d.wait_for_socket()
    scrape = Scraper(port)
    assert wait_until(scrape.up)
    assert "containerpilot_sensor_samples" not in scrape.text()
    finish(d)
