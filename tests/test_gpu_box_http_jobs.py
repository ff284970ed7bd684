"""Http jobs on the box, with the daemon as deployed.

As in test_gpu_box.py, "gpu" means the MI355X node's host: the workload
is a CPU-only daemon, here behind its subreaper supervisor. One
`cpilot_probesink http200`, which answers with a length and closes, and
fifty http jobs doing a bodyless GET every 100 ms give 500 actions/s: the
smallest shape where several requests are in flight in one loop turn and
both the drain and the close path run continuously.

The sink is up before the daemon starts, so unlike signal jobs there is no
start-up race: no request may fail in the whole run.

Recorded run (MI355X node host, 2026-10-21, together with the other
gpu-marked tests): 501.7 actions/s and 501.3 accepted connections/s over a
3.004 s window against a floor of 485.0, no failed request in the whole
run, the daemon exited 0.
"""

import re
import socket
import time
import urllib.request

import pytest

from containerpilot_amd import harness
from containerpilot_amd.mockconsul import MockConsul

JOBS = 50
INTERVAL_MS = 100
ACTIONS_PER_SEC = JOBS * 1000.0 / INTERVAL_MS
# the margin test_gpu_box.py, test_gpu_box_probe.py, test_gpu_box_sensors.py
# and test_gpu_box_signals.py allow at this cadence
MARGIN = 0.97
WARMUP_S = 2
WINDOW_S = 3
SUP = {"CPILOT_FORCE_SUP": "1"}


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def scrape(port):
    """{(code, source): count} for the http jobs' events."""
    url = "http://127.0.0.1:%d/metrics" % port
    with urllib.request.urlopen(url, timeout=10) as resp:
        text = resp.read().decode()
    events = {}
    for m in re.finditer(r'^containerpilot_events\{code="([^"]*)",'
                         r'source="(act-[^"]*)"\} (\S+)$', text, re.M):
        events[(m.group(1), m.group(2))] = float(m.group(3))
    return events


def total(events, code):
    return sum(v for (c, _), v in events.items() if c == code)


@pytest.mark.gpu
def test_http_jobs_sustain_the_action_rate_on_gpu_box(daemon_factory):
    t_start = time.monotonic()
    mc = MockConsul().start()
    sink = harness.ProbeSink("http200").start()
    port = free_port()
    jobs = [{"name": "act-%02d" % j,
             "http": "http://127.0.0.1:%d/tick" % sink.port,
             "when": {"interval": "%dms" % INTERVAL_MS}}
            for j in range(JOBS)]
    d = daemon_factory({
        "consul": mc.address, "stopTimeout": 1,
        "logging": {"level": "WARN"}, "jobs": jobs,
        "telemetry": {"port": port, "interfaces": ["static:127.0.0.1"]},
    }, env=SUP)
    try:
        d.start()
        d.wait_for_socket(timeout=30)
        time.sleep(WARMUP_S)
        # each counter is read at both window edges with its own clock
        # reading, so neither rate is diluted by the other's request
        a0, ta0 = sink.accepted(), time.monotonic()
        e0, te0 = scrape(port), time.monotonic()
        time.sleep(WINDOW_S)
        a1, ta1 = sink.accepted(), time.monotonic()
        e1, te1 = scrape(port), time.monotonic()

        ok = total(e1, "ExitSuccess") - total(e0, "ExitSuccess")
        accepted = a1 - a0
        print("actions/s=%.1f accepted/s=%.1f (want >= %.1f) window=%.3fs "
              "failed=%d"
              % (ok / (te1 - te0), accepted / (ta1 - ta0),
                 MARGIN * ACTIONS_PER_SEC, te1 - te0,
                 total(e1, "ExitFailed")))
        assert ok >= MARGIN * ACTIONS_PER_SEC * (te1 - te0), (ok, te1 - te0)
        assert accepted >= MARGIN * ACTIONS_PER_SEC * (ta1 - ta0), \
            (accepted, ta1 - ta0)
        assert len([k for k in e1 if k[0] == "ExitSuccess"]) == JOBS

        d.terminate()
        assert d.wait(timeout=30) == 0, d.log()[-4000:]
        # nothing failed in the whole run: not in the last scrape, and a
        # failure after it would have left its warning in the log
        assert total(e1, "ExitFailed") == 0, \
            {k: v for k, v in e1.items() if k[0] == "ExitFailed"}
        assert "act-" not in d.log(), d.log()[-4000:]
    finally:
        sink.stop()
        mc.stop()
    assert time.monotonic() - t_start < 10
