"""Signal jobs on the box, with the daemon as deployed.

As in test_gpu_box.py, "gpu" means the MI355X node's host: the workload
is a CPU-only daemon, here behind its subreaper supervisor. Ten trapping
targets and fifty signal jobs at 100 ms, five per target, give 500
deliveries/s: the smallest shape where deliveries interleave with the
spawn-helper traffic of the targets' own launches.

An interval job also runs once at start-up, when every target's launch is
still in flight and has no pid: that run fails by the documented rule. So
"no ExitFailed" is required of the measured window, and of the time before
it only that no job failed more than that once.
"""

import re
import socket
import time
import urllib.request

import pytest

from containerpilot_amd.mockconsul import MockConsul

from test_signal_jobs import (finish, lines, ready, run_render_reload,
                              trap_target, wait_running)

TARGETS = 10
JOBS_PER_TARGET = 5
INTERVAL_MS = 100
DELIVERIES_PER_SEC = TARGETS * JOBS_PER_TARGET * 1000.0 / INTERVAL_MS
# the margin test_gpu_box.py, test_gpu_box_probe.py and
# test_gpu_box_sensors.py allow at this cadence
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
    """{(code, source): count} for the signal jobs' events."""
    url = "http://127.0.0.1:%d/metrics" % port
    with urllib.request.urlopen(url, timeout=10) as resp:
        text = resp.read().decode()
    events = {}
    for m in re.finditer(r'^containerpilot_events\{code="([^"]*)",'
                         r'source="(sig-[^"]*)"\} (\S+)$', text, re.M):
        events[(m.group(1), m.group(2))] = float(m.group(3))
    return events


def total(events, code, prefix="sig-"):
    return sum(v for (c, source), v in events.items()
               if c == code and source.startswith(prefix))


@pytest.mark.gpu
def test_render_then_reload_on_gpu_box(daemon_factory, mock_consul, tmp_path):
    d = run_render_reload(daemon_factory, mock_consul, tmp_path, env=SUP)
    assert "onchange-backend.Run start" not in d.log()
    finish(d)


@pytest.mark.gpu
def test_signal_jobs_sustain_the_delivery_rate_on_gpu_box(daemon_factory,
                                                          tmp_path):
    t_start = time.monotonic()
    mc = MockConsul().start()
    port = free_port()
    jobs, outs = [], []
    for t in range(TARGETS):
        out = tmp_path / ("target-%02d.out" % t)
        outs.append(out)
        jobs.append(trap_target("target-%02d" % t, out, sig="USR1"))
        for j in range(JOBS_PER_TARGET):
            jobs.append({"name": "sig-%02d-%d" % (t, j),
                         "when": {"interval": "%dms" % INTERVAL_MS},
                         "signal": {"job": "target-%02d" % t,
                                    "send": "SIGUSR1"}})
    d = daemon_factory({
        "consul": mc.address, "stopTimeout": 1,
        "logging": {"level": "WARN"}, "jobs": jobs,
        "telemetry": {"port": port, "interfaces": ["static:127.0.0.1"]},
    }, env=SUP)
    try:
        d.start()
        d.wait_for_socket(timeout=30)
        time.sleep(WARMUP_S)
        # the start-up runs found the launches in flight: by now every
        # target is up, so nothing fails from here on
        assert all(ready(out)() for out in outs), d.log()[-3000:]
        wait_running(d, *["target-%02d" % t for t in range(TARGETS)])
        e0 = scrape(port)
        t0 = time.monotonic()
        time.sleep(WINDOW_S)
        e1 = scrape(port)
        t1 = time.monotonic()

        ok = total(e1, "ExitSuccess") - total(e0, "ExitSuccess")
        failed = total(e1, "ExitFailed") - total(e0, "ExitFailed")
        rate = ok / (t1 - t0)
        print("deliveries/s=%.1f (want >= %.1f) window=%.3fs failed=%d"
              % (rate, MARGIN * DELIVERIES_PER_SEC, t1 - t0, failed))
        assert ok >= MARGIN * DELIVERIES_PER_SEC * (t1 - t0), (ok, t1 - t0)
        assert failed == 0, {k: v for k, v in e1.items()
                             if k[0] == "ExitFailed" and v != e0.get(k, 0)}
        # before the window only a start-up run can have failed: it found
        # its target's launch still in flight
        print("failed before the window: %d" % total(e0, "ExitFailed"))
        assert all(v <= 1 for k, v in e1.items() if k[0] == "ExitFailed"), e1
        assert len([k for k in e1 if k[0] == "ExitSuccess"]) == \
            TARGETS * JOBS_PER_TARGET

        # standard signals coalesce: each target saw at least one, and no
        # more than were sent to it (files read first, counters after)
        recorded = [len(lines(out)) for out in outs]
        e2 = scrape(port)
        for t, got in enumerate(recorded):
            sent = total(e2, "ExitSuccess", prefix="sig-%02d-" % t)
            assert 1 <= got <= sent, (t, got, sent)
        print("recorded per target: %s" % recorded)

        d.terminate()
        assert d.wait(timeout=30) == 0, d.log()[-4000:]
    finally:
        mc.stop()
    assert time.monotonic() - t_start < 8
