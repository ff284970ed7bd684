"""Native telemetry sensors at a 100 ms cadence on the box.

As in test_gpu_box.py, "gpu" means the MI355X node's host: the workload
is a CPU-only daemon. 50 file sensors at 100 ms plus one on /proc/meminfo
is the smallest shape where samples overlap across the worker pool. The
amdgpu sysfs file, when one is readable, is read through a sensor too.
"""

import glob
import os
import re
import socket
import tempfile
import time
import urllib.request

import pytest

from containerpilot_amd import harness
from containerpilot_amd.mockconsul import MockConsul

FILE_SENSORS = 50
INTERVAL_MS = 100
SAMPLES_PER_SEC = (FILE_SENSORS + 1) * 1000.0 / INTERVAL_MS
# the margin test_gpu_box.py and test_gpu_box_probe.py allow at this cadence
MARGIN = 0.97
WARMUP_S = 2
WINDOW_S = 3
VRAM_GLOB = "/sys/class/drm/card*/device/mem_info_vram_used"


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def scrape(port):
    url = "http://127.0.0.1:%d/metrics" % port
    with urllib.request.urlopen(url, timeout=10) as resp:
        text = resp.read().decode()
    samples = {}
    for m in re.finditer(r'^containerpilot_sensor_samples\{sensor="([^"]*)",'
                         r'result="([^"]*)"\} (\S+)$', text, re.M):
        samples[(m.group(1), m.group(2))] = float(m.group(3))
    gauges = {}
    for m in re.finditer(r"^(box_[a-z_0-9]+) (\S+)$", text, re.M):
        gauges[m.group(1)] = float(m.group(2))
    return samples, gauges


def total(samples, result, skip=()):
    return sum(v for (name, res), v in samples.items()
               if res == result and name not in skip)


def mem_total_bytes():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemTotal:"):
                return int(line.split()[1]) * 1024
    raise AssertionError("no MemTotal in /proc/meminfo")


def readable_vram_file():
    for path in sorted(glob.glob(VRAM_GLOB)):
        try:
            with open(path) as f:
                int(f.read().strip())
            return path
        except (OSError, ValueError):
            continue
    return None


@pytest.mark.gpu
def test_sensors_sustain_the_sample_rate_on_gpu_box():
    t_start = time.monotonic()
    mc = MockConsul().start()
    wd = tempfile.mkdtemp(prefix="cpilot-gpu-sensors-")
    port = free_port()
    metrics = [{"namespace": "box", "subsystem": "mem", "name": "available",
                "type": "gauge", "help": "MemAvailable in bytes"},
               {"namespace": "box", "subsystem": "vram", "name": "used",
                "type": "gauge", "help": "VRAM in use"}]
    sensors = [{"name": "meminfo", "file": "/proc/meminfo",
                "interval": "%dms" % INTERVAL_MS,
                "record": [{"metric": "box_mem_available", "scale": 1024,
                            "line": "MemAvailable:", "field": 2}]}]
    for i in range(FILE_SENSORS):
        path = os.path.join(wd, "source-%02d" % i)
        with open(path, "w") as f:
            f.write("value %d\n" % i)
        metrics.append({"namespace": "box", "subsystem": "file",
                        "name": "v%02d" % i, "type": "gauge", "help": "file"})
        sensors.append({"name": "file-%02d" % i, "file": path,
                        "interval": "%dms" % INTERVAL_MS,
                        "record": [{"metric": "box_file_v%02d" % i,
                                    "line": "value", "field": 2}]})
    vram = readable_vram_file()
    if vram:
        print("vram sensor on %s" % vram)
        sensors.append({"name": "vram", "file": vram, "interval": "500ms",
                        "record": [{"metric": "box_vram_used"}]})
    else:
        print("no readable %s: running without the vram sensor" % VRAM_GLOB)

    d = harness.Daemon(config_dict={
        "consul": mc.address, "stopTimeout": 1,
        "logging": {"level": "WARN"},
        "telemetry": {"port": port, "interfaces": ["static:127.0.0.1"],
                      "metrics": metrics, "sensors": sensors},
    }, workdir=wd, env={"CPILOT_FORCE_SUP": "1"})
    try:
        d.start()
        d.wait_for_socket(timeout=30)
        time.sleep(WARMUP_S)
        s0, _ = scrape(port)
        t0 = time.monotonic()
        time.sleep(WINDOW_S)
        s1, gauges = scrape(port)
        t1 = time.monotonic()

        # the 51 sensors at the 100 ms cadence; the vram sensor is slower
        # and is judged on its own below
        ok = total(s1, "ok", skip=("vram",)) - total(s0, "ok", skip=("vram",))
        rate = ok / (t1 - t0)
        print("ok samples/s=%.1f (want >= %.1f) window=%.3fs errors=%s"
              % (rate, MARGIN * SAMPLES_PER_SEC, t1 - t0, total(s1, "error")))
        assert ok >= MARGIN * SAMPLES_PER_SEC * (t1 - t0), (ok, t1 - t0)
        assert total(s1, "error") == 0, \
            {k: v for k, v in s1.items() if k[1] == "error" and v}
        assert len([k for k in s1 if k[1] == "ok"]) == len(sensors)

        assert 0 < gauges["box_mem_available"] <= mem_total_bytes(), gauges
        for i in (0, FILE_SENSORS - 1):
            assert gauges["box_file_v%02d" % i] == i
        if vram:
            print("vram used=%d" % gauges["box_vram_used"])
            assert s1[("vram", "ok")] >= 2, s1
            assert gauges["box_vram_used"] >= 0

        d.terminate()
        assert d.wait(timeout=30) == 0, d.log()[-4000:]
        assert "sample failed" not in d.log()
    finally:
        d.cleanup()
        mc.stop()
    assert time.monotonic() - t_start < 10
