"""Native tcp health checks at the BASELINE stress cadence on the box.

As in test_gpu_box.py, "gpu" means the MI355X node's host: the workload
is a CPU-only daemon. 100 jobs x 100 ms tcp checks is the smallest shape
where probes overlap, the loop's batch caps engage and many sockets are
in flight at once.
"""

import os
import sys
import tempfile
import time

import pytest

from containerpilot_amd import harness

JOBS = 100
CHECK_MS = 100
# 100 jobs x 10 checks/s: one connection per check, two events per check
# (ExitSuccess check.<job> + StatusHealthy <job>)
CHECKS_PER_SEC = JOBS * 1000.0 / CHECK_MS
# the margin test_gpu_box.py allows on its 11,000/s exec-check shape
MARGIN = 0.97


@pytest.mark.gpu
def test_tcp_probes_sustain_the_check_rate_on_gpu_box():
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    from bench import stress_config, free_port, scrape
    from containerpilot_amd.mockconsul import MockConsul

    mc = MockConsul().start()
    sink = harness.ProbeSink("accept").start()
    wd = tempfile.mkdtemp(prefix="cpilot-gpu-probe-")
    port = free_port()
    cfg = stress_config(mc.address, port, JOBS, 0, CHECK_MS,
                        os.path.join(wd, "cp.socket"))
    for job in cfg["jobs"]:
        job["health"] = {"tcp": "127.0.0.1:%d" % sink.port,
                         "interval": "%dms" % CHECK_MS, "ttl": 10}
    d = harness.Daemon(config_dict=cfg, workdir=wd)
    try:
        d.start()
        d.wait_for_socket(timeout=30)
        time.sleep(2)  # warmup: exclude the startup/registration burst
        # each counter is read at both window edges with its own clock
        # reading, so neither rate is diluted by the other's request
        a0, ta0 = sink.accepted(), time.monotonic()
        s0, ts0 = scrape(port), time.monotonic()
        time.sleep(3)
        a1, ta1 = sink.accepted(), time.monotonic()
        s1, ts1 = scrape(port), time.monotonic()
        published_per_sec = (s1["published"] - s0["published"]) / (ts1 - ts0)
        accepted_per_sec = (a1 - a0) / (ta1 - ta0)
        print("published/s=%.1f accepted/s=%.1f window=%.3fs"
              % (published_per_sec, accepted_per_sec, ts1 - ts0))
        assert published_per_sec >= MARGIN * 2 * CHECKS_PER_SEC, \
            (published_per_sec, s0["published"], s1["published"])
        assert accepted_per_sec >= MARGIN * CHECKS_PER_SEC, (a0, a1)
        d.terminate()
        assert d.wait(timeout=60) == 0, d.log()[-4000:]
    finally:
        d.cleanup()
        sink.stop()
        mc.stop()
