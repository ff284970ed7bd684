"""The /metrics exposition under load on the box.

As in test_gpu_box.py, "gpu" means the MI355X node's host: the workload is
a CPU-only daemon. The stress config at 20 jobs x 100 ms keeps the event
counter and the dispatch histogram moving; two scrapes 2 s apart, a reload
and a third scrape must each parse strictly (containerpilot_amd.prommodel)
and keep the histogram invariants, and nothing may count backwards between
the first two.
"""

import os
import sys
import tempfile
import time
import urllib.request

import pytest

from containerpilot_amd import harness, prommodel
from containerpilot_amd.mockconsul import MockConsul

JOBS = 20
WATCHES = 2
CHECK_MS = 100
DISPATCH = "containerpilot_event_dispatch_seconds"


def scrape(port):
    url = "http://127.0.0.1:%d/metrics" % port
    with urllib.request.urlopen(url, timeout=10) as resp:
        text = resp.read().decode()
    families = prommodel.parse_exposition(text)
    for fam in families:
        if fam.type == "histogram":
            assert prommodel.histogram_violations(fam) == [], fam.name
    return {(s.name, s.labels): s.value for f in families for s in f.samples}


def wait_for_scrape(port, timeout=15.0):
    deadline = time.monotonic() + timeout
    while True:
        try:
            return scrape(port)
        except OSError:
            if time.monotonic() > deadline:
                raise
            time.sleep(0.05)


@pytest.mark.gpu
def test_exposition_stays_well_formed_under_load_and_reload_on_gpu_box():
    t_start = time.monotonic()
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    from bench import stress_config, free_port

    mc = MockConsul().start()
    for i in range(WATCHES):
        mc.set_health("upstream-%02d" % i,
                      [{"ID": "u-%d" % i, "Address": "10.0.0.1",
                        "Port": 1000 + i}])
    wd = tempfile.mkdtemp(prefix="cpilot-gpu-metrics-")
    port = free_port()
    cfg = stress_config(mc.address, port, JOBS, WATCHES, CHECK_MS,
                        os.path.join(wd, "cp.socket"))
    d = harness.Daemon(config_dict=cfg, workdir=wd)
    try:
        d.start()
        d.wait_for_socket(timeout=30)
        s0 = wait_for_scrape(port)
        time.sleep(2)
        s1 = scrape(port)

        counting = [k for k in s0 if k[0] == "containerpilot_events"
                    or k[0].startswith(DISPATCH)
                    and not k[0].endswith("_sum")]
        assert len(counting) > 13, counting
        for key in counting:
            assert s1[key] >= s0[key], (key, s0[key], s1[key])
        published = [sum(v for k, v in s.items()
                         if k[0] == "containerpilot_events")
                     for s in (s0, s1)]
        dispatched = [s[(DISPATCH + "_count", ())] for s in (s0, s1)]
        print("events %d -> %d, dispatches %d -> %d"
              % (published[0], published[1], dispatched[0], dispatched[1]))
        # 20 checks at 10/s, two events each, over 2 s is 800: half is asked
        assert published[1] - published[0] >= JOBS * 10 * 2
        assert dispatched[1] - dispatched[0] >= JOBS * 10 * 2

        status, _ = d.control("POST", "/v3/reload")
        assert status == 200
        time.sleep(0.3)
        d.wait_for_socket(timeout=30)
        s2 = wait_for_scrape(port)
        # internal collectors live on across generations
        for key in s1:
            if key[0] == DISPATCH + "_bucket" or key[0] == DISPATCH + "_count":
                assert s2[key] >= s1[key], (key, s1[key], s2[key])
        print("after reload: dispatches %d" % s2[(DISPATCH + "_count", ())])

        d.terminate()
        assert d.wait(timeout=60) == 0, d.log()[-4000:]
    finally:
        d.cleanup()
        mc.stop()
    assert time.monotonic() - t_start < 15
