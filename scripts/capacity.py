"""Single-daemon capacity probe: scale the stress shape up (more jobs =
more health checks per second) and measure sustained rates + windowed
p99 dispatch latency + the daemon's own CPU time.

Usage: python3 scripts/capacity.py [jobs ...]   (default: 100 300 500)
Env: CPILOT_CAPACITY_WATCHES (default 0), CPILOT_CAPACITY_WINDOW (20s),
     CPILOT_CAPACITY_WARMUP (8s),
     CPILOT_CAPACITY_CHECK = exec | tcp | http (default exec): exec is
     the stress shape as bench.py generates it (a real fork/exec of
     `true` per check); tcp and http start bin/cpilot_probesink and
     rewrite every job's health block to a native probe against it.
     CPILOT_CAPACITY_JOB_EXEC = 1 | 0 (default 1): 0 drops each job's
     supervised `sleep 3600`, leaving only its checks, so job counts
     beyond the machine's process limit can still be measured (the
     sleeps are idle; the row records which shape ran).
"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd())
from containerpilot_amd import harness  # noqa: E402
from bench import stress_config, free_port, scrape, histogram_p99  # noqa: E402

job_counts = [int(a) for a in sys.argv[1:]] or [100, 300, 500]
watches = int(os.environ.get("CPILOT_CAPACITY_WATCHES", "0"))
window = int(os.environ.get("CPILOT_CAPACITY_WINDOW", "20"))
warmup = int(os.environ.get("CPILOT_CAPACITY_WARMUP", "8"))
check = os.environ.get("CPILOT_CAPACITY_CHECK", "exec")
if check not in ("exec", "tcp", "http"):
    sys.exit("CPILOT_CAPACITY_CHECK must be exec, tcp or http")
job_exec = os.environ.get("CPILOT_CAPACITY_JOB_EXEC", "1") != "0"

CHECK_MS = 100
TICKS_PER_SEC = os.sysconf("SC_CLK_TCK")


def cpu_seconds(pid, reactor_only=False):
    """utime + stime of the daemon process itself (children excluded):
    all its threads, or only the main thread, which runs the reactor
    (the rest are the Consul pool and the spawner's reader)."""
    path = "/proc/%d/task/%d/stat" % (pid, pid) if reactor_only \
        else "/proc/%d/stat" % pid
    with open(path) as f:
        # the comm field may contain spaces; fields resume after ')'
        fields = f.read().rpartition(")")[2].split()
    return (int(fields[11]) + int(fields[12])) / TICKS_PER_SEC


for jobs in job_counts:
    wd = tempfile.mkdtemp()
    port = free_port()
    cfg = stress_config("localhost:79", port, jobs, watches, CHECK_MS,
                        os.path.join(wd, "cp.socket"))
    if not job_exec:
        for job in cfg["jobs"]:
            del job["exec"]
    sink = None
    if check != "exec":
        sink = harness.ProbeSink(
            "accept" if check == "tcp" else "http200").start()
        target = "127.0.0.1:%d" % sink.port
        for job in cfg["jobs"]:
            health = {"interval": job["health"]["interval"],
                      "ttl": job["health"]["ttl"]}
            if check == "tcp":
                health["tcp"] = target
            else:
                health["http"] = "http://%s/health" % target
            job["health"] = health
    d = harness.Daemon(config_dict=cfg, workdir=wd)
    d.start()
    d.wait_for_socket(timeout=60)
    time.sleep(warmup)
    s0 = scrape(port)
    c0 = cpu_seconds(d.proc.pid)
    r0 = cpu_seconds(d.proc.pid, reactor_only=True)
    a0 = sink.accepted() if sink else None
    t0 = time.time()
    time.sleep(window)
    s1 = scrape(port)
    c1 = cpu_seconds(d.proc.pid)
    r1 = cpu_seconds(d.proc.pid, reactor_only=True)
    a1 = sink.accepted() if sink else None
    el = time.time() - t0
    pub = (s1["published"] - s0["published"]) / el
    dlv = (s1["delivered"] - s0["delivered"]) / el
    p99 = histogram_p99(s0["buckets"], s1["buckets"])
    print(json.dumps({
        "check": check,
        "jobs": jobs,
        "job_exec": job_exec,
        "checks_per_sec_target": jobs * 10,
        "published_per_sec": round(pub),
        "completion_pct": round(100.0 * pub / (2 * jobs * 10), 1),
        "delivered_per_sec": round(dlv),
        "p99_dispatch_ms": round(p99 * 1000, 3) if p99 else None,
        "daemon_cpu_sec_per_sec": round((c1 - c0) / el, 3),
        "reactor_cpu_sec_per_sec": round((r1 - r0) / el, 3),
        "sink_accepted_per_sec": round((a1 - a0) / el) if sink else None,
    }), flush=True)
    d.cleanup()
    if sink:
        sink.stop()
