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
     CPILOT_CAPACITY_SENSORS = native | exec (default unset): instead of
     the stress shape, feed N gauges from N files (the arguments are
     source counts, default 50) every CPILOT_CAPACITY_SENSOR_MS (1000)
     and report CPU seconds per 1000 samples of the daemon plus all its
     descendants. native uses `telemetry.sensors`; exec is the only way
     without them: one periodic job per source running a script that
     reads the file and execs `containerpilot -putmetric`.
     CPILOT_CAPACITY_SIGNALS = native | exec (default unset): instead of
     the stress shape, N periodic jobs (the arguments are job counts,
     default 10) each send SIGHUP to one supervised target every
     CPILOT_CAPACITY_SIGNAL_MS (100); reports CPU seconds per 1000
     deliveries of the daemon plus all its descendants. native uses
     `jobs[].signal`; exec is the only way without it: a job running
     `/bin/sh -c 'kill -HUP $CONTAINERPILOT_NGINX_PID'`.
     CPILOT_CAPACITY_HTTPJOBS = native | exec (default unset): instead of
     the stress shape, N periodic jobs (the arguments are job counts,
     default 10) each POST to one bin/cpilot_probesink every
     CPILOT_CAPACITY_HTTPJOB_MS (100); reports CPU seconds per 1000
     actions, of the daemon process alone and of the daemon plus all its
     descendants. native uses `jobs[].http`; exec is the only way without
     it: a job running `curl --fail -s -XPOST`. Without a `curl` on the
     machine the exec side is skipped, and says so.
"""
import json
import os
import re
import shutil
import stat
import sys
import tempfile
import time
import urllib.request

sys.path.insert(0, os.getcwd())
from containerpilot_amd import BINARY, harness  # noqa: E402
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


def tree_cpu_seconds(root):
    """CPU time of `root` and every live descendant, each with the
    children it has already reaped (cutime + cstime), so short-lived
    grandchildren count once their parent has waited for them."""
    children = {}
    times = {}
    for entry in os.listdir("/proc"):
        if not entry.isdigit():
            continue
        try:
            with open("/proc/%s/stat" % entry) as f:
                fields = f.read().rpartition(")")[2].split()
        except OSError:
            continue  # exited while we were listing
        children.setdefault(int(fields[1]), []).append(int(entry))
        times[int(entry)] = sum(int(x) for x in fields[11:15])
    total, todo = 0, [root]
    while todo:
        pid = todo.pop()
        total += times.get(pid, 0)
        todo.extend(children.get(pid, []))
    return total / TICKS_PER_SEC


def sensor_capacity(mode, sources, every_ms):
    wd = tempfile.mkdtemp()
    port = free_port()
    socket_path = os.path.join(wd, "cp.socket")
    config_path = os.path.join(wd, "containerpilot.json5")
    metrics, sensors, jobs = [], [], []
    for i in range(sources):
        path = os.path.join(wd, "source-%03d" % i)
        with open(path, "w") as f:
            f.write("%d\n" % (1000 + i))
        key = "cap_src_v%03d" % i
        metrics.append({"namespace": "cap", "subsystem": "src",
                        "name": "v%03d" % i, "type": "gauge", "help": "v"})
        if mode == "native":
            sensors.append({"name": "src-%03d" % i, "file": path,
                            "interval": "%dms" % every_ms,
                            "record": [{"metric": key}]})
        else:
            script = os.path.join(wd, "sensor-%03d.sh" % i)
            with open(script, "w") as f:
                f.write('#!/bin/sh\nexec %s -config %s -putmetric '
                        '"%s=$(cat %s)"\n' % (BINARY, config_path, key, path))
            os.chmod(script, os.stat(script).st_mode | stat.S_IXUSR)
            jobs.append({"name": "sensor-%03d" % i, "exec": script,
                         "when": {"interval": "%dms" % every_ms}})
    telemetry = {"port": port, "interfaces": ["static:127.0.0.1"],
                 "metrics": metrics}
    if sensors:
        telemetry["sensors"] = sensors
    d = harness.Daemon(config_dict={
        "consul": "localhost:79", "stopTimeout": 1,
        "logging": {"level": "ERROR"}, "control": {"socket": socket_path},
        "jobs": jobs, "telemetry": telemetry}, workdir=wd)
    d.start()
    d.wait_for_socket(timeout=60)

    def samples():
        url = "http://127.0.0.1:%d/metrics" % port
        with urllib.request.urlopen(url, timeout=10) as resp:
            text = resp.read().decode()
        if mode == "native":
            pattern = (r'^containerpilot_sensor_samples\{sensor="[^"]*",'
                       r'result="ok"\} (\S+)$')
        else:
            pattern = (r'^containerpilot_control_http_requests\{code="200",'
                       r'path="/v3/metric"\} (\S+)$')
        return sum(float(v) for v in re.findall(pattern, text, re.M))

    time.sleep(warmup)
    n0, c0, t0 = samples(), tree_cpu_seconds(d.proc.pid), time.time()
    time.sleep(window)
    n1, c1, el = samples(), tree_cpu_seconds(d.proc.pid), time.time() - t0
    print(json.dumps({
        "sensors": mode,
        "sources": sources,
        "interval_ms": every_ms,
        "window_sec": round(el, 2),
        "samples": round(n1 - n0),
        "samples_per_sec": round((n1 - n0) / el, 1),
        "tree_cpu_sec": round(c1 - c0, 3),
        "cpu_sec_per_1000_samples":
            round(1000.0 * (c1 - c0) / (n1 - n0), 4) if n1 > n0 else None,
    }), flush=True)
    d.cleanup()


def signal_capacity(mode, count, every_ms):
    wd = tempfile.mkdtemp()
    port = free_port()
    # the target handles SIGHUP and otherwise idles: its cost is the same
    # in both modes
    jobs = [{"name": "nginx",
             "exec": ["/bin/sh", "-c",
                      "trap : HUP; while :; do sleep 1; done"]}]
    for i in range(count):
        job = {"name": "reload-%03d" % i,
               "when": {"interval": "%dms" % every_ms}}
        if mode == "native":
            job["signal"] = {"job": "nginx", "send": "SIGHUP"}
        else:
            job["exec"] = ["/bin/sh", "-c",
                           "kill -HUP $CONTAINERPILOT_NGINX_PID"]
        jobs.append(job)
    d = harness.Daemon(config_dict={
        "consul": "localhost:79", "stopTimeout": 1,
        "logging": {"level": "ERROR"}, "jobs": jobs,
        "telemetry": {"port": port, "interfaces": ["static:127.0.0.1"]}},
        workdir=wd)
    d.start()
    d.wait_for_socket(timeout=60)

    def deliveries():
        url = "http://127.0.0.1:%d/metrics" % port
        with urllib.request.urlopen(url, timeout=10) as resp:
            text = resp.read().decode()
        pattern = (r'^containerpilot_events\{code="ExitSuccess",'
                   r'source="reload-\d+"\} (\S+)$')
        return sum(float(v) for v in re.findall(pattern, text, re.M))

    time.sleep(warmup)
    n0, c0, t0 = deliveries(), tree_cpu_seconds(d.proc.pid), time.time()
    time.sleep(window)
    n1, c1, el = deliveries(), tree_cpu_seconds(d.proc.pid), time.time() - t0
    print(json.dumps({
        "signals": mode,
        "jobs": count,
        "interval_ms": every_ms,
        "window_sec": round(el, 2),
        "deliveries": round(n1 - n0),
        "deliveries_per_sec": round((n1 - n0) / el, 1),
        "tree_cpu_sec": round(c1 - c0, 3),
        "cpu_sec_per_1000_deliveries":
            round(1000.0 * (c1 - c0) / (n1 - n0), 4) if n1 > n0 else None,
    }), flush=True)
    d.cleanup()


def httpjob_capacity(mode, count, every_ms):
    curl = shutil.which("curl")
    if mode == "exec" and not curl:
        print(json.dumps({"httpjobs": "exec", "skipped": "no curl here"}),
              flush=True)
        return
    wd = tempfile.mkdtemp()
    port = free_port()
    # the sink answers with a length and closes: its cost is the same in
    # both modes and it is no descendant of the daemon
    sink = harness.ProbeSink("http200").start()
    url = "http://127.0.0.1:%d/-/reload" % sink.port
    jobs = []
    for i in range(count):
        job = {"name": "reload-%03d" % i,
               "when": {"interval": "%dms" % every_ms}}
        if mode == "native":
            job["http"] = {"url": url, "method": "POST"}
        else:
            job["exec"] = [curl, "--fail", "-s", "-o", "/dev/null",
                           "-XPOST", url]
        jobs.append(job)
    d = harness.Daemon(config_dict={
        "consul": "localhost:79", "stopTimeout": 1,
        "logging": {"level": "ERROR"}, "jobs": jobs,
        "telemetry": {"port": port, "interfaces": ["static:127.0.0.1"]}},
        workdir=wd)
    d.start()
    d.wait_for_socket(timeout=60)

    def actions():
        target = "http://127.0.0.1:%d/metrics" % port
        with urllib.request.urlopen(target, timeout=10) as resp:
            text = resp.read().decode()
        pattern = (r'^containerpilot_events\{code="ExitSuccess",'
                   r'source="reload-\d+"\} (\S+)$')
        return sum(float(v) for v in re.findall(pattern, text, re.M))

    def cpu():
        return cpu_seconds(d.proc.pid), tree_cpu_seconds(d.proc.pid)

    time.sleep(warmup)
    n0, (c0, tree0), t0 = actions(), cpu(), time.time()
    time.sleep(window)
    n1, (c1, tree1), el = actions(), cpu(), time.time() - t0

    def per_1000(seconds):
        return round(1000.0 * seconds / (n1 - n0), 4) if n1 > n0 else None

    print(json.dumps({
        "httpjobs": mode,
        "jobs": count,
        "interval_ms": every_ms,
        "window_sec": round(el, 2),
        "actions": round(n1 - n0),
        "actions_per_sec": round((n1 - n0) / el, 1),
        "daemon_cpu_sec": round(c1 - c0, 3),
        "tree_cpu_sec": round(tree1 - tree0, 3),
        "daemon_cpu_sec_per_1000_actions": per_1000(c1 - c0),
        "tree_cpu_sec_per_1000_actions": per_1000(tree1 - tree0),
    }), flush=True)
    d.cleanup()
    sink.stop()


httpjobs_mode = os.environ.get("CPILOT_CAPACITY_HTTPJOBS")
if httpjobs_mode:
    if httpjobs_mode not in ("native", "exec"):
        sys.exit("CPILOT_CAPACITY_HTTPJOBS must be native or exec")
    every = int(os.environ.get("CPILOT_CAPACITY_HTTPJOB_MS", "100"))
    for count in [int(a) for a in sys.argv[1:]] or [10]:
        httpjob_capacity(httpjobs_mode, count, every)
    sys.exit(0)

signals_mode = os.environ.get("CPILOT_CAPACITY_SIGNALS")
if signals_mode:
    if signals_mode not in ("native", "exec"):
        sys.exit("CPILOT_CAPACITY_SIGNALS must be native or exec")
    every = int(os.environ.get("CPILOT_CAPACITY_SIGNAL_MS", "100"))
    for count in [int(a) for a in sys.argv[1:]] or [10]:
        signal_capacity(signals_mode, count, every)
    sys.exit(0)

sensors_mode = os.environ.get("CPILOT_CAPACITY_SENSORS")
if sensors_mode:
    if sensors_mode not in ("native", "exec"):
        sys.exit("CPILOT_CAPACITY_SENSORS must be native or exec")
    every = int(os.environ.get("CPILOT_CAPACITY_SENSOR_MS", "1000"))
    for count in [int(a) for a in sys.argv[1:]] or [50]:
        sensor_capacity(sensors_mode, count, every)
    sys.exit(0)

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
