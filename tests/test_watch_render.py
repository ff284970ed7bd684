"""Native rendering of a watch's upstream file (`watches[].render`): the
daemon writes the healthy set through a template into `dest`, atomically,
before it publishes the change events for that set — so an onChange job
always finds the file for the set its event is about."""

import glob
import json
import os
import re
import shutil
import threading
import time

from containerpilot_amd import native

TEMPLATE = ("# begin\n"
            "{{ range .Services }}server {{ .Address }}:{{ .Port }};\n"
            "{{ end }}# end {{ len .Services }}\n")

ONE = [{"ID": "b-1", "Address": "10.0.0.1", "Port": 9000}]
# given in reverse address order on purpose
TWO = [{"ID": "b-2", "Address": "10.0.0.2", "Port": 9000},
       {"ID": "b-1", "Address": "10.0.0.1", "Port": 9000}]


def wait_until(predicate, timeout=10.0, interval=0.02):
    deadline = time.time() + timeout
    while time.time() < deadline:
        if predicate():
            return True
        time.sleep(interval)
    return False


def rendering(entries):
    """What TEMPLATE renders for `entries`: sorted by (Address, Port, ID)."""
    rows = sorted(entries, key=lambda e: (e["Address"], e["Port"], e["ID"]))
    return ("# begin\n" +
            "".join("server %s:%d;\n" % (e["Address"], e["Port"])
                    for e in rows) +
            "# end %d\n" % len(rows))


def job_outputs(log, job="onchange"):
    """The logged stdout of each run of `job`, oldest first. The daemon
    logs a job's output as `<time> <job> <pid> <line>`."""
    runs = {}
    pattern = re.compile(r"^\S+ %s (\d+) (.*)$" % re.escape(job))
    for line in log.splitlines():
        m = pattern.match(line)
        if m:
            runs.setdefault(m.group(1), []).append(m.group(2))
    return ["".join(text + "\n" for text in lines) for lines in runs.values()]


def read_file(path):
    try:
        with open(path) as f:
            return f.read()
    except OSError:
        return None


def render_config(mock_consul, source, dest, onchange_exec):
    return {
        "consul": mock_consul.address,
        "stopTimeout": 1,
        "logging": {"level": "DEBUG"},
        "jobs": [
            {"name": "main-app", "exec": "sleep 60"},
            {"name": "onchange", "exec": onchange_exec,
             "when": {"source": "watch.backend", "each": "changed"}},
        ],
        # interval 30: only the blocking query can notice a change within
        # the time these tests wait
        "watches": [{"name": "backend", "interval": 30, "blocking": True,
                     "render": {"source": source, "dest": dest}}],
    }


def start_daemon(daemon_factory, mock_consul, tmp_path, onchange_exec=None,
                 dest=None, template=TEMPLATE, **kwargs):
    """A daemon watching `backend` (empty at first) that renders TEMPLATE
    to tmp_path/upstreams.conf; returns (daemon, dest) once the first
    rendering is on disk."""
    source = str(tmp_path / "upstreams.ctmpl")
    with open(source, "w") as f:
        f.write(template)
    dest = dest or str(tmp_path / "upstreams.conf")
    mock_consul.set_health("backend", [])
    d = daemon_factory(render_config(mock_consul, source, dest,
                                     onchange_exec or ["cat", dest]),
                       **kwargs).start()
    d.wait_for_socket()
    assert wait_until(lambda: read_file(dest) is not None), d.log()
    return d, dest


def check_ordering(d, mock_consul, dest, changes):
    """After each change, the onChange job's `cat <dest>` must have logged
    the rendering of exactly that set."""
    for n, entries in enumerate(changes, start=1):
        mock_consul.set_health("backend", entries)
        want = rendering(entries)

        def logged():
            outputs = job_outputs(d.log())
            return len(outputs) >= n and outputs[n - 1] == want

        assert wait_until(logged), (n, want, job_outputs(d.log()),
                                    d.log()[-3000:])
        assert read_file(dest) == want
    assert len(job_outputs(d.log())) == len(changes)


def health_queries(mock_consul):
    with mock_consul.lock:
        return sum(1 for method, path in mock_consul.requests
                   if method == "GET" and
                   path.startswith("/v1/health/service/backend"))


def test_first_result_renders_the_empty_set(daemon_factory, mock_consul,
                                            tmp_path):
    d, dest = start_daemon(daemon_factory, mock_consul, tmp_path)
    assert read_file(dest) == "# begin\n# end 0\n"
    assert os.stat(dest).st_mode & 0o7777 == 0o644
    # the re-issued long-poll is parked: the first result is fully handled
    assert wait_until(lambda: health_queries(mock_consul) >= 2)
    assert "StatusChanged" not in d.log()
    assert job_outputs(d.log()) == []
    d.terminate()
    assert d.wait(timeout=30) == 0


def test_file_is_rendered_before_the_change_events(daemon_factory,
                                                   mock_consul, tmp_path):
    d, dest = start_daemon(daemon_factory, mock_consul, tmp_path)
    check_ordering(d, mock_consul, dest, [ONE, TWO, []])
    assert d.log().count("{StatusChanged watch.backend}") == 3
    assert "{Error" not in d.log()
    d.terminate()
    assert d.wait(timeout=30) == 0


def test_unchanged_set_leaves_the_file_alone(daemon_factory, mock_consul,
                                             tmp_path):
    d, dest = start_daemon(daemon_factory, mock_consul, tmp_path)
    mock_consul.set_health("backend", TWO)
    assert wait_until(lambda: read_file(dest) == rendering(TWO)), d.log()
    assert wait_until(
        lambda: d.log().count("{StatusChanged watch.backend}") == 1)
    before = os.stat(dest)

    # same entries again: consul's index moves, so the long-poll returns.
    # Once the daemon has asked again, that result has been handled.
    queries = health_queries(mock_consul)
    mock_consul.set_health("backend", list(TWO))
    assert wait_until(lambda: health_queries(mock_consul) > queries), d.log()
    after = os.stat(dest)
    assert (after.st_ino, after.st_mtime_ns) == (before.st_ino,
                                                 before.st_mtime_ns)
    assert d.log().count("{StatusChanged watch.backend}") == 1
    d.terminate()
    assert d.wait(timeout=30) == 0


def test_readers_never_see_a_partial_file(daemon_factory, mock_consul,
                                          tmp_path):
    d, dest = start_daemon(daemon_factory, mock_consul, tmp_path,
                           onchange_exec="true")
    small = ONE
    large = [{"ID": "b-%d" % i, "Address": "10.0.1.%d" % i, "Port": 9000}
             for i in range(1, 41)]
    seen = set()
    broken = []
    done = threading.Event()

    def reader():
        while not done.is_set():
            text = read_file(dest)
            if text is None:
                continue
            servers = text.count("server ")
            if (text.startswith("# begin\n") and
                    text.endswith("# end %d\n" % servers)):
                seen.add(text)
            else:
                broken.append(text)

    thread = threading.Thread(target=reader, daemon=True)
    thread.start()
    try:
        for flip in range(20):
            entries = large if flip % 2 == 0 else small
            mock_consul.set_health("backend", entries)
            assert wait_until(
                lambda: read_file(dest) == rendering(entries)), \
                (flip, d.log()[-2000:])
    finally:
        done.set()
        thread.join(timeout=10)
    assert broken == []
    assert len(seen) >= 2, seen
    assert seen <= {rendering([]), rendering(small), rendering(large)}
    d.terminate()
    assert d.wait(timeout=30) == 0


def test_render_failure_is_reported_and_events_still_flow(
        daemon_factory, mock_consul, tmp_path):
    confd = tmp_path / "conf.d"
    confd.mkdir()
    d, dest = start_daemon(daemon_factory, mock_consul, tmp_path,
                           onchange_exec="echo onchange-ran",
                           dest=str(confd / "upstreams.conf"))
    shutil.rmtree(str(confd))
    mock_consul.set_health("backend", ONE)
    assert wait_until(lambda: "onchange-ran" in d.log()), d.log()
    log = d.log()
    # logged as an error, and published on the bus before the usual events
    error_lines = [line for line in log.splitlines()
                   if "watch.backend: render: " in line]
    assert any("event:" not in line for line in error_lines), log
    assert "No such file or directory" in error_lines[0]
    error_at = log.index("event: {Error watch.backend: render: ")
    assert error_at < log.index("{StatusChanged watch.backend}")
    assert "{StatusHealthy watch.backend}" in log
    # nothing left behind: no resurrected directory, no temporary file
    assert not confd.exists()
    assert glob.glob(str(tmp_path / "**" / "*.tmp*"), recursive=True) == []
    d.terminate()
    assert d.wait(timeout=30) == 0


def test_template_execution_error_keeps_the_previous_file(
        daemon_factory, mock_consul, tmp_path):
    # .Name is a string: fine while there is nothing to range over in the
    # first branch, an execution error once the set is healthy
    template = ("{{ if .Healthy }}{{ range .Name }}x{{ end }}"
                "{{ else }}nothing up\n{{ end }}")
    d, dest = start_daemon(daemon_factory, mock_consul, tmp_path,
                           onchange_exec="echo onchange-ran",
                           template=template)
    assert read_file(dest) == "nothing up\n"
    mock_consul.set_health("backend", ONE)
    assert wait_until(lambda: "onchange-ran" in d.log()), d.log()
    assert ("event: {Error watch.backend: render: template: range over "
            "non-list value}") in d.log()
    assert read_file(dest) == "nothing up\n"
    d.terminate()
    assert d.wait(timeout=30) == 0


def test_bad_template_fails_the_start(daemon_factory, mock_consul, tmp_path):
    source = tmp_path / "upstreams.ctmpl"
    source.write_text("# begin\n{{ range .Services }}server {{ .Address \n")
    dest = str(tmp_path / "upstreams.conf")
    d = daemon_factory(render_config(mock_consul, str(source), dest,
                                     ["cat", dest])).start()
    assert d.wait(timeout=30) != 0
    assert "watch[backend].render.source: template: unclosed action" \
        in d.log()
    assert not os.path.exists(dest)


def test_reload_picks_up_the_edited_template(daemon_factory, mock_consul,
                                             tmp_path):
    d, dest = start_daemon(daemon_factory, mock_consul, tmp_path)
    assert read_file(dest) == rendering([])
    with open(str(tmp_path / "upstreams.ctmpl"), "w") as f:
        f.write("edited: {{ len .Services }} up\n")
    status, _ = d.control("POST", "/v3/reload")
    assert status == 200
    # the set is still empty and unchanged: it is the new generation's
    # first result that renders
    assert wait_until(lambda: read_file(dest) == "edited: 0 up\n"), d.log()
    assert "StatusChanged" not in d.log()
    d.wait_for_socket(timeout=15)
    mock_consul.set_health("backend", ONE)
    assert wait_until(lambda: read_file(dest) == "edited: 1 up\n"), d.log()
    d.terminate()
    assert d.wait(timeout=30) == 0


def test_native_watch_render_and_validate_config():
    body = json.dumps([
        {"Node": {"Node": "n2", "Address": "192.168.0.2"},
         "Service": {"ID": "b-2", "Service": "backend",
                     "Address": "10.0.0.2", "Port": 9000,
                     "Tags": ["blue", "v2"]},
         "Checks": []},
        # no Service.Address: consul means the node's address
        {"Node": {"Node": "n1", "Address": "10.0.0.1"},
         "Service": {"ID": "b-1", "Service": "backend", "Address": "",
                     "Port": 9001, "Tags": []},
         "Checks": []},
    ])
    assert native.watch_render(TEMPLATE, body, "backend") == (
        "# begin\nserver 10.0.0.1:9001;\nserver 10.0.0.2:9000;\n# end 2\n")
    assert native.watch_render(
        "{{ .Name }}/{{ .Tag }}/{{ .DC }}/{{ .Healthy }}:"
        "{{ range .Services }} {{ .ID }}@{{ .Node }}({{ .NodeAddress }})"
        "[{{ join \",\" .Tags }}]{{ end }}",
        body, "backend", tag="blue", dc="dc1") == (
        "backend/blue/dc1/true: b-1@n1(10.0.0.1)[] "
        "b-2@n2(192.168.0.2)[blue,v2]")
    assert native.watch_render(TEMPLATE, "[]", "backend") == rendering([])

    for bad_template in ("{{ range .Services }}", "{{ range .Name }}{{ end }}"):
        try:
            native.watch_render(bad_template, body, "backend")
        except ValueError as e:
            assert "template:" in str(e)
        else:
            raise AssertionError("accepted " + bad_template)

    config = {
        "consul": "localhost:8500",
        "watches": [{"name": "backend", "interval": 3, "blocking": True,
                     "render": {"source": "/etc/nginx/upstreams.ctmpl",
                                "dest": "/etc/nginx/conf.d/upstreams.conf",
                                "mode": "0644"}}],
    }
    # text only: neither file has to exist
    assert native.validate_config(json.dumps(config)) is None
    config["watches"][0]["render"]["dest"] = "conf.d/upstreams.conf"
    assert native.validate_config(json.dumps(config)) == (
        "unable to parse watches: watch[backend].render.dest must be an "
        "absolute path")
