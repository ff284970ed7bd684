"""Key watches (`watches[].key`, `watches[].keyPrefix`): the daemon against
MockConsul's /v1/kv. A key watch publishes from `watch.<name>` like a
service watch, "healthy" meaning that the key exists, and renders its file
before the events of the result the file is about."""

import json
import os
import socket
import urllib.request

from test_watch_render import job_outputs, read_file, wait_until

KEY = "myapp/config/mode"
TEMPLATE = ("{{ if .Exists }}mode = {{ .Value }}\n"
            "{{ else }}# mode is not set\n{{ end }}")
MISSING = "# mode is not set\n"

PREFIX = "myapp/vhosts/"
LIST_TEMPLATE = ("{{ range .Keys }}{{ .Rel }} = {{ .Value }}\n{{ end }}"
                 "# {{ len .Keys }} vhosts\n")


def rendering(value):
    return MISSING if value is None else "mode = %s\n" % value.decode()


def listing(kv):
    return ("".join("%s = %s\n" % (k[len(PREFIX):], v.decode())
                    for k, v in sorted(kv.items())) +
            "# %d vhosts\n" % len(kv))


def kv_queries(mock_consul, prefix="/v1/kv/"):
    with mock_consul.lock:
        return [path for method, path in mock_consul.requests
                if method == "GET" and path.startswith(prefix)]


def events(d, code, name="mode"):
    return d.log().count("{%s watch.%s}" % (code, name))


def parked(mock_consul):
    """A blocking query that asks with consul's current index is waiting."""
    wanted = "index=%d&" % mock_consul.index
    return any(wanted in path for path in kv_queries(mock_consul))


def handled(mock_consul):
    """With a long-poll parked, the predicate "the daemon has asked again":
    by then the result that woke it has been handled."""
    assert wait_until(lambda: parked(mock_consul)), kv_queries(mock_consul)
    before = len(kv_queries(mock_consul))
    return lambda: len(kv_queries(mock_consul)) > before


def kv_config(mock_consul, watch, onchange_exec, name="mode"):
    return {
        "consul": mock_consul.address,
        "stopTimeout": 1,
        "logging": {"level": "DEBUG"},
        "jobs": [
            {"name": "main-app", "exec": "sleep 60"},
            {"name": "onchange", "exec": onchange_exec,
             "when": {"source": "watch." + name, "each": "changed"}},
        ],
        "watches": [watch],
    }


def start_daemon(daemon_factory, mock_consul, tmp_path, template=TEMPLATE,
                 watch=None, onchange_exec=None, **kwargs):
    """A daemon with one key watch (by default a blocking one on KEY whose
    interval is too long for polling to matter) that renders `template` to
    tmp_path/mode.conf; returns (daemon, dest) once the first rendering is
    on disk."""
    source = str(tmp_path / "mode.ctmpl")
    with open(source, "w") as f:
        f.write(template)
    dest = str(tmp_path / "mode.conf")
    watch = dict(watch or {"name": "mode", "key": KEY, "interval": 30,
                           "blocking": True})
    watch["render"] = {"source": source, "dest": dest}
    d = daemon_factory(kv_config(mock_consul, watch,
                                 onchange_exec or ["cat", dest],
                                 name=watch["name"]), **kwargs).start()
    d.wait_for_socket()
    assert wait_until(lambda: read_file(dest) is not None), d.log()
    return d, dest


def check_kv_ordering(d, mock_consul, dest, key=KEY):
    """Three set_kv and a delete_kv: after each, the onChange job's
    `cat <dest>` has logged exactly that value's rendering."""
    changes = [b"blue", b"green", b"red", None]
    for n, value in enumerate(changes, start=1):
        if value is None:
            mock_consul.delete_kv(key)
        else:
            mock_consul.set_kv(key, value)
        want = rendering(value)

        def logged():
            outputs = job_outputs(d.log())
            return len(outputs) >= n and outputs[n - 1] == want

        assert wait_until(logged), (n, want, job_outputs(d.log()),
                                    d.log()[-3000:])
        assert read_file(dest) == want
    assert len(job_outputs(d.log())) == len(changes)
    assert events(d, "StatusChanged") == 4
    assert events(d, "StatusHealthy") == 3
    assert events(d, "StatusUnhealthy") == 1
    log = d.log()
    assert log.rindex("{StatusUnhealthy watch.mode}") > \
        log.rindex("{StatusHealthy watch.mode}")
    assert "{Error" not in log


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def telemetry_get(port, path):
    url = "http://127.0.0.1:%d%s" % (port, path)
    with urllib.request.urlopen(url, timeout=10) as resp:
        return resp.read().decode()


def finish(d):
    d.terminate()
    assert d.wait(timeout=30) == 0, d.log()[-3000:]


def test_first_result_of_a_missing_key(daemon_factory, mock_consul,
                                       tmp_path):
    d, dest = start_daemon(daemon_factory, mock_consul, tmp_path)
    assert read_file(dest) == MISSING
    # the re-issued long-poll is parked: the first result is fully handled
    assert wait_until(lambda: len(kv_queries(mock_consul)) >= 2), d.log()
    assert "watch.mode}" not in d.log()
    assert job_outputs(d.log()) == []
    finish(d)


def test_first_result_of_an_existing_key(daemon_factory, mock_consul,
                                         tmp_path):
    mock_consul.set_kv(KEY, b"blue", flags=42)
    d, dest = start_daemon(
        daemon_factory, mock_consul, tmp_path,
        template=TEMPLATE + "# flags {{ .Flags }}\n")
    want = "mode = blue\n# flags 42\n"
    # `changed` and `healthy`, after the file is in place
    assert wait_until(lambda: job_outputs(d.log()) == [want]), d.log()
    assert read_file(dest) == want
    assert events(d, "StatusChanged") == 1
    assert events(d, "StatusHealthy") == 1
    assert events(d, "StatusUnhealthy") == 0
    finish(d)


def test_once_healthy_starts_a_job_when_the_key_is_there(
        daemon_factory, mock_consul, tmp_path):
    config = kv_config(mock_consul,
                       {"name": "mode", "key": KEY, "interval": 30,
                        "blocking": True}, "true")
    config["jobs"].append({"name": "needs-mode", "exec": "echo mode-is-there",
                           "when": {"source": "watch.mode",
                                    "once": "healthy"}})
    d = daemon_factory(config).start()
    d.wait_for_socket()
    assert wait_until(lambda: len(kv_queries(mock_consul)) >= 2), d.log()
    assert "mode-is-there" not in d.log()
    mock_consul.set_kv(KEY, b"blue")
    assert wait_until(lambda: "mode-is-there" in d.log()), d.log()
    finish(d)


def test_file_is_rendered_before_the_change_events(daemon_factory,
                                                   mock_consul, tmp_path):
    d, dest = start_daemon(daemon_factory, mock_consul, tmp_path)
    check_kv_ordering(d, mock_consul, dest)
    finish(d)


def test_identical_rewrite_is_no_change(daemon_factory, mock_consul,
                                        tmp_path):
    d, dest = start_daemon(daemon_factory, mock_consul, tmp_path)
    mock_consul.set_kv(KEY, b"blue")
    assert wait_until(lambda: read_file(dest) == rendering(b"blue")), d.log()
    assert wait_until(lambda: events(d, "StatusHealthy") == 1)
    before = os.stat(dest)

    # same bytes again: consul's index moves, so the long-poll returns
    asked_again = handled(mock_consul)
    mock_consul.set_kv(KEY, b"blue")
    assert wait_until(asked_again), d.log()
    after = os.stat(dest)
    assert (after.st_ino, after.st_mtime_ns) == (before.st_ino,
                                                 before.st_mtime_ns)
    assert events(d, "StatusChanged") == 1
    assert len(job_outputs(d.log())) == 1

    # the flags alone are a change
    mock_consul.set_kv(KEY, b"blue", flags=1)
    assert wait_until(lambda: events(d, "StatusChanged") == 2), d.log()
    finish(d)


def test_prefix(daemon_factory, mock_consul, tmp_path):
    mock_consul.set_kv("myapp/other", b"outside")
    d, dest = start_daemon(
        daemon_factory, mock_consul, tmp_path, template=LIST_TEMPLATE,
        watch={"name": "vhosts", "keyPrefix": PREFIX, "interval": 30,
               "blocking": True})
    assert read_file(dest) == listing({})
    kv = {}
    steps = [("set", PREFIX + "b", b"beta"),     # added
             ("set", PREFIX + "a", b"alpha"),    # added before it
             ("set", PREFIX + "c/d", b"deep"),   # nested
             ("set", PREFIX + "b", b"BETA"),     # changed
             ("delete", PREFIX + "a", None)]     # removed
    for n, (op, key, value) in enumerate(steps, start=1):
        if op == "set":
            kv[key] = value
            mock_consul.set_kv(key, value)
        else:
            del kv[key]
            mock_consul.delete_kv(key)
        want = listing(kv)

        def logged():
            outputs = job_outputs(d.log())
            return len(outputs) >= n and outputs[n - 1] == want

        assert wait_until(logged), (n, want, job_outputs(d.log()),
                                    d.log()[-3000:])
        assert read_file(dest) == want
        # each fires once
        assert events(d, "StatusChanged", "vhosts") == n
    assert read_file(dest) == "b = BETA\nc/d = deep\n# 2 vhosts\n"

    # a key outside the prefix wakes the long-poll and fires nothing
    asked_again = handled(mock_consul)
    mock_consul.set_kv("myapp/other", b"still outside")
    assert wait_until(asked_again), d.log()
    assert events(d, "StatusChanged", "vhosts") == len(steps)
    assert len(job_outputs(d.log())) == len(steps)
    assert events(d, "StatusUnhealthy", "vhosts") == 0

    # the last key gone: unhealthy
    mock_consul.delete_kv(PREFIX + "b")
    mock_consul.delete_kv(PREFIX + "c/d")
    assert wait_until(
        lambda: events(d, "StatusUnhealthy", "vhosts") == 1), d.log()
    assert wait_until(lambda: read_file(dest) == listing({}))
    finish(d)


def test_polling_sees_a_change(daemon_factory, mock_consul, tmp_path):
    d, dest = start_daemon(
        daemon_factory, mock_consul, tmp_path,
        watch={"name": "mode", "key": KEY, "interval": 1})
    assert read_file(dest) == MISSING
    mock_consul.set_kv(KEY, b"polled")
    assert wait_until(
        lambda: job_outputs(d.log()) == [rendering(b"polled")]), d.log()
    assert events(d, "StatusHealthy") == 1
    # polled queries carry neither index nor wait
    assert set(kv_queries(mock_consul)) == {"/v1/kv/" + KEY}
    finish(d)


def test_exact_requests(daemon_factory, mock_consul):
    d = daemon_factory({
        "consul": {"address": mock_consul.address, "token": "kv-token"},
        "stopTimeout": 1,
        "jobs": [{"name": "main-app", "exec": "sleep 60"}],
        "watches": [
            {"name": "single", "key": "myapp/config/my mode?#%",
             "interval": 1},
            {"name": "vhosts", "keyPrefix": PREFIX, "interval": 1,
             "dc": "dc2"},
            {"name": "parked", "key": "myapp/parked", "interval": 30,
             "blocking": True, "dc": "dc3"},
            {"name": "parked-prefix", "keyPrefix": "café/", "interval": 30,
             "blocking": True},
        ],
    }, env={"CONSUL_HTTP_TOKEN": ""}).start()
    d.wait_for_socket()
    index = str(mock_consul.index)
    want = {
        "/v1/kv/myapp/config/my%20mode%3F%23%25",
        "/v1/kv/myapp/vhosts/?recurse=true&dc=dc2",
        "/v1/kv/myapp/parked?dc=dc3&index=0&wait=10s",
        "/v1/kv/myapp/parked?dc=dc3&index=" + index + "&wait=10s",
        "/v1/kv/caf%C3%A9/?recurse=true&index=0&wait=10s",
        "/v1/kv/caf%C3%A9/?recurse=true&index=" + index + "&wait=10s",
    }
    assert wait_until(lambda: set(kv_queries(mock_consul)) >= want), \
        (kv_queries(mock_consul), d.log())
    assert set(kv_queries(mock_consul)) == want
    with mock_consul.lock:
        assert mock_consul.tokens
        assert set(mock_consul.tokens) == {"kv-token"}
    finish(d)


def test_failed_query_keeps_the_state(daemon_factory, mock_consul, tmp_path):
    mock_consul.set_kv(KEY, b"blue")
    d, dest = start_daemon(
        daemon_factory, mock_consul, tmp_path,
        watch={"name": "mode", "key": KEY, "interval": 1, "blocking": True})
    assert wait_until(lambda: job_outputs(d.log()) == [rendering(b"blue")])
    assert wait_until(lambda: len(kv_queries(mock_consul)) >= 2)
    before = os.stat(dest)

    # every request fails from here on; another key wakes the parked
    # long-poll, whose re-issue then meets the failure
    mock_consul.fail_mode = True
    mock_consul.set_kv("myapp/other", b"wake")
    assert wait_until(
        lambda: "failed to query key " + KEY in d.log()), d.log()
    mock_consul.set_kv(KEY, b"green")  # pending while consul is down
    # a second failure: the first one's back-off (interval) has run out
    assert wait_until(
        lambda: d.log().count("failed to query key") >= 2), d.log()
    after = os.stat(dest)
    assert (after.st_ino, after.st_mtime_ns) == (before.st_ino,
                                                 before.st_mtime_ns)
    assert read_file(dest) == rendering(b"blue")
    assert events(d, "StatusChanged") == 1
    assert events(d, "StatusUnhealthy") == 0
    assert "{Error" not in d.log()

    mock_consul.fail_mode = False
    assert wait_until(lambda: job_outputs(d.log()) == [
        rendering(b"blue"), rendering(b"green")]), d.log()
    assert read_file(dest) == rendering(b"green")
    assert events(d, "StatusChanged") == 2
    finish(d)


def test_body_over_the_cap_is_a_failed_query(daemon_factory, mock_consul,
                                             tmp_path):
    # nine values of 512 KiB, Consul's own limit for one: about 6 MiB of
    # base64 in one response
    for n in range(9):
        mock_consul.set_kv("big/%d" % n, bytes([65 + n]) * (512 * 1024))
    source = tmp_path / "big.ctmpl"
    source.write_text("{{ len .Keys }} keys\n")
    dest = str(tmp_path / "big.conf")
    config = kv_config(
        mock_consul,
        {"name": "big", "keyPrefix": "big/", "interval": 1, "blocking": True,
         "render": {"source": str(source), "dest": dest}},
        "echo onchange-ran", name="big")
    # the text format shows the level
    config["logging"] = {"level": "DEBUG", "format": "text"}
    d = daemon_factory(config).start()
    d.wait_for_socket()
    assert wait_until(
        lambda: 'level=warning msg="failed to query key big/"' in d.log()), \
        d.log()
    assert read_file(dest) is None
    assert "watch.big}" not in d.log()
    # under the cap again: the retry after `interval` gets through
    for n in range(4, 9):
        mock_consul.delete_kv("big/%d" % n)
    assert wait_until(lambda: read_file(dest) == "4 keys\n"), d.log()
    assert wait_until(lambda: "onchange-ran" in d.log())
    assert events(d, "StatusChanged", "big") == 1
    finish(d)


def test_reload_and_terminate_do_not_wait_for_a_parked_long_poll(
        daemon_factory, mock_consul, tmp_path):
    mock_consul.set_kv(KEY, b"blue")
    d, dest = start_daemon(daemon_factory, mock_consul, tmp_path)
    assert wait_until(lambda: events(d, "StatusHealthy") == 1)
    # parked: asked with the index of the first answer
    assert wait_until(lambda: any(
        "index=%d" % mock_consul.index in path
        for path in kv_queries(mock_consul))), d.log()

    with open(str(tmp_path / "mode.ctmpl"), "w") as f:
        f.write("edited: {{ .Value }}\n")
    status, _ = d.control("POST", "/v3/reload")
    assert status == 200
    # the new generation's first result renders, and is a change again:
    # the cache starts empty each generation
    assert wait_until(lambda: read_file(dest) == "edited: blue\n"), d.log()
    d.wait_for_socket()
    assert wait_until(lambda: events(d, "StatusHealthy") == 2), d.log()
    assert wait_until(lambda: sum(
        "index=%d" % mock_consul.index in path
        for path in kv_queries(mock_consul)) >= 2), d.log()

    d.terminate()
    assert d.wait() == 0, d.log()[-3000:]


def test_service_and_key_watches_do_not_disturb_each_other(
        daemon_factory, mock_consul):
    mock_consul.set_health("backend", [])
    port = free_port()
    d = daemon_factory({
        "consul": mock_consul.address,
        "stopTimeout": 1,
        "logging": {"level": "DEBUG"},
        "telemetry": {"port": port, "interfaces": ["static:127.0.0.1"]},
        "jobs": [
            {"name": "main-app", "exec": "sleep 60"},
            {"name": "on-backend", "exec": "echo backend-changed",
             "when": {"source": "watch.backend", "each": "changed"}},
            {"name": "on-mode", "exec": "echo mode-changed",
             "when": {"source": "watch.mode", "each": "changed"}},
        ],
        "watches": [
            {"name": "backend", "interval": 30, "blocking": True},
            {"name": "mode", "key": KEY, "interval": 30, "blocking": True},
        ],
    }).start()
    d.wait_for_socket()

    def health_queries():
        with mock_consul.lock:
            return sum(1 for _, path in mock_consul.requests
                       if path.startswith("/v1/health/service/backend"))

    assert wait_until(lambda: health_queries() >= 2 and
                      len(kv_queries(mock_consul)) >= 2), d.log()
    assert "StatusChanged" not in d.log()

    # the mock's single index wakes both long-polls
    queries = health_queries()
    mock_consul.set_kv(KEY, b"blue")
    assert wait_until(lambda: "mode-changed" in d.log()), d.log()
    assert wait_until(lambda: health_queries() > queries), d.log()
    assert events(d, "StatusChanged", "mode") == 1
    assert events(d, "StatusChanged", "backend") == 0

    asked_again = handled(mock_consul)
    mock_consul.set_health("backend", [
        {"ID": "b-1", "Address": "10.0.0.1", "Port": 9000}])
    assert wait_until(lambda: "backend-changed" in d.log()), d.log()
    assert wait_until(asked_again), d.log()
    assert events(d, "StatusChanged", "mode") == 1
    assert events(d, "StatusChanged", "backend") == 1
    assert events(d, "StatusHealthy", "backend") == 1
    assert d.log().count("mode-changed") == 1

    # /status lists both by name; the instances gauge knows services only
    assert json.loads(telemetry_get(port, "/status"))["Watches"] == [
        "backend", "mode"]
    metrics = telemetry_get(port, "/metrics")
    assert 'containerpilot_watch_instances{service="backend"} 1' in metrics
    assert 'service="mode"' not in metrics
    finish(d)


def test_duplicate_name_is_refused_at_start(daemon_factory, mock_consul):
    d = daemon_factory({
        "consul": mock_consul.address,
        "jobs": [{"name": "main-app", "exec": "sleep 60"}],
        "watches": [{"name": "mode", "interval": 3},
                    {"name": "mode", "key": KEY, "interval": 3}],
    }).start()
    assert d.wait(timeout=30) != 0
    assert ("watch[mode]: a key watch must not share its name with another "
            "watch") in d.log()
