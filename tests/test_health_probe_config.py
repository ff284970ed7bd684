"""Validation of the native health checks (`health.tcp`, `health.http`)
through the daemon's own config code (native.validate_config)."""

import json
import os

import pytest

from containerpilot_amd import REPO_ROOT, native


def config(health, name="web"):
    health = dict(health)
    health.setdefault("interval", 1)
    health.setdefault("ttl", 5)
    return json.dumps({
        "consul": "localhost:8500",
        "jobs": [{"name": name, "exec": "sleep 60", "port": 8000,
                  "interfaces": ["static:10.1.2.3"], "health": health}],
    })


def error_for(health):
    err = native.validate_config(config(health))
    assert err is not None, "accepted: %r" % (health,)
    return err


ERROR_CASES = [
    # more than one of exec / http / tcp
    ({"exec": "true", "tcp": "127.0.0.1:80"},
     ["job[web].health can have only one of 'exec', 'http', or 'tcp'"]),
    ({"http": "http://127.0.0.1/", "tcp": "127.0.0.1:80"},
     ["job[web].health can have only one of 'exec', 'http', or 'tcp'"]),
    ({"exec": "true", "http": "http://127.0.0.1/", "tcp": "127.0.0.1:80"},
     ["can have only one of"]),
    # port outside 1-65535
    ({"tcp": "127.0.0.1:0"},
     ["job[web].health.tcp", "between 1 and 65535"]),
    ({"tcp": "127.0.0.1:65536"},
     ["job[web].health.tcp", "between 1 and 65535"]),
    ({"tcp": "127.0.0.1:http"},
     ["job[web].health.tcp", "between 1 and 65535"]),
    ({"tcp": "127.0.0.1"}, ["job[web].health.tcp", "missing port"]),
    ({"http": "http://127.0.0.1:70000/"},
     ["job[web].health.http", "between 1 and 65535"]),
    ({"http": {"url": "http://127.0.0.1:0/"}},
     ["job[web].health.http.url", "between 1 and 65535"]),
    # names are never resolved on the reactor
    ({"tcp": "db.internal:5432"},
     ["job[web].health.tcp", "names are not resolved on the reactor",
      "health.exec"]),
    ({"http": "http://example.com/health"},
     ["job[web].health.http", "names are not resolved on the reactor",
      "health.exec"]),
    ({"tcp": "::1:80"}, ["job[web].health.tcp", "must be bracketed"]),
    ({"tcp": "[::zz]:80"}, ["job[web].health.tcp", "IPv6 literal"]),
    # TLS is out of scope
    ({"http": "https://127.0.0.1/health"},
     ["job[web].health.http", "https is not supported", "health.exec"]),
    # malformed URLs
    ({"http": "127.0.0.1:8000/health"},
     ["job[web].health.http", "malformed URL"]),
    ({"http": "http:///health"}, ["job[web].health.http", "malformed URL"]),
    ({"http": "http://127.0.0.1/a b"},
     ["job[web].health.http", "malformed URL"]),
    ({"http": "ftp://127.0.0.1/"}, ["job[web].health.http", "malformed URL"]),
    ({"http": {"method": "GET"}}, ["job[web].health.http.url"]),
    ({"http": 8000}, ["job[web].health.http", "URL string or an object"]),
    # unknown key inside the http object
    ({"http": {"url": "http://127.0.0.1/", "body": "x"}},
     ["job[web].health.http", "body"]),
    # method
    ({"http": {"url": "http://127.0.0.1/", "method": "POST"}},
     ["job[web].health.http.method", "'GET' or 'HEAD'"]),
    ({"http": {"url": "http://127.0.0.1/", "method": "get"}},
     ["job[web].health.http.method", "'GET' or 'HEAD'"]),
    # expect
    ({"http": {"url": "http://127.0.0.1/", "expect": 99}},
     ["job[web].health.http.expect", "between 100 and 599"]),
    ({"http": {"url": "http://127.0.0.1/", "expect": [200, 600]}},
     ["job[web].health.http.expect", "between 100 and 599"]),
    ({"http": {"url": "http://127.0.0.1/", "expect": "200"}},
     ["job[web].health.http.expect", "int or a list of ints"]),
    # header injection
    ({"http": {"url": "http://127.0.0.1/",
               "headers": {"X-A": "ok\r\nX-Evil: 1"}}},
     ["job[web].health.http.headers", "CR or LF"]),
    ({"http": {"url": "http://127.0.0.1/", "headers": {"X-A\nX-B": "v"}}},
     ["job[web].health.http.headers", "CR or LF"]),
    ({"http": {"url": "http://127.0.0.1/", "headers": {"X-A": "v\n"}}},
     ["job[web].health.http.headers", "CR or LF"]),
    ({"http": {"url": "http://127.0.0.1/", "headers": {"X-A": 1}}},
     ["job[web].health.http.headers", "strings"]),
    # health.logging belongs to exec checks only
    ({"tcp": "127.0.0.1:80", "logging": {"raw": True}},
     ["job[web].health.logging", "only applies to 'exec'"]),
    ({"http": "http://127.0.0.1/", "logging": {"raw": False}},
     ["job[web].health.logging", "only applies to 'exec'"]),
]


@pytest.mark.parametrize("health,needles", ERROR_CASES,
                         ids=[json.dumps(c[0])[:60] for c in ERROR_CASES])
def test_rejected(health, needles):
    err = error_for(health)
    for needle in needles:
        assert needle in err, err


VALID_CASES = [
    {"tcp": "127.0.0.1:8000"},
    {"tcp": "localhost:1"},
    {"tcp": "[::1]:65535"},
    {"http": "http://localhost:8000/health"},
    {"http": "http://10.0.0.7"},
    {"http": "http://[::1]:8080/ready?deep=1&x=y"},
    {"http": "http://127.0.0.1?only=query"},
    {"http": {"url": "http://127.0.0.1:8000/health"}},
    {"http": {"url": "http://127.0.0.1:8000/health", "method": "HEAD",
              "headers": {"X-Token": "a b", "Authorization": "Bearer z"},
              "expect": [200, 204]}},
    {"http": {"url": "http://127.0.0.1/", "expect": 404}},
    {"http": "http://127.0.0.1/", "timeout": "250ms", "interval": "500ms"},
    # the exec form is untouched, logging included
    {"exec": "true", "logging": {"raw": True}},
]


@pytest.mark.parametrize("health", VALID_CASES,
                         ids=[json.dumps(c)[:60] for c in VALID_CASES])
def test_accepted(health):
    assert native.validate_config(config(health)) is None


def test_error_names_the_job():
    err = native.validate_config(config({"tcp": "nope:1"}, name="cache"))
    assert err is not None and "job[cache].health.tcp" in err


def test_native_example_validates():
    path = os.path.join(REPO_ROOT, "docs", "examples", "native-health.json5")
    with open(path) as f:
        rendered = native.render_template(f.read())
    assert native.validate_config(rendered) is None
    doc = json.loads(native.json5_to_json(rendered))
    kinds = [k for job in doc["jobs"] for k in ("http", "tcp", "exec")
             if k in job.get("health", {})]
    assert kinds == ["http", "http", "tcp"]
