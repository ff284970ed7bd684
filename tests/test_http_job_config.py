"""Config rules of http jobs (`jobs[].http`) through the full config
pipeline: the accepted shapes, every refusal by its text, and that
`health.http` keeps its own, narrower rules."""

import json

import pytest

from containerpilot_amd import native

URL = "http://127.0.0.1:8000/hook"
# what the config loader puts before a job's error
PREFIX = "unable to parse jobs: "
NO_DNS = ("host '%s' is not an IP literal: names are not resolved on the "
          "reactor (use an IP address or 'localhost', or a health.exec check "
          "where DNS is needed)")
OWN = "'%s' is set by the daemon and cannot be configured"
METHODS = ("must be one of 'GET', 'HEAD', 'POST', 'PUT', 'PATCH' or "
           "'DELETE'")


def validate(*jobs):
    return native.validate_config(json.dumps(
        {"consul": "localhost:8500", "jobs": list(jobs)}))


def job(http, **extra):
    out = {"name": "act", "http": http}
    out.update(extra)
    return out


APP = {"name": "app", "exec": "sleep 1"}

ACCEPTED = [
    job(URL),
    job("http://[::1]:8001/tick", when={"interval": "30s"}),
    job("http://localhost"),
    job({"url": "http://localhost:9090/-/reload", "method": "POST"},
        when={"source": "watch.targets", "each": "changed"}),
    job({"url": "http://127.0.0.1:8000/drain", "method": "POST",
         "headers": {"Content-Type": "application/json"},
         "body": "{\"grace\": 10}", "expect": [200, 202]},
        timeout="15s", when={"source": "app", "once": "stopping"}),
    job({"url": URL, "method": "PUT", "body": "x" * 65536}),
    job({"url": URL, "method": "PATCH", "body": ""}),
    job({"url": URL, "method": "DELETE", "body": "gone", "expect": 204}),
    job({"url": URL, "method": "HEAD", "headers": None}),
    job({"url": URL, "body": None}),
    job(URL, restarts="never"),
    job(URL, restarts=0),
    job(URL, restarts=3, when={"interval": "1s"}),
    job(URL, restarts="unlimited", when={"interval": "1s"}, timeout="500ms"),
    job(URL, stopTimeout="3s", when={"source": "app", "each": "exitFailed"}),
]


@pytest.mark.parametrize("spec", ACCEPTED,
                         ids=[str(i) for i in range(len(ACCEPTED))])
def test_accepted(spec):
    assert validate(APP, spec) is None


REFUSED = [
    (job(7), "job[act].http: must be a URL string or an object"),
    (job({"url": URL, "retries": 2}), "job[act].http: invalid keys: retries"),
    (job({"method": "POST"}),
     "job[act].http.url: is required and must be a string"),
    (job({"url": ""}), "job[act].http.url: is required and must be a string"),
    (job("https://127.0.0.1/"),
     "job[act].http: https is not supported: TLS checks are not run on the "
     "reactor (use a health.exec check instead)"),
    (job({"url": "unix:///run/app.sock"}),
     "job[act].http.url: malformed URL 'unix:///run/app.sock': expected "
     "http://HOST[:PORT][/path]"),
    (job({"url": "http://prometheus:9090/-/reload"}),
     "job[act].http.url: " + NO_DNS % "prometheus"),
    (job("http://example.com/"), "job[act].http: " + NO_DNS % "example.com"),
    (job({"url": "http://127.0.0.1:0/"}),
     "job[act].http.url: port '0' must be a number between 1 and 65535"),
    (job({"url": "http://127.0.0.1:65536/"}),
     "job[act].http.url: port '65536' must be a number between 1 and 65535"),
    (job({"url": "http://::1/"}),
     "job[act].http.url: malformed URL 'http://::1/': IPv6 literals must be "
     "bracketed, as in [::1]:8080"),
    (job({"url": "http://127.0.0.1/a#b"}),
     "job[act].http.url: malformed URL 'http://127.0.0.1/a#b': whitespace, "
     "control characters and fragments are not allowed"),
    (job({"url": URL, "method": "TRACE"}), "job[act].http.method: " + METHODS),
    (job({"url": URL, "method": "post"}), "job[act].http.method: " + METHODS),
    (job({"url": URL, "method": 3}), "job[act].http.method: " + METHODS),
    (job({"url": URL, "expect": 99}),
     "job[act].http.expect: entries must be between 100 and 599, got 99"),
    (job({"url": URL, "expect": [200, 600]}),
     "job[act].http.expect: entries must be between 100 and 599, got 600"),
    (job({"url": URL, "expect": []}),
     "job[act].http.expect: must not be an empty list"),
    (job({"url": URL, "expect": "200"}),
     "job[act].http.expect: must be an int or a list of ints"),
    (job({"url": URL, "headers": ["a"]}),
     "job[act].http.headers: must be an object of strings"),
    (job({"url": URL, "headers": {"A": 1}}),
     "job[act].http.headers: must be an object of strings"),
    (job({"url": URL, "headers": {"A": "x\r\nB: y"}}),
     "job[act].http.headers: names and values must not contain CR or LF"),
    (job({"url": URL, "headers": {"A\n": "x"}}),
     "job[act].http.headers: names and values must not contain CR or LF"),
    (job({"url": URL, "headers": {"A:": "x"}}),
     "job[act].http.headers: names must be non-empty and free of ':' and "
     "whitespace"),
    (job({"url": URL, "headers": {"Host": "x"}}),
     "job[act].http.headers: " + OWN % "Host"),
    (job({"url": URL, "headers": {"connection": "keep-alive"}}),
     "job[act].http.headers: " + OWN % "connection"),
    (job({"url": URL, "method": "POST", "headers": {"CONTENT-LENGTH": "3"}}),
     "job[act].http.headers: " + OWN % "CONTENT-LENGTH"),
    (job({"url": URL, "method": "POST",
          "headers": {"Transfer-Encoding": "chunked"}}),
     "job[act].http.headers: " + OWN % "Transfer-Encoding"),
    (job({"url": URL, "method": "POST", "body": 5}),
     "job[act].http.body: must be a string"),
    (job({"url": URL, "method": "POST", "body": {"grace": 10}}),
     "job[act].http.body: must be a string"),
    (job({"url": URL, "body": "x"}),
     "job[act].http.body: cannot be sent with method 'GET': use POST, PUT, "
     "PATCH or DELETE"),
    (job({"url": URL, "method": "HEAD", "body": "x"}),
     "job[act].http.body: cannot be sent with method 'HEAD': use POST, PUT, "
     "PATCH or DELETE"),
    (job({"url": URL, "method": "POST", "body": "x" * 65537}),
     "job[act].http.body: must be at most 65536 bytes, got 65537"),
    # what an http job excludes
    (job(URL, exec="true"), "job[act].http cannot be combined with 'exec'"),
    (job(URL, signal={"job": "app", "send": "HUP"}),
     "job[act].http cannot be combined with 'signal'"),
    (job(URL, port=80),
     "job[act].http cannot be combined with 'port': an http job starts no "
     "process"),
    (job(URL, health={"exec": "true", "interval": 1, "ttl": 2}),
     "job[act].http cannot be combined with 'health': an http job starts no "
     "process"),
    (job(URL, logging={"raw": True}),
     "job[act].http cannot be combined with 'logging': an http job starts "
     "no process"),
    # restarts need an interval to pace them
    (job(URL, restarts=3),
     "job[act].http cannot be combined with restarts '3' unless "
     "'when.interval' is set"),
    (job(URL, restarts="unlimited",
         when={"source": "app", "once": "healthy"}),
     "job[act].http cannot be combined with restarts 'unlimited' unless "
     "'when.interval' is set"),
    (job(URL, timeout="0s"), "job[act].timeout '0s' cannot be less than 1ms"),
    (job(URL, timeout="soon"), None),
]


@pytest.mark.parametrize("spec,want", REFUSED,
                         ids=[str(i) for i in range(len(REFUSED))])
def test_refused(spec, want):
    err = validate(APP, spec)
    if want is None:
        # the duration parser's own words follow the key
        assert err.startswith(
            PREFIX + "unable to parse job[act].timeout 'soon': ")
    else:
        assert err == PREFIX + want


def test_health_http_keeps_its_rules():
    def check(http):
        return validate({"name": "web", "exec": "sleep 1", "port": 80,
                         "health": {"http": http, "interval": 1, "ttl": 5}})

    assert check({"url": URL, "method": "POST"}) == \
        PREFIX + "job[web].health.http.method: must be 'GET' or 'HEAD'"
    assert check({"url": URL, "body": "x"}) == \
        PREFIX + "job[web].health.http: invalid keys: body"
    # a check may still set a Host of its own
    assert check({"url": URL, "headers": {"Host": "web.internal"}}) is None
    assert check({"url": URL, "method": "HEAD"}) is None
