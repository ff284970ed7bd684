"""The bytes an http job writes, `native.http_action_request`, against a few
lines of Python that build them from the same JSON."""

import json

import pytest

from containerpilot_amd import native


def expected(http):
    """Request line, the daemon's own headers, the configured ones in the
    order written, a blank line, the body."""
    if isinstance(http, str):
        http = {"url": http}
    method = http.get("method", "GET")
    rest = http["url"][len("http://"):]
    cut = min([i for i in (rest.find("/"), rest.find("?")) if i >= 0],
              default=len(rest))
    authority, target = rest[:cut], rest[cut:]
    if not target.startswith("/"):
        target = "/" + target
    body = http.get("body")
    lines = ["%s %s HTTP/1.1" % (method, target),
             "Host: " + authority,
             "User-Agent: containerpilot/" + native.version(),
             "Accept: */*",
             "Connection: close"]
    if body is not None or method in ("POST", "PUT", "PATCH"):
        lines.append("Content-Length: %d" % len((body or "").encode()))
    lines += ["%s: %s" % kv for kv in (http.get("headers") or {}).items()]
    return ("\r\n".join(lines) + "\r\n\r\n").encode() + (body or "").encode()


def request(http):
    return native.http_action_request(json.dumps({"name": "act",
                                                  "http": http}))


SPECS = [
    "http://127.0.0.1:8000/tick",
    "http://localhost",
    "http://[::1]:8001/tick",
    {"url": "http://[fe80::1]/", "method": "HEAD"},
    "http://127.0.0.1:9090?probe=1",
    {"url": "http://127.0.0.1:9090/-/reload?force=1&why=a%20b",
     "method": "POST"},
    {"url": "http://127.0.0.1/x", "method": "PUT"},
    {"url": "http://127.0.0.1/x", "method": "PATCH", "body": ""},
    {"url": "http://127.0.0.1/x", "method": "DELETE"},
    {"url": "http://127.0.0.1/x", "method": "DELETE", "body": "gone"},
    {"url": "http://127.0.0.1:8000/drain", "method": "POST",
     "headers": {"Content-Type": "application/json", "X-Zed": "1",
                 "Authorization": "Bearer t", "accept": "text/plain"},
     "body": "{\"grace\": 10}", "expect": [200, 202]},
    {"url": "http://127.0.0.1/x", "method": "POST", "body": "a\x00b\x00"},
    {"url": "http://127.0.0.1/x", "method": "POST",
     "headers": {"Content-Type": "text/plain; charset=utf-8"},
     "body": "grüße 世界 \U0001f600\r\n"},
    {"url": "http://127.0.0.1/x", "method": "PUT", "body": "x" * 65536},
    {"url": "http://127.0.0.1/x", "method": "PUT",
     "body": "é" * 32768},
]


@pytest.mark.parametrize("http", SPECS,
                         ids=[str(i) for i in range(len(SPECS))])
def test_request_bytes(http):
    got = request(http)
    assert isinstance(got, bytes)
    assert got == expected(http)


def test_body_limit_counts_bytes():
    with pytest.raises(ValueError) as e:
        request({"url": "http://127.0.0.1/x", "method": "PUT",
                 "body": "x" * 65537})
    assert str(e.value) == \
        "job[act].http.body: must be at most 65536 bytes, got 65537"
    # 32769 two-byte characters are 65538 bytes
    with pytest.raises(ValueError) as e:
        request({"url": "http://127.0.0.1/x", "method": "PUT",
                 "body": "é" * 32769})
    assert str(e.value) == \
        "job[act].http.body: must be at most 65536 bytes, got 65538"


def test_config_errors_are_raised():
    with pytest.raises(ValueError) as e:
        request({"url": "http://127.0.0.1/x", "body": "x"})
    assert str(e.value) == (
        "job[act].http.body: cannot be sent with method 'GET': use POST, "
        "PUT, PATCH or DELETE")
    with pytest.raises(ValueError) as e:
        native.http_action_request(json.dumps({"name": "act",
                                               "exec": "true"}))
    assert str(e.value) == "job[act] has no 'http'"


def test_health_http_request_is_unchanged():
    """The probe request of a spec without body and with GET is what the
    same spec gives as an action: no Content-Length crept in."""
    got = request({"url": "http://127.0.0.1:80/h", "headers": {"A": "b"}})
    assert got == (b"GET /h HTTP/1.1\r\nHost: 127.0.0.1:80\r\n"
                   b"User-Agent: containerpilot/" +
                   native.version().encode() +
                   b"\r\nAccept: */*\r\nConnection: close\r\nA: b\r\n\r\n")
