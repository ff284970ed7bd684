"""Config rules of key watches (`watches[].key`, `watches[].keyPrefix`)
through native.validate_config: shape only, as for `render`."""

import json

import pytest

from containerpilot_amd import native

PREFIX = "unable to parse watches: "


def validate(*watches):
    return native.validate_config(json.dumps(
        {"consul": "localhost:8500", "watches": list(watches)}))


def kw(**fields):
    watch = {"name": "mode", "interval": 5}
    watch.update(fields)
    return watch


ACCEPTED = [
    kw(key="myapp/config/mode"),
    kw(key="myapp/config/mode", blocking=True, dc="dc2",
       render={"source": "/etc/app/mode.ctmpl", "dest": "/etc/app/mode.conf"}),
    kw(keyPrefix="myapp/vhosts/"),
    kw(keyPrefix="myapp/vhosts/", interval=10, dc="dc2", blocking=True),
    kw(key="a" * 512),
    kw(key="café/a b/50%/what?/#1"),
    kw(key="a//b/"),
    # null counts as not given: a service watch, where tag is fine
    kw(key=None, keyPrefix=None, tag="blue"),
    kw(key="a", keyPrefix=None, tag=None),
]


@pytest.mark.parametrize("watch", ACCEPTED,
                         ids=[str(n) for n in range(len(ACCEPTED))])
def test_accepted(watch):
    assert validate(watch) is None


REFUSED = [
    (kw(key="a", keyPrefix="a/"),
     "watch[mode]: key and keyPrefix are mutually exclusive"),
    (kw(key=""), "watch[mode].key must be a non-empty string"),
    (kw(key=7), "watch[mode].key must be a non-empty string"),
    (kw(key=["a"]), "watch[mode].key must be a non-empty string"),
    (kw(keyPrefix=""), "watch[mode].keyPrefix must be a non-empty string"),
    (kw(keyPrefix=True), "watch[mode].keyPrefix must be a non-empty string"),
    (kw(key="a" * 513), "watch[mode].key must be at most 512 bytes"),
    # 512 is a limit in bytes: 257 two-byte characters are 514
    (kw(key="é" * 257), "watch[mode].key must be at most 512 bytes"),
    (kw(keyPrefix="a/" * 257),
     "watch[mode].keyPrefix must be at most 512 bytes"),
    (kw(key="/myapp/mode"), "watch[mode].key must not start with '/'"),
    (kw(keyPrefix="/"), "watch[mode].keyPrefix must not start with '/'"),
    (kw(key="a\tb"), "watch[mode].key must not contain control characters"),
    (kw(key="a\nb"), "watch[mode].key must not contain control characters"),
    (kw(key="a\u0000b"),
     "watch[mode].key must not contain control characters"),
    (kw(key="a\u001fb"),
     "watch[mode].key must not contain control characters"),
    (kw(keyPrefix="a\u007f"),
     "watch[mode].keyPrefix must not contain control characters"),
    (kw(key="a", tag="blue"), "watch[mode].tag does not apply to a key watch"),
    (kw(keyPrefix="a/", tag=""),
     "watch[mode].tag does not apply to a key watch"),
    # the shared options keep their rules
    (kw(key="a", interval=0), "watch[mode].interval must be > 0"),
    (kw(key="a", blocking="maybe"), "watch[mode].blocking must be a bool"),
    (kw(key="a", render={"source": "/a", "dest": "b"}),
     "watch[mode].render.dest must be an absolute path"),
]


@pytest.mark.parametrize("watch,error", REFUSED,
                         ids=[str(n) for n in range(len(REFUSED))])
def test_refused(watch, error):
    assert validate(watch) == PREFIX + error


def test_name_is_still_a_service_name():
    err = validate(kw(name="Bad_Name", key="a"))
    assert err is not None and err.startswith(PREFIX + "service names must")


def test_unknown_keys_are_still_refused():
    assert validate(kw(key="a", keys="b")) == (
        PREFIX + "Watch configuration error: invalid keys: keys")


DUPLICATE = ("watch[mode]: a key watch must not share its name with another "
             "watch")


def test_a_key_watch_shares_its_name_with_nobody():
    service = {"name": "mode", "interval": 3}
    assert validate(kw(key="a"), service) == PREFIX + DUPLICATE
    assert validate(service, kw(keyPrefix="a/")) == PREFIX + DUPLICATE
    assert validate(kw(key="a"), kw(key="b")) == PREFIX + DUPLICATE
    assert validate(kw(key="a"), kw(name="other", key="a")) is None
    # two service watches with one name keep what they did
    assert validate(service, dict(service, tag="blue")) is None
