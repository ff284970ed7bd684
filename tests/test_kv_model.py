"""Key watches against a table and a model: tests/golden/kv_cases.json is
replayed through native.kv_decode and native.kv_render (the daemon's own
base64 decoder, body parser and template data model), and random values
encoded by Python's base64 module must come back byte for byte. Refused
inputs come from the table only."""

import base64
import json
import os
import random

import pytest

from containerpilot_amd import REPO_ROOT, native

with open(os.path.join(REPO_ROOT, "tests", "golden", "kv_cases.json")) as f:
    CASES = json.load(f)


def body_of(value_text, key="k", flags=0):
    return json.dumps([{"Key": key, "Flags": flags, "Value": value_text}])


def test_table_is_complete():
    assert len(CASES["base64_valid"]) >= 8
    assert len(CASES["base64_refused"]) >= 10
    assert len(CASES["bodies"]) >= 4
    assert len(CASES["bodies_refused"]) >= 4
    assert len(CASES["render"]) >= 6


@pytest.mark.parametrize("row", CASES["base64_valid"],
                         ids=lambda r: r["value"][:12] or "empty")
def test_base64_valid(row):
    assert native.kv_decode(body_of(row["value"])) == [
        {"Key": "k", "ValueHex": row["hex"], "Flags": 0}]


@pytest.mark.parametrize("value", CASES["base64_refused"], ids=repr)
def test_base64_refused(value):
    with pytest.raises(ValueError):
        native.kv_decode(body_of(value))
    # and it fails the whole body when it comes second
    good = {"Key": "a", "Flags": 0, "Value": "QQ=="}
    bad = {"Key": "b", "Flags": 0, "Value": value}
    assert native.kv_decode(json.dumps([good])) == [
        {"Key": "a", "ValueHex": "41", "Flags": 0}]
    with pytest.raises(ValueError):
        native.kv_decode(json.dumps([good, bad]))


@pytest.mark.parametrize("row", CASES["bodies"], ids=lambda r: r["name"])
def test_bodies(row):
    assert native.kv_decode(row["body"]) == row["want"]


@pytest.mark.parametrize("row", CASES["bodies_refused"],
                         ids=lambda r: r["name"])
def test_bodies_refused(row):
    with pytest.raises(ValueError):
        native.kv_decode(row["body"])
    with pytest.raises(ValueError):
        native.kv_render("x", row["body"], "mode", "k")


@pytest.mark.parametrize("row", CASES["render"], ids=lambda r: r["name"])
def test_render(row):
    got = native.kv_render(row["template"], row["body"], row["watch"],
                           row["key"], prefix=row["prefix"], dc=row["dc"])
    assert got == bytes.fromhex(row["wantHex"])


def test_render_reports_template_errors():
    for bad in ("{{ range .Keys }}", "{{ range .Name }}{{ end }}"):
        with pytest.raises(ValueError, match="template:"):
            native.kv_render(bad, None, "mode", "k")


def test_random_values_round_trip():
    """The model is Python's encoder: whatever it encodes, the daemon's
    decoder gives back exactly, one value at a time and many in a body."""
    rng = random.Random(20240611)
    values = [bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 64)))
              for _ in range(400)]
    # every length at least once
    values += [bytes(rng.getrandbits(8) for _ in range(n)) for n in range(65)]
    for value in values:
        got = native.kv_decode(
            body_of(base64.b64encode(value).decode(), flags=len(value)))
        assert got == [{"Key": "k", "ValueHex": value.hex(),
                        "Flags": len(value)}], value
    # one body with all of them, given in reverse key order
    keys = ["p/%04d" % n for n in range(len(values))]
    body = json.dumps([
        {"Key": k, "Flags": 1, "Value": base64.b64encode(v).decode() or None}
        for k, v in reversed(list(zip(keys, values)))])
    assert native.kv_decode(body) == [
        {"Key": k, "ValueHex": v.hex(), "Flags": 1}
        for k, v in zip(keys, values)]
