"""ctypes bindings to the in-tree native library (_native.so).

These call directly into the same C++ code the daemon runs (template
engine, JSON5 parser, duration rules, config validation).
"""

import ctypes
import json
import os

from . import REPO_ROOT

_LIB_PATH = os.path.join(REPO_ROOT, "containerpilot_amd", "_native.so")
_lib = None


def _load():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                "native library missing: %s (run __graft_entry__.build())"
                % _LIB_PATH)
        _lib = ctypes.CDLL(_LIB_PATH)
        _lib.cp_version.restype = ctypes.c_char_p
        _lib.cp_render_template.restype = ctypes.c_void_p
        _lib.cp_render_template.argtypes = [
            ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        _lib.cp_parse_duration_ns.restype = ctypes.c_longlong
        _lib.cp_parse_duration_ns.argtypes = [ctypes.c_char_p]
        _lib.cp_parse_duration.restype = ctypes.c_int
        _lib.cp_parse_duration.argtypes = [
            ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong)]
        _lib.cp_render_data.restype = ctypes.c_void_p
        _lib.cp_render_data.argtypes = [
            ctypes.c_char_p, ctypes.c_char_p,
            ctypes.POINTER(ctypes.c_void_p)]
        _lib.cp_json5_to_json.restype = ctypes.c_void_p
        _lib.cp_json5_to_json.argtypes = [
            ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        _lib.cp_validate_config.restype = ctypes.c_void_p
        _lib.cp_validate_config.argtypes = [ctypes.c_char_p]
        _lib.cp_consul_endpoint.restype = ctypes.c_void_p
        _lib.cp_consul_endpoint.argtypes = [
            ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        _lib.cp_watch_render.restype = ctypes.c_void_p
        _lib.cp_watch_render.argtypes = [
            ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
            ctypes.c_char_p, ctypes.c_char_p,
            ctypes.POINTER(ctypes.c_void_p)]
        _lib.cp_kv_decode.restype = ctypes.c_void_p
        _lib.cp_kv_decode.argtypes = [
            ctypes.c_char_p, ctypes.c_size_t,
            ctypes.POINTER(ctypes.c_void_p)]
        _lib.cp_kv_render.restype = ctypes.c_void_p
        _lib.cp_kv_render.argtypes = [
            ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t,
            ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int,
            ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t),
            ctypes.POINTER(ctypes.c_void_p)]
        _lib.cp_sensor_extract.restype = ctypes.c_int
        _lib.cp_sensor_extract.argtypes = [
            ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p,
            ctypes.POINTER(ctypes.c_double),
            ctypes.POINTER(ctypes.c_void_p)]
        _lib.cp_signal_number.restype = ctypes.c_int
        _lib.cp_signal_number.argtypes = [
            ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        _lib.cp_http_action_request.restype = ctypes.c_void_p
        _lib.cp_http_action_request.argtypes = [
            ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t),
            ctypes.POINTER(ctypes.c_void_p)]
        _lib.cp_metrics_replay.restype = ctypes.c_void_p
        _lib.cp_metrics_replay.argtypes = [
            ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        _lib.cp_metric_value_string.restype = ctypes.c_void_p
        _lib.cp_metric_value_string.argtypes = [
            ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
        _lib.cp_free.argtypes = [ctypes.c_void_p]
    return _lib


def _take_string(lib, ptr):
    if not ptr:
        return None
    out = ctypes.string_at(ptr).decode()
    lib.cp_free(ptr)
    return out


def version():
    return _load().cp_version().decode()


def render_template(text):
    lib = _load()
    err = ctypes.c_void_p()
    out = lib.cp_render_template(text.encode(), ctypes.byref(err))
    if not out:
        raise ValueError(_take_string(lib, err.value))
    return _take_string(lib, out)


def parse_duration_ns(text):
    ns = _load().cp_parse_duration_ns(text.encode())
    if ns < 0:
        raise ValueError("invalid duration: %s" % text)
    return ns


def parse_duration(text):
    """Like parse_duration_ns, but negative durations are values too: returns
    the nanoseconds (any int64) or raises ValueError."""
    ns = ctypes.c_longlong()
    if not _load().cp_parse_duration(text.encode(), ctypes.byref(ns)):
        raise ValueError("invalid duration: %s" % text)
    return ns.value


def render_data(template_text, data_json):
    """Render a data template (the language of a watch's `render` file)
    against the JSON document `data_json`. Raises ValueError on a bad
    document or a template error."""
    lib = _load()
    err = ctypes.c_void_p()
    out = lib.cp_render_data(template_text.encode(), data_json.encode(),
                             ctypes.byref(err))
    if not out:
        raise ValueError(_take_string(lib, err.value))
    return _take_string(lib, out)


def json5_to_json(text):
    lib = _load()
    err = ctypes.c_void_p()
    out = lib.cp_json5_to_json(text.encode(), ctypes.byref(err))
    if not out:
        raise ValueError(_take_string(lib, err.value))
    return _take_string(lib, out)


def validate_config(text):
    """Returns None when valid, else the error message."""
    lib = _load()
    return _take_string(lib, lib.cp_validate_config(text.encode()))


def consul_endpoint(consul_json):
    """Resolve the consul endpoint "scheme://host:port" the given consul
    config value produces under the current CONSUL_* environment.

    Note: the CONSUL_* env vars are read by the calling process's own
    environment, so tests set os.environ before calling.
    """
    lib = _load()
    err = ctypes.c_void_p()
    out = lib.cp_consul_endpoint(consul_json.encode(), ctypes.byref(err))
    if not out:
        raise ValueError(_take_string(lib, err.value))
    return _take_string(lib, out)


def sensor_extract(body, record_json):
    """Dry-run of one `telemetry.sensors[].record` entry: the float the
    daemon would record for the source text `body` (str or bytes), scale
    applied. Raises ValueError with the stable reason the daemon would log
    (bytes that are not UTF-8 are shown as U+FFFD), or with the config
    error of a bad record."""
    lib = _load()
    if isinstance(body, str):
        body = body.encode()
    err = ctypes.c_void_p()
    value = ctypes.c_double()
    if not lib.cp_sensor_extract(body, len(body), record_json.encode(),
                                 ctypes.byref(value), ctypes.byref(err)):
        reason = ctypes.string_at(err.value).decode(errors="replace")
        lib.cp_free(err.value)
        raise ValueError(reason)
    return value.value


def signal_number(name):
    """The number of a signal that `jobs[].signal.send`, POST /v3/signal and
    `-signal` accept ("SIGHUP" or "HUP"). Raises ValueError, listing the
    accepted names, for any other name."""
    lib = _load()
    err = ctypes.c_void_p()
    signo = lib.cp_signal_number(name.encode(), ctypes.byref(err))
    if signo < 0:
        raise ValueError(_take_string(lib, err.value))
    return signo


def http_action_request(job_json):
    """The exact bytes the http job `job_json` (one entry of `jobs`, as JSON
    text) writes to its target: request line, headers and body. Raises
    ValueError with the config error of a refused job, or for a job that
    has no `http`."""
    lib = _load()
    err = ctypes.c_void_p()
    size = ctypes.c_size_t()
    out = lib.cp_http_action_request(job_json.encode(), ctypes.byref(size),
                                     ctypes.byref(err))
    if not out:
        raise ValueError(_take_string(lib, err.value))
    request = ctypes.string_at(out, size.value)
    lib.cp_free(out)
    return request


def watch_render(template_text, health_body_json, name, tag="", dc=""):
    """Dry-run of a watch's `render`: what the daemon would write for the
    raw /v1/health/service response body `health_body_json` of service
    `name`. Raises ValueError on a bad body or a template error."""
    lib = _load()
    err = ctypes.c_void_p()
    out = lib.cp_watch_render(template_text.encode(),
                              health_body_json.encode(), name.encode(),
                              tag.encode(), dc.encode(), ctypes.byref(err))
    if not out:
        raise ValueError(_take_string(lib, err.value))
    return _take_string(lib, out)


def kv_decode(body):
    """Decode a /v1/kv response body (str or bytes) the way a key watch
    does: a list of {"Key", "ValueHex", "Flags"} sorted by key, the value
    as hex so it stays byte-exact. Raises ValueError on what the daemon
    treats as a failed query."""
    lib = _load()
    if isinstance(body, str):
        body = body.encode()
    err = ctypes.c_void_p()
    out = lib.cp_kv_decode(body, len(body), ctypes.byref(err))
    if not out:
        raise ValueError(_take_string(lib, err.value))
    return json.loads(_take_string(lib, out))


def kv_render(template_text, body, name, key, prefix=False, dc=""):
    """Dry-run of a key watch's `render`: the bytes the daemon would write
    for the raw /v1/kv response body `body` (str or bytes; None stands for
    the 404 of a missing key) of watch `name` on `key`, or on the prefix
    `key` when `prefix` is set. Returns bytes, since values pass through
    unchanged. Raises ValueError on a bad body or a template error."""
    lib = _load()
    if isinstance(body, str):
        body = body.encode()
    err = ctypes.c_void_p()
    size = ctypes.c_size_t()
    out = lib.cp_kv_render(template_text.encode(), body,
                           len(body) if body is not None else 0,
                           name.encode(), key.encode(), int(bool(prefix)),
                           dc.encode(), ctypes.byref(size), ctypes.byref(err))
    if not out:
        raise ValueError(_take_string(lib, err.value))
    rendered = ctypes.string_at(out, size.value)
    lib.cp_free(out)
    return rendered


def metrics_replay(script_json):
    """Replay a script against the daemon's own metrics path in a registry
    of its own and return the /metrics text. The script (JSON text) has
    `metrics` (entries as in `telemetry.metrics`) with `events` (a list of
    "name|value" strings, each offered to every metric as the bus would),
    and for the internal-collector path `families` ({name, help, type,
    labels, buckets}) with `ops` ({family, op: inc | set | observe |
    setBuckets, labels, value, bounds}). Raises ValueError with the config
    error of a refused metric, or on a malformed script."""
    lib = _load()
    err = ctypes.c_void_p()
    out = lib.cp_metrics_replay(script_json.encode(), ctypes.byref(err))
    if not out:
        raise ValueError(_take_string(lib, err.value))
    return _take_string(lib, out)


def metric_value_string(json_text):
    """The value text `POST /v3/metric` records for one JSON value."""
    lib = _load()
    err = ctypes.c_void_p()
    out = lib.cp_metric_value_string(json_text.encode(), ctypes.byref(err))
    if not out:
        raise ValueError(_take_string(lib, err.value))
    return _take_string(lib, out)
