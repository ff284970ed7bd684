"""Config fidelity against the reference's own test fixture corpus.

The fixtures are the reference's JSON5 config files (settings only, no
program text), stored verbatim under tests/golden/reference_configs/
with the reference's own directory layout, so the tests run from any
checkout. Expected outcomes mirror the reference's own unit tests
(jobs/config_test.go, watches/config_test.go,
telemetry/telemetry_config_test.go).
"""

import json
import os

import pytest

from containerpilot_amd import native

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                   "golden", "reference_configs")


def load(rel):
    with open(os.path.join(REF, rel)) as f:
        return f.read()


def validate_jobs_array(raw_array_text):
    """Wrap a jobs-array fixture in a minimal full config and validate."""
    arr = json.loads(native.json5_to_json(raw_array_text))
    cfg = json.dumps({"consul": "localhost:8500", "jobs": arr})
    return native.validate_config(cfg)


def test_job_smoke_fixture_valid():
    # jobs/config_test.go:TestJobConfigSmokeTest expects this to parse
    err = validate_jobs_array(load("jobs/testdata/TestJobConfigSmokeTest.json5"))
    assert err is None, err


@pytest.mark.parametrize("fixture", [
    "TestJobConfigPeriodicTask",
    "TestJobConfigServiceWithPreStart",
    "TestJobConfigServiceWithStopping",
    "TestJobConfigServiceWithArrayExec",
    "TestJobConfigServiceWithInitialStatus",
    "TestJobConfigConsulExtras",
    "TestJobConfigHealthTimeout",
    "TestJobConfigServiceNonAdvertised",
])
def test_job_fixtures_valid(fixture):
    err = validate_jobs_array(load("jobs/testdata/%s.json5" % fixture))
    assert err is None, "%s: %s" % (fixture, err)


@pytest.mark.parametrize("fixture,why", [
    ("TestErrJobConfigConsulDeregisterCriticalServiceAfter",
     "bad duration 'nope'"),
    ("TestErrJobConfigConsulEnableTagOverride",
     "enableTagOverride must be a bool"),
])
def test_job_fixtures_invalid(fixture, why):
    err = validate_jobs_array(load("jobs/testdata/%s.json5" % fixture))
    assert err is not None, "%s should be rejected (%s)" % (fixture, why)


def test_watches_fixture_valid():
    arr = json.loads(native.json5_to_json(
        load("watches/testdata/TestWatchesParse.json5")))
    cfg = json.dumps({"consul": "localhost:8500", "watches": arr})
    assert native.validate_config(cfg) is None


def test_telemetry_fixture_valid():
    tel = json.loads(native.json5_to_json(
        load("telemetry/testdata/TestTelemetryConfigParse.json5")))
    cfg = json.dumps({"consul": "localhost:8500", "telemetry": tel})
    assert native.validate_config(cfg) is None


def test_app_testcfg_shapes():
    """The config shapes core/app_test.go feeds NewApp."""
    # valid minimal reload config (core/app_test.go:128)
    assert native.validate_config('{ "consul": "newconsul:8500" }') is None
    # missing job name (core/app_test.go:25-30)
    err = native.validate_config(
        '{"consul": "consul:8500", "jobs": ['
        '{"name": "", "port": 8080, '
        '"health": {"interval": 30, "ttl": 19}}]}')
    assert err and "'name' must not be blank" in err
    # missing health interval (core/app_test.go:33-38)
    err = native.validate_config(
        '{"consul": "consul:8500", "jobs": ['
        '{"name": "name", "port": 8080, "health": {"ttl": 19}}]}')
    assert err and "health.interval must be > 0" in err
    # missing ttl
    err = native.validate_config(
        '{"consul": "consul:8500", "jobs": ['
        '{"name": "name", "port": 8080, "health": {"interval": 19}}]}')
    assert err and "health.ttl must be > 0" in err
    # missing watch name (core/app_test.go:51-55)
    err = native.validate_config(
        '{"consul": "consul:8500", "watches": ['
        '{"name": "", "interval": 30}]}')
    assert err and "'name' must not be blank" in err
    # missing watch interval
    err = native.validate_config(
        '{"consul": "consul:8500", "watches": [{"name": "name"}]}')
    assert err and "interval must be > 0" in err



class TestReferenceDocsExamples:
    """Run the reference's own docs example configs
    (docs/30-configuration/examples/*.json5) through our
    render+validate pipeline and pin the exact outcome of each.

    Notably, most of those examples are broken in the reference's OWN
    pipeline too (missing JSON5 commas, `health` without `interval` —
    which jobs/config.go:305 rejects with the same message we emit, a
    `tll` typo that strict decoding rejects): doc rot the rebuild
    faithfully rejects the same way rather than silently accepting."""

    EXDIR = os.path.join(REF, "docs", "30-configuration", "examples")

    def _outcome(self, name):
        from containerpilot_amd import native
        os.environ.setdefault("CONSUL", "consul.example.com")
        text = open(os.path.join(self.EXDIR, name)).read()
        rendered = native.render_template(text)
        return native.validate_config(rendered)

    def test_examples_present(self):
        assert sorted(os.listdir(self.EXDIR)) == [
            "consul-agent.json5", "database-config.json5",
            "nginx-upstreams.json5", "periodic-tasks.json5",
            "service-reg-only.json5", "stopping.json5"]

    def test_missing_comma_examples_rejected_at_parse(self):
        # flynn/json5 (the reference's parser) also requires commas
        for name in ("consul-agent.json5", "nginx-upstreams.json5",
                     "periodic-tasks.json5"):
            err = self._outcome(name)
            assert err is not None and "parse error" in err, (name, err)

    def test_health_without_interval_rejected_same_message(self):
        # jobs/config.go:305: job[%s].health.interval must be > 0
        for name in ("database-config.json5", "service-reg-only.json5"):
            err = self._outcome(name)
            assert err is not None and \
                "job[consul-agent].health.interval must be > 0" in err, \
                (name, err)

    def test_unknown_key_typo_rejected(self):
        # stopping.json5 has `tll:` (sic); strict decoding rejects it
        # like the reference's mapstructure ErrorUnused
        err = self._outcome("stopping.json5")
        assert err is not None and "tll" in err, err
