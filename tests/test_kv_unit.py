"""Run the native key-watch test binary (cpp/tests/kvtests.cpp): the base64
decoder, the /v1/kv body parser, the change rule, the data model handed to
templates, the `watches[].key` / `keyPrefix` config rules and the request
path."""

import os
import subprocess

from containerpilot_amd import REPO_ROOT, harness

KVTEST_BINARY = os.path.join(REPO_ROOT, "bin", "cpilot_kvtests")


def test_cpp_kvtests():
    # harness.build() returns early once bin/containerpilot exists, so a
    # tree built before this binary was added needs the build forced
    if not os.path.exists(KVTEST_BINARY):
        harness.build(force=True)
    result = subprocess.run([KVTEST_BINARY], capture_output=True,
                            text=True, timeout=60)
    assert result.returncode == 0, result.stdout + result.stderr
    assert "all kv tests passed" in result.stdout
