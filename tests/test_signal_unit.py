"""Run the native signal test binary (cpp/tests/signaltests.cpp): the name
table, the `signal` spec parser and the config rules with target resolution
in newJobConfigs, and a Job with a signal action on a real loop and bus
against a real child (delivered, no pid, `wait` satisfied, `wait` timed
out, cleanup during `wait`, the pre-stop drain)."""

import os
import subprocess

from containerpilot_amd import REPO_ROOT, harness

SIGNALTEST_BINARY = os.path.join(REPO_ROOT, "bin", "cpilot_signaltests")


def test_cpp_signaltests():
    # harness.build() returns early once bin/containerpilot exists, so a
    # tree built before this binary was added needs the build forced
    if not os.path.exists(SIGNALTEST_BINARY):
        harness.build(force=True)
    result = subprocess.run([SIGNALTEST_BINARY], capture_output=True,
                            text=True, timeout=60)
    assert result.returncode == 0, result.stdout + result.stderr
    assert "all signal tests passed" in result.stdout
