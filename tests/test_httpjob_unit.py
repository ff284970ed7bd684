"""Run the native http job test binary (cpp/tests/httpjobtests.cpp): the
`http` spec parser and the config rules, the request bytes, and a Job with
an http action on a real loop and bus against a scripted listener (200 with
and without a length, 503, garbage, early close, a bytewise status line,
more than the drain cap, no answer, starts while in flight, cleanup while in
flight, the pre-stop chain)."""

import os
import subprocess

from containerpilot_amd import REPO_ROOT, harness

HTTPJOBTEST_BINARY = os.path.join(REPO_ROOT, "bin", "cpilot_httpjobtests")


def test_cpp_httpjobtests():
    # harness.build() returns early once bin/containerpilot exists, so a
    # tree built before this binary was added needs the build forced
    if not os.path.exists(HTTPJOBTEST_BINARY):
        harness.build(force=True)
    result = subprocess.run([HTTPJOBTEST_BINARY], capture_output=True,
                            text=True, timeout=60)
    assert result.returncode == 0, result.stdout + result.stderr
    assert "all http job tests passed" in result.stdout
