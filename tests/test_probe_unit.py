"""Run the native probe-engine test binary (cpp/tests/probetests.cpp):
tcp/http verdicts, the request on the wire, split and oversized status
lines, timeout, overlap, cancel, fd accounting and bus lifetime, against
listeners the binary opens itself on 127.0.0.1."""

import os
import subprocess

from containerpilot_amd import REPO_ROOT, harness

PROBETEST_BINARY = os.path.join(REPO_ROOT, "bin", "cpilot_probetests")


def test_cpp_probetests():
    # harness.build() returns early once bin/containerpilot exists, so a
    # tree built before this binary was added needs the build forced
    if not os.path.exists(PROBETEST_BINARY):
        harness.build(force=True)
    result = subprocess.run([PROBETEST_BINARY], capture_output=True,
                            text=True, timeout=60)
    assert result.returncode == 0, result.stdout + result.stderr
    assert "all probe tests passed" in result.stdout
