"""Run the native sensor test binary (cpp/tests/sensortests.cpp): the
extraction table with every documented reason, counter deltas, the file
source (missing file, directory, FIFO without a writer, oversized file)
and the engine on a real loop against a listener the binary opens itself
on 127.0.0.1 (periodic sampling, skipped ticks, timeout, cancel with fd
accounting, dropped bus)."""

import os
import subprocess

from containerpilot_amd import REPO_ROOT, harness

SENSORTEST_BINARY = os.path.join(REPO_ROOT, "bin", "cpilot_sensortests")


def test_cpp_sensortests():
    # harness.build() returns early once bin/containerpilot exists, so a
    # tree built before this binary was added needs the build forced
    if not os.path.exists(SENSORTEST_BINARY):
        harness.build(force=True)
    # the timeout is also the FIFO check: a worker blocked on a FIFO with
    # no writer would hang the binary
    result = subprocess.run([SENSORTEST_BINARY], capture_output=True,
                            text=True, timeout=60)
    assert result.returncode == 0, result.stdout + result.stderr
    assert "all sensor tests passed" in result.stdout
