"""Run the native render test binary (cpp/tests/rendertests.cpp): the
template engine against data, the health-entry parser and the model
handed to templates, the `watches[].render` config rules, and the atomic
write helper in a temporary directory."""

import os
import subprocess

from containerpilot_amd import REPO_ROOT, harness

RENDERTEST_BINARY = os.path.join(REPO_ROOT, "bin", "cpilot_rendertests")


def test_cpp_rendertests():
    # harness.build() returns early once bin/containerpilot exists, so a
    # tree built before this binary was added needs the build forced
    if not os.path.exists(RENDERTEST_BINARY):
        harness.build(force=True)
    result = subprocess.run([RENDERTEST_BINARY], capture_output=True,
                            text=True, timeout=60)
    assert result.returncode == 0, result.stdout + result.stderr
    assert "all render tests passed" in result.stdout
