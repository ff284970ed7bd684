"""Run the native metrics test binary (cpp/tests/metricstests.cpp): the
float printer, name rules, the value parser, nearest-rank quantiles, bucket
state across setBuckets, the refusals, and a replay of every row of
tests/golden/metrics_cases.json through the native hooks."""

import os
import subprocess

from containerpilot_amd import REPO_ROOT, harness

METRICSTEST_BINARY = os.path.join(REPO_ROOT, "bin", "cpilot_metricstests")
TABLE = os.path.join(REPO_ROOT, "tests", "golden", "metrics_cases.json")


def test_cpp_metricstests():
    # harness.build() returns early once bin/containerpilot exists, so a
    # tree built before this binary was added needs the build forced
    if not os.path.exists(METRICSTEST_BINARY):
        harness.build(force=True)
    result = subprocess.run([METRICSTEST_BINARY, TABLE], capture_output=True,
                            text=True, timeout=60)
    assert result.returncode == 0, result.stdout + result.stderr
    assert "all metrics tests passed" in result.stdout
    assert "(0 table rows)" not in result.stdout
