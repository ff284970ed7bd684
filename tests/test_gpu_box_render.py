"""Native watch rendering on the box, with the daemon as deployed.

As in test_gpu_box.py, "gpu" means the MI355X node's host: the workload
is a CPU-only daemon. The daemon runs behind its subreaper supervisor and
starts the onChange job through its spawn helpers; a blocking watch sees
three changes, and after each the job's `cat <dest>` must have logged the
rendering of exactly that set.
"""

import pytest

from test_watch_render import ONE, TWO, check_ordering, start_daemon


@pytest.mark.gpu
def test_render_ordering_on_gpu_box(daemon_factory, mock_consul, tmp_path):
    d, dest = start_daemon(daemon_factory, mock_consul, tmp_path,
                           env={"CPILOT_FORCE_SUP": "1"})
    check_ordering(d, mock_consul, dest, [ONE, TWO, []])
    assert "{Error" not in d.log()
    d.terminate()
    assert d.wait(timeout=30) == 0, d.log()[-3000:]
