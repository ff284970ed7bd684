"""Key watches on the box, with the daemon as deployed.

As in test_gpu_box.py, "gpu" means the MI355X node's host: the workload is
a CPU-only daemon, here behind its subreaper supervisor. Twenty blocking
key watches changed in one burst are the smallest shape where twenty
long-poll threads wake together and their completions interleave on the
reactor with twenty launches through the spawn helpers. No rate or latency
is asserted: nobody has measured one. wait_until's default timeout is a
liveness bound only.

Run once on the box with the other `gpu`-marked files
(`python -m pytest tests/ -q -m gpu`): 12 passed in 75 s, the two tests
here in 1.2 s and 3.1 s; all twenty files held their key's value, each
job's last `cat` equalled its file, no `Error` event.
"""

import pytest

from test_kv_watch import (TEMPLATE, check_kv_ordering, finish, rendering,
                           start_daemon)
from test_watch_render import job_outputs, read_file, wait_until

WATCHES = 20
SUP = {"CPILOT_FORCE_SUP": "1"}


@pytest.mark.gpu
def test_kv_render_ordering_on_gpu_box(daemon_factory, mock_consul, tmp_path):
    d, dest = start_daemon(daemon_factory, mock_consul, tmp_path, env=SUP)
    check_kv_ordering(d, mock_consul, dest)
    finish(d)


@pytest.mark.gpu
def test_twenty_key_watches_change_at_once_on_gpu_box(daemon_factory,
                                                      mock_consul, tmp_path):
    source = tmp_path / "mode.ctmpl"
    source.write_text(TEMPLATE)
    names = ["kv-%02d" % n for n in range(WATCHES)]
    keys = {name: "myapp/burst/%s" % name for name in names}
    dests = {name: str(tmp_path / (name + ".conf")) for name in names}
    jobs = [{"name": "main-app", "exec": "sleep 60"}]
    watches = []
    for name in names:
        jobs.append({"name": "on-" + name, "exec": ["cat", dests[name]],
                     "when": {"source": "watch." + name, "each": "changed"}})
        watches.append({"name": name, "key": keys[name], "interval": 30,
                        "blocking": True,
                        "render": {"source": str(source),
                                   "dest": dests[name]}})
    d = daemon_factory({
        "consul": mock_consul.address, "stopTimeout": 1,
        "logging": {"level": "DEBUG"}, "jobs": jobs, "watches": watches,
    }, env=SUP).start()
    d.wait_for_socket()
    # every first result (a missing key) is rendered
    assert wait_until(lambda: all(
        read_file(dest) == rendering(None) for dest in dests.values())), \
        d.log()[-3000:]

    # one burst, one value per key: what an `each` job does with an event
    # that arrives while it runs is not this test's subject. Each set_kv
    # moves the mock's single index, so every long-poll wakes again and
    # again while the others' changes arrive.
    final = {}
    for name in names:
        final[name] = ("final-" + name).encode()
        mock_consul.set_kv(keys[name], final[name])

    def settled():
        log = d.log()
        for name in names:
            want = rendering(final[name])
            if read_file(dests[name]) != want:
                return False
            outputs = job_outputs(log, job="on-" + name)
            if not outputs or outputs[-1] != want:
                return False
        return True

    assert wait_until(settled), d.log()[-4000:]
    log = d.log()
    for name in names:
        # each job's last logged `cat` equals its file
        assert job_outputs(log, job="on-" + name)[-1] == \
            read_file(dests[name]) == rendering(final[name])
    assert "{Error" not in log
    finish(d)
