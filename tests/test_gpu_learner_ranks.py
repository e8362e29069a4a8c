"""Two torch.distributed ranks against their in-process twin on the MI355X: PPOLearner(group=ShardGroup()) in two fresh child
processes (tests/learner_rank_child.py, both on cuda:0, backend gloo over a file rendezvous in a temporary directory) and
PPOLearner(group=LocalShards(2)) here, on the same two shards — 64 arenas at offset 0, 16 arenas at offset 64, so the short shard is
empty at the tail of every pass.  After two collect -> update_window -> publish rounds the three digests (the result dicts without
rows_local, the SHA-256 of every parameter and of Adam's m, v, t) are the same bytes: W ranks compute what one process over the W
shards computes.  Three processes hold the GPU; nearly all of the time is their start-up.  Every gloo wait is bounded by the group's
60 s timeout and each child by its own `timeout`, so a mismatch ends as an error, never as a wait."""
import os
import subprocess
import sys

import pytest

import learner_rank_child as RC

pytestmark = pytest.mark.gpu
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "learner_rank_child.py")


def test_two_ranks_equal_local_shards(tmp_path):
    import torch
    from hhmarl_2d_amd.learner import LocalShards
    env = dict(os.environ, GLOO_SOCKET_IFNAME="lo")
    outs = [str(tmp_path / f"rank{r}.json") for r in range(2)]
    logs = [open(tmp_path / f"rank{r}.log", "w") for r in range(2)]
    procs = [subprocess.Popen(["timeout", "-k", "10", "150", sys.executable, CHILD, str(r), "2", str(tmp_path / "rendezvous"), outs[r]],
                              env=env, stdout=logs[r], stderr=subprocess.STDOUT) for r in range(2)]
    try:
        # the twin, while the ranks start up
        shards = [RC.build_shard(n, off) for n, off in zip(RC.ARENAS, RC.OFFSETS)]
        learner = RC.make_learner(group=LocalShards(2), **RC.LEARNER)
        results = RC.two_rounds(learner, [s[0] for s in shards], [s[1] for s in shards])
        torch.cuda.synchronize()
        mine = RC.digest(learner, results)
        codes = [p.wait(timeout=170) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
        for f in logs:
            f.close()
    tails = [open(tmp_path / f"rank{r}.log").read()[-3000:] for r in range(2)]
    assert codes == [0, 0], f"rank 0:\n{tails[0]}\nrank 1:\n{tails[1]}"
    ranks = [open(o).read() for o in outs]
    print(mine)
    assert all(d["steps"] >= 4 and d["rows"] == RC.T * sum(RC.ARENAS) == d["rows_local"] for res in results for d in res)
    assert ranks[0] == ranks[1], "both ranks hold the same results, parameters and Adam state"
    assert ranks[0] == mine, "and they are the in-process twin's"
