"""The one minibatch-step driver of both learners (_PolicySGD) on the MI355X: from identical weights an eager learner and a graph learner
with the device Adam run one update of the same small policy batch, and the unpadded rows that each step wrote to its statistics table
are update_schedule's column 2, row for row — eager and graph walked the same table in the same order, with shuffle_sequences off and on.
Weights after several Adam steps are not compared between the two (ill-conditioned); the yardstick tests of
test_gpu_learner_graph.py and test_gpu_commander_learner_graph.py cover the statistics."""
import numpy as np
import pytest
import torch

import test_gpu_commander_learner_graph as TC
import test_gpu_learner_graph as TG

pytestmark = pytest.mark.gpu
SIZE, PASSES = 32, 2        # the builders' 14 ragged chunks of 20 hold 135 .. 145 rows: four steps per pass, the last one a remainder


def _fight(shuffle, step):
    """PPOLearner over the fight kinds -> (learner, [(driver, policy batch, policy index), ...]): both policies, each with its own batch"""
    from hhmarl_2d_amd import learner as LR
    from hhmarl_2d_amd import policy_nets as PN
    kinds = (PN.FIGHT1, PN.FIGHT2)
    ln = LR.PPOLearner(kinds, [TG._weights(k, 9) for k in kinds], torch.device("cuda", 0), seed=9, kl_coeff=0.0, num_sgd_iter=PASSES,
                       sgd_minibatch_size=SIZE, optimizer="fused", step=step, shuffle_sequences=shuffle)
    return ln, [(ln._sgd[a], TG._policy_batch(k, ln.modules[a], 40 + k), a) for a, k in enumerate(kinds)]


def _commander(shuffle, step):
    """CommanderLearner -> (learner, [(driver, policy batch with old_logits, 0)])"""
    ln = TC._learner(kl_coeff=0.0, num_sgd_iter=PASSES, sgd_minibatch_size=SIZE, optimizer="fused", step=step, shuffle_sequences=shuffle)
    return ln, [(ln._sgd, TC._policy_batch(ln.module, 41), 0)]


@pytest.mark.parametrize("make", (_fight, _commander), ids=("fight", "commander"))
def test_a_dropped_graph_learner_is_freed_by_reference_counting(make):
    """A learner that has captured its step holds a HIP graph with a memory pool of its own.  Were the learner part of a reference cycle
    (its driver holding it back), the graph would live until the cyclic collector runs — which may be in the middle of another capture,
    where freeing a pool aborts the process.  With the collector switched off, dropping the last reference frees learner and step book."""
    import gc
    import weakref
    ln, todo = make(False, "graph")
    driver, b, _ = todo[0]
    driver.run(*ln._columns(b, staged=True))
    torch.cuda.synchronize()
    assert driver.book.captures == 1 and driver.book.graph is not None
    refs = [weakref.ref(ln), weakref.ref(driver), weakref.ref(driver.book)]
    was_on = gc.isenabled()
    gc.disable()
    try:
        del ln, todo, driver, b
        assert [r() for r in refs] == [None, None, None]
    finally:
        if was_on:
            gc.enable()


@pytest.mark.parametrize("shuffle", (False, True), ids=("in order", "shuffled"))
@pytest.mark.parametrize("make", (_fight, _commander), ids=("fight", "commander"))
def test_eager_and_graph_walk_the_same_table(make, shuffle):
    from hhmarl_2d_amd import learner as LR
    (eager, todo_e), (graph, todo_g) = make(shuffle, "eager"), make(shuffle, "graph")
    assert eager.step == "eager" and graph.step == "graph" and eager.shuffle_sequences is shuffle and graph.shuffle_sequences is shuffle
    for (d_e, b, _), (d_g, b_g, _) in zip(todo_e, todo_g):      # before any step: the fight policies share a layer that every step moves
        assert type(d_e) is LR._PolicySGD and type(d_g) is LR._PolicySGD, "one driver class serves PPOLearner and CommanderLearner"
        assert all(torch.equal(p, q) for p, q in zip(d_e.module.parameters(), d_g.module.parameters())), "identical weights"
        assert all(torch.equal(b[k], b_g[k]) for k in b), "the same batch"
    for (d_e, b, policy), (d_g, _, _) in zip(todo_e, todo_g):
        cols, seq_len = eager._columns(b)
        _, sched, _ = LR.update_schedule(seq_len, SIZE, PASSES, eager.seed, 0, policy, shuffle)
        parts = LR.minibatch_partition(seq_len, SIZE)
        assert len(parts) >= 3 and int(np.asarray(seq_len)[parts[-1][0]:].sum()) < SIZE, "at least three steps per pass, the last a remainder"
        assert len(sched) >= PASSES * 3
        st_e, st_g = d_e.run(cols, seq_len), d_g.run(*graph._columns(b, staged=True))
        torch.cuda.synchronize()
        steps = len(sched)
        assert st_e["steps"] == st_g["steps"] == steps and st_e["rows"] == st_g["rows"] == int(np.sum(seq_len))
        for what, d in (("eager", d_e), ("graph", d_g)):
            walked = d.book.table[:steps, 5].tolist()
            print(f"{make.__name__[1:]} policy {policy}, shuffle {shuffle}, {what}: unpadded rows per step {[int(x) for x in walked]}")
            assert walked == sched[:, 2].tolist(), f"{what} visited update_schedule's rows in its order"
            assert int(d.book.cursor.item()) == steps and int(d.optimizer.t.item()) == steps
        assert d_g.book.captures == 1 and d_g.book.n_steps == steps
