"""CommanderLearner(shuffle_sequences=True) on the MI355X: the default stays what it was, the graph's two gather stages put exactly
the sequences the host schedule names into all ten staging buffers (state_in and seq_len travel with their sequences), and one whole
update of the graph and both eager learners takes the same steps and agrees by the fused = True / False yardstick."""
import numpy as np
import pytest
import torch

import test_gpu_commander_learner_graph as TC
from test_gpu_commander_learner_graph import episodes  # noqa: F401  (the module's fixture: 64 arenas, whole episodes, read only)

pytestmark = pytest.mark.gpu
GRAPH, STAT_KEYS = TC.GRAPH, TC.STAT_KEYS
SHUF = dict(shuffle_sequences=True)
KW = dict(num_sgd_iter=2, sgd_minibatch_size=256)


def _batch(learner, ep):
    seqs = ep.sequences()
    with torch.no_grad():
        b = learner.policy_batch(seqs)
        b["old_logits"] = learner.batch_old_logits(seqs, b)
    return b


def _staged_equals(book, idx, what):
    from hhmarl_2d_amd import learner as LR
    torch.cuda.synchronize()
    assert tuple(book.staged) == LR.COMMANDER_STAGE_COLS
    for k, st in book.staged.items():
        want = LR.minibatch_stage_gather_torch([book.src[k]], book.cap, idx)[0]
        assert st.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (what, k)


def test_the_default_is_off_and_changes_nothing(episodes):  # noqa: F811
    from hhmarl_2d_amd import learner as LR
    ep, net, _ = episodes
    a, b = TC._learner(**KW), TC._learner(shuffle_sequences=False, **KW)
    assert a.shuffle_sequences is False and b.shuffle_sequences is False
    st_a, st_b = a.update(ep, net), b.update(ep, net)
    torch.cuda.synchronize()
    assert st_a == st_b
    assert all(p.detach().cpu().numpy().tobytes() == q.detach().cpu().numpy().tobytes() for p, q in zip(a.module.parameters(), b.module.parameters()))
    graph = TC._learner(**KW, **GRAPH)
    st_g = graph.update(ep, net)
    book = graph._book
    assert book.captures == 1 and book.order is None and len(book.key) == 8 + len(LR.COMMANDER_STAGE_COLS), "no order table without the flag"
    _, sched = LR.sequence_schedule(_batch(graph, ep)["seq_len"].cpu().numpy(), 256, 2, 6, 0, 0)
    assert st_g["steps"] == len(sched)
    _staged_equals(book, range(sched[-1][0], sched[-1][1]), "contiguous")


def test_the_graph_stages_what_the_host_schedule_names(episodes):  # noqa: F811
    from hhmarl_2d_amd import learner as LR
    ep, net, _ = episodes
    graph = TC._learner(**KW, **GRAPH, **SHUF)
    b = _batch(graph, ep)
    seq_len = b["seq_len"].cpu().numpy()
    S = len(seq_len)
    order, sched = LR.shuffled_schedule(seq_len, 256, 2, 6, 0, 0)
    n_steps, n_rows = graph.graph_prepare(b)
    book = graph._book
    assert (n_steps, n_rows) == (len(sched), int(seq_len.sum())) and book.cap == int((sched[:, 1] - sched[:, 0]).max()) and book.captures == 1
    assert book.order[:len(order)].cpu().tolist() == order.tolist() and book.order_len == 2 * S
    second = int(np.searchsorted(sched[:, 0], S))
    assert 0 < second < n_steps and sched[second][0] == S
    seen, done = {}, 0
    for k in (1, second + 1, n_steps):
        graph.graph_replay(k - done)
        done = k
        o0, o1, nv, _ = sched[k - 1].tolist()
        _staged_equals(book, order[o0:o1], k)
        assert int(book.n_valid.item()) == nv == int(book.staged["mask"].sum()) == int(book.staged["seq_len"].sum()) and int(book.cursor.item()) == k
        assert int(book.staged["seq_len"][0]) >= 1, "slot 0 is a real sequence: the GRU kernels' contract"
        seen[k] = book.staged["obs"].clone()
    assert not torch.equal(seen[1], seen[second + 1]), "two passes stage different first minibatches"
    nv = graph.graph_stats(n_steps)[:, 5].cpu().numpy()
    assert np.array_equal(nv, sched[:, 2].astype(np.float64)) and nv[:second].sum() == n_rows and nv[second:].sum() == n_rows
    assert int(graph.optimizer.t.item()) == n_steps and torch.isfinite(graph.graph_stats(n_steps)).all()


def test_one_shuffled_update_on_all_three_paths(episodes):  # noqa: F811
    ep, net, _ = episodes
    graph, fused, plain = TC._learner(**KW, **GRAPH, **SHUF), TC._learner(**KW, **SHUF), TC._learner(fused=False, **KW, **SHUF)
    rows = int(ep.sequences()["mask"].sum()) * 3
    st_g, st_f, st_p = graph.update(ep, net), fused.update(ep, net), plain.update(ep, net)
    assert set(st_g) == set(st_f) == set(STAT_KEYS + ("kl_coeff", "steps", "rows")) and graph.updates == 1 and graph._book.captures == 1
    for st in (st_g, st_f, st_p):
        assert st["rows"] == rows and all(np.isfinite(st[k]) for k in STAT_KEYS + ("kl_coeff",))
    assert st_g["steps"] == st_f["steps"] == st_p["steps"] and st_g["steps"] >= 4
    steps, book = st_g["steps"], graph._book
    assert int(book.cursor.item()) == steps == book.n_steps and int(graph.optimizer.t.item()) == steps
    sched, S = book.schedule[:steps].cpu().numpy(), book.order_len // 2
    nv = graph.graph_stats(steps)[:, 5].cpu().numpy()
    assert int(nv[sched[:, 0] < S].sum()) == rows and int(nv[sched[:, 0] >= S].sum()) == rows, "every pass visits every row once"
    yard, got = TC._gap(st_f, st_p), TC._gap(st_g, st_f)
    print(f"shuffled: max |difference| over the five mean statistics: eager fused=True vs fused=False (the yardstick) {yard:.3e}; graph vs eager "
          f"fused=True {got:.3e}")
    assert got <= 4.0 * yard
    dev_adam = TC._learner(optimizer="fused", **KW, **SHUF)
    st_d = dev_adam.update(ep, net)
    assert st_d["steps"] == steps and int(dev_adam.optimizer.t.item()) == steps and TC._gap(st_d, st_f) <= 4.0 * yard
