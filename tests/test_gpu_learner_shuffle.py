"""PPOLearner(shuffle_sequences=True) on the MI355X: the default stays what it was, the graph stages exactly the chunks the host schedule
names (byte for byte), whole updates of the graph and both eager learners take the same steps and agree by the project's yardstick (the
fused = True / False difference), one minibatch over the whole batch does not care about the order, and every pass and every update
draws another order.  Weights after many Adam steps are never compared between paths."""
import numpy as np
import pytest
import torch

import test_gpu_learner_graph as TG

pytestmark = pytest.mark.gpu
GRAPH, STAT_KEYS = TG.GRAPH, TG.STAT_KEYS
SHUF = dict(shuffle_sequences=True)


@pytest.fixture(scope="module")
def fight():
    """64 arenas, T = 32: one collect, shared and left unchanged"""
    ro, bank = TG._world()
    ro.collect()
    return ro, bank


@pytest.fixture(scope="module")
def escape():
    ro, bank = TG._world("escape")
    ro.collect()
    return ro, bank


def _weight_bytes(learner):
    torch.cuda.synchronize()
    return [p.detach().cpu().numpy().tobytes() for m in learner.modules for p in m.parameters()]


def _batch(learner, ro, bank, agent):
    rows = ro.episodes.rows()
    with torch.no_grad():
        old = learner.batch_old_logits(rows, bank, ro.episodes.N)
        return learner.policy_batch(rows, old, agent)


def _seq_len(learner, b):
    return b["seq_len"].cpu().numpy() if learner.recurrent else np.ones(b["obs"].shape[0], dtype=np.int64)


def _staged_equals(book, idx, what):
    """every staged column = its source column's chunks idx, in that order, zeros behind, byte for byte"""
    from hhmarl_2d_amd import learner as LR
    torch.cuda.synchronize()
    for k, st in book.staged.items():
        want = LR.minibatch_stage_gather_torch([book.src[k]], book.cap, idx)[0]
        assert st.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (what, k)


def test_the_default_is_off_and_changes_nothing(fight):
    ro, bank = fight
    a, b = TG._learner(), TG._learner(shuffle_sequences=False)
    assert a.shuffle_sequences is False and b.shuffle_sequences is False
    st_a, st_b = a.update(ro.episodes, bank), b.update(ro.episodes, bank)
    assert st_a == st_b and _weight_bytes(a) == _weight_bytes(b)
    graph = TG._learner(**GRAPH)
    st_g = graph.update(ro.episodes, bank)
    assert [bk.captures for bk in graph._books] == [1, 1] and all(bk.order is None for bk in graph._books), "no order table without the flag"
    from hhmarl_2d_amd import learner as LR
    for agent, bk in enumerate(graph._books):      # the last step's staging buffers hold the contiguous range of the unshuffled schedule
        batch = _batch(graph, ro, bank, agent)
        _, sched = LR.sequence_schedule(_seq_len(graph, batch), 256, 2, 5, 0, agent)
        assert st_g[agent]["steps"] == len(sched) and len(bk.key) == 8 + len(bk.staged)
        s0, s1 = sched[-1][:2]
        _staged_equals(bk, range(s0, s1), "contiguous")


@pytest.mark.parametrize("mode", ("fight", "escape"))
def test_the_graph_stages_what_the_host_schedule_names(mode, fight, escape):
    from hhmarl_2d_amd import learner as LR
    ro, bank = fight if mode == "fight" else escape
    graph = TG._learner(mode, **GRAPH, **SHUF)
    for agent in range(2):
        b = _batch(graph, ro, bank, agent)
        seq_len = _seq_len(graph, b)
        S = len(seq_len)
        order, sched = LR.shuffled_schedule(seq_len, 256, 2, 5, 0, agent)
        n_steps, n_rows = graph.graph_prepare(agent, b)
        book = graph._books[agent]
        assert (n_steps, n_rows) == (len(sched), int(seq_len.sum())) and book.cap == int((sched[:, 1] - sched[:, 0]).max())
        assert book.order.dtype == torch.int32 and book.order[:len(order)].cpu().tolist() == order.tolist() and book.order.shape[0] >= 2 * S
        second = int(np.searchsorted(sched[:, 0], S))          # the first step of the second pass
        assert 0 < second < n_steps and sched[second][0] == S
        seen, done = {}, 0
        for k in (1, second + 1, n_steps):
            graph.graph_replay(agent, k - done)
            done = k
            o0, o1, nv, _ = sched[k - 1].tolist()
            _staged_equals(book, order[o0:o1], (mode, agent, k))
            assert int(book.n_valid.item()) == nv and int(book.cursor.item()) == k
            assert int(book.staged["mask"].sum()) == nv
            seen[k] = book.staged["obs"].clone()
        assert not torch.equal(seen[1], seen[second + 1]), "two passes stage different first minibatches"
        assert set(order[sched[0][0]:sched[0][1]].tolist()) != set(order[sched[second][0]:sched[second][1]].tolist())
        assert int(book.cursor.item()) == n_steps and int(graph.optimizers[agent].t.item()) == n_steps
        nv = graph.graph_stats(agent, n_steps)[:, 5].cpu().numpy()
        assert np.array_equal(nv, sched[:, 2].astype(np.float64))
        assert nv[:second].sum() == n_rows and nv[second:].sum() == n_rows, "every pass visits every row once"
        assert book.captures == 1


def _check(what, st_graph, st_fused, st_plain, graph, n_rows):
    """TG._check_update for schedules whose passes may differ in length: the same step counts on all three paths, the cursor at n_steps, every
    pass's n_valid summing to the batch's rows, and graph vs eager fused=True within 4 x eager fused=True vs fused=False"""
    from hhmarl_2d_amd import learner as LR
    for st in (st_graph, st_fused, st_plain):
        assert len(st) == 2 and all(s["rows"] == n_rows for s in st)
        assert all(np.isfinite(s[k]) for s in st for k in STAT_KEYS + ("kl_coeff",))
    assert [s["steps"] for s in st_graph] == [s["steps"] for s in st_fused] == [s["steps"] for s in st_plain] and all(s["steps"] >= 2 for s in st_graph)
    for a in range(2):
        book, steps = graph._books[a], st_graph[a]["steps"]
        assert int(book.cursor.item()) == steps == book.n_steps
        sched = book.schedule[:steps].cpu().numpy()
        S = book.order_len // graph.num_sgd_iter
        nv = graph.graph_stats(a, steps)[:, 5].cpu().numpy()
        for p in range(graph.num_sgd_iter):
            in_pass = (sched[:, 0] >= p * S) & (sched[:, 0] < (p + 1) * S)
            assert int(nv[in_pass].sum()) == n_rows, "every pass visits every row once"
    yard, got = TG._gap(st_fused, st_plain), TG._gap(st_graph, st_fused)
    print(f"{what}: per policy max |difference| over the five mean statistics: eager fused=True vs fused=False (the yardstick) "
          f"{yard[0]:.3e}, {yard[1]:.3e}; graph vs eager fused=True {got[0]:.3e}, {got[1]:.3e}")
    for a in range(2):
        assert got[a] <= 4.0 * yard[a], (what, a, got, yard)


@pytest.mark.parametrize("mode", ("fight", "escape"))
def test_one_shuffled_update_on_all_three_paths(mode, fight, escape):
    ro, bank = fight if mode == "fight" else escape
    graph, fused, plain = TG._learner(mode, **GRAPH, **SHUF), TG._learner(mode, **SHUF), TG._learner(mode, fused=False, **SHUF)
    R = ro.episodes.rows()["obs"].shape[0]
    assert R > 512
    st_g, st_f, st_p = graph.update(ro.episodes, bank), fused.update(ro.episodes, bank), plain.update(ro.episodes, bank)
    _check(f"one shuffled update, {mode}", st_g, st_f, st_p, graph, R)
    assert set(st_g[0]) == set(st_f[0]) == set(STAT_KEYS + ("kl_coeff", "steps", "rows")), "update() keeps its keys"
    dev_adam = TG._learner(mode, optimizer="fused", **SHUF)
    st_d = dev_adam.update(ro.episodes, bank)
    assert [s["steps"] for s in st_d] == [s["steps"] for s in st_f] and all(int(o.t.item()) == s["steps"] for o, s in zip(dev_adam.optimizers, st_d))
    assert all(g <= 4.0 * y for g, y in zip(TG._gap(st_d, st_f), TG._gap(st_f, st_p)))


@pytest.mark.parametrize("mode", ("fight", "escape"))
def test_one_minibatch_over_the_whole_batch_does_not_care_about_the_order(mode, fight, escape):
    """num_sgd_iter = 1 and a minibatch size beyond the batch's rows: ONE step on all rows, shuffled or not — the same sums in another order"""
    ro, bank = fight if mode == "fight" else escape
    kw = dict(num_sgd_iter=1, sgd_minibatch_size=100000)
    plain_fused, plain_torch = TG._learner(mode, **kw), TG._learner(mode, fused=False, **kw)
    shuffled, shuffled_graph = TG._learner(mode, **kw, **SHUF), TG._learner(mode, **kw, **GRAPH, **SHUF)
    st = [ln.update(ro.episodes, bank) for ln in (plain_fused, plain_torch, shuffled, shuffled_graph)]
    assert all(s["steps"] == 1 for x in st for s in x)
    yard, eager, graph = TG._gap(st[0], st[1]), TG._gap(st[2], st[0]), TG._gap(st[3], st[0])
    print(f"{mode}, one step on the whole batch: yardstick {yard}, shuffled eager vs unshuffled {eager}, shuffled graph vs unshuffled {graph}")
    for a in range(2):
        assert eager[a] <= 4.0 * yard[a] and graph[a] <= 4.0 * yard[a], (a, yard, eager, graph)


def test_a_second_update_draws_another_order_and_keeps_the_graph(escape):
    """kl_coeff = 0 and the same escape batch twice: rows are chunks of one row, so every order cuts minibatches of the same sizes and
    nothing in the graph's key changes — one capture serves both updates, while the order table's content is update 1's"""
    from hhmarl_2d_amd import learner as LR
    ro, bank = escape
    graph = TG._learner("escape", kl_coeff=0.0, **GRAPH, **SHUF)
    R = ro.episodes.rows()["obs"].shape[0]
    tables = []
    for upd in range(2):
        st = graph.update(ro.episodes, bank)
        for agent, bk in enumerate(graph._books):
            want, sched = LR.shuffled_schedule(np.ones(R, dtype=np.int64), 256, 2, 5, upd, agent)
            assert bk.order[:2 * R].cpu().tolist() == want.tolist() and bk.order_len == 2 * R and st[agent]["steps"] == len(sched)
        tables.append([bk.order[:2 * R].clone() for bk in graph._books])
    assert all(not torch.equal(x, y) for x, y in zip(*tables)), "update 1 uses another order than update 0"
    assert not torch.equal(tables[0][0], tables[0][1]), "and the two policies differ"
    assert [bk.captures for bk in graph._books] == [1, 1] and graph.updates == 2
    assert all(int(o.t.item()) == 2 * s["steps"] for o, s in zip(graph.optimizers, st))
