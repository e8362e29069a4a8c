"""The scripted long-episode streams of tests/episodes_long_ref.py without a GPU: what tests/test_gpu_episodes_long.py relies on them to
cover is asserted here on the host restatement alone, so that a later edit of the patterns cannot quietly stop covering it — episodes
one short of, exactly and one past one, two and three GAE chunks (c = 512 // n_agents rows), an episode of exactly carry_cap + 1
rows, more than 64 episodes of one arena in one window, a done on tick 0 behind a carry and one on tick T - 1, and with sequences
ceil(E / L) per episode and a sequence that starts exactly on a window's first tick, inside an episode that began in the carry."""
import numpy as np
import pytest

from episodes_long_ref import COMMANDER, GEOMETRIES, SEQ_LENS, most_per_window, reference, script

# the figures of the scripts: (K, rows, episodes, longest episode) per geometry
EXPECTED = {(2, 26, 96): (9, 6241, 796, 768), (3, 34, 96): (6, 4117, 532, 510), (1, 26, 96): (17, 12385, 1580, 1536),
            (5, 7, 96): (4, 2509, 324, 306), (64, 1, 7): (4, 194, 42, 24)}


def _check_coverage(ref):
    per, carried, c, T, cap = ref["per"], ref["carried"], ref["c"], ref["T"], ref["carry_cap"]
    N = len(ref["arenas"])
    lens = np.concatenate([p["ep_len"] for p in per])
    for want in (c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 3 * c):
        assert (lens == want).any(), f"no episode of {want} rows"
    assert lens.max() == cap + 1 == 3 * c
    if T > 64:
        assert most_per_window(per, N) > 64, "no window ends more than 64 episodes in one arena"
    assert most_per_window(per, N) == min(T, 3 * c)
    assert carried.max() <= cap, "a carry beyond carry_cap"
    first_tick = last_tick = 0
    for k, p in enumerate(per):
        before = carried[k - 1] if k else np.zeros(N, dtype=np.int32)
        _, first = np.unique(p["ep_arena"], return_index=True)   # every arena's first episode of the collect
        for e in first:
            a = p["ep_arena"][e]
            first_tick += before[a] > 0 and p["ep_len"][e] == before[a] + 1
        last_tick += int(((carried[k] == 0) & (np.bincount(p["ep_arena"], minlength=N) > 0)).sum())
    assert first_tick > 0, "no done on tick 0 behind a carry"
    assert last_tick > 0, "no done on tick T - 1"
    return lens


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_scripts_cover_what_they_claim(geometry):
    nA, D, T = geometry
    ref = reference(nA, D, T)
    lens = _check_coverage(ref)
    K, rows, episodes, longest = EXPECTED[geometry]
    assert (ref["K"], sum(len(p["t"]) for p in ref["per"]), len(lens), int(lens.max())) == (K, rows, episodes, longest)
    assert ref["n"] == K * T and ref["n"] >= 3 * ref["c"] + 2 > ref["n"] - T
    # every column of every row once: what is emitted and what is still carried add up to the stream
    per_arena = sum(np.bincount(p["arena"], minlength=8) for p in ref["per"])
    assert np.array_equal(per_arena + ref["carried"][-1], np.full(8, ref["n"]))


@pytest.mark.parametrize("L", SEQ_LENS)
def test_commander_scripts_cover_the_sequence_cuts(L):
    nA, D, T = COMMANDER
    ref = reference(nA, D, T, L)
    per, carried, cap = ref["per"], ref["carried"], ref["carry_cap"]
    assert len(ref["arenas"]) == 9 and ref["arenas"][8][:4] == [max(L - 1, 1), L, L + 1, 2 * L]
    assert ref["stream"]["done"].shape[0] - sum(ref["arenas"][8]) < max(L - 1, 1) + 3 * L + 1, "the ninth arena's cycle runs up to n"
    lens = _check_coverage(ref)
    for want in {max(L - 1, 1), L, L + 1, 2 * L}:
        assert (lens == want).any()
    if L > 1:
        assert cap % L != 0, "carry_cap no multiple of L: the last state-carry slot is a partial one"
    on_first_tick = from_carry = 0
    for k, p in enumerate(per):
        E = len(p["ep_len"])
        assert np.array_equal(np.bincount(p["seq_ep"], minlength=E), -(-p["ep_len"] // L)), f"collect {k}: sequences per episode"
        assert p["state_in"].shape == (len(p["seq_start"]), 3, 2, 200)
        before = carried[k - 1] if k else np.zeros(9, dtype=np.int32)
        _, first = np.unique(p["ep_arena"], return_index=True)
        for e in first:
            cl = before[p["ep_arena"][e]]
            off = p["seq_start"][p["seq_ep"] == e] - p["ep_start"][e]
            on_first_tick += cl > 0 and (off == cl).any()   # i == cl: the state comes from the window, not from the carry
            from_carry += int(((off > 0) & (off < cl)).sum())
    assert on_first_tick > 0, "no sequence starts exactly on a window's first tick behind a carry"
    assert from_carry > 0, "no sequence start inside the carry"


def test_script_sizes():
    for nA, D, T in GEOMETRIES:
        arenas, c, n, K, cap = script(nA, T)
        assert c == 512 // nA and cap == 3 * c - 1 and n % T == 0 and n - T < 3 * c + 2 <= n
        assert [sum(a) for a in arenas[:6]] == [3 * c] * 6 and sum(arenas[6]) == n and sum(arenas[7]) == n - T + 1
