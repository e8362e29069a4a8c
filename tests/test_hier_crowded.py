"""The CPU half of the crowded-arena test of the HighLevelEnv tick's envelope queue: the oracle alone runs every fixture of hier_crowded.py and
counts how often each site is reached, and how many entries a lane queues at least (from exact geometry: the kernels' prefilters are
conservative).  A fixture that never reaches a site would let the GPU test (test_gpu_hier_crowded.py) pass on nothing, so a zero count
fails HERE.

What the counts say about the GPU test (it cannot be shown without a GPU, so it is argued from them): with QCAP back at 8 for the ten-slot
instances, a lane that reserves more than 8 entries writes 8 and the rest of its reservation is drained as stale codes — the fixtures hold lanes
with 9 and more entries (`lane_entries_max`) and `kill_hangs_on_ninth_entry_or_later` counts kills that only such an entry decides (a cannon hit
nobody else scores on that target in that tick, or a fuse behind eight cannon candidates).  With the slot field masked by 7, a target in slot 8
or 9 is looked up as slot 0 or 1: `cannon_target_8_or_9` counts the cannon kills of those slots.

`wave_all_groups_queue`: a tick on which every laid-out arena of the first wave queues something.  At 6 arenas per wave (ten slots) that is the whole
wave, arenas 0..5.  At 8 and at 10 arenas per wave (six slots) the first wave also holds arena 6, the untouched one of the layout table, which queues
nothing by design: there the condition covers the other 7 and 9 arenas."""
import numpy as np
import pytest

import hier_crowded as H

# the largest lower bound of one lane that the fixture must reach: layout 3 gives (nU - 1) cannon candidates + 2 fuses, layout 5 (v = 0)
# 1 launch + (nU - 1) cannon candidates + 2 fuses — the full 12 of a ten-slot lane with ten aircraft
LANE_ENTRIES = {sides: sum(sides) + 2 for sides in H.SIDES}


def _needs(site, key):
    (nA, nO), _ = key
    if site == "cannon_target_8_or_9":
        return nA + nO > 8          # the arena has an aircraft in slot 8
    if site == "kill_hangs_on_ninth_entry_or_later":
        return nA + nO > 8          # nine candidates, or eight and the fuses behind them
    return True


@pytest.mark.parametrize("key", H.KEYS, ids=[H.key_id(k) for k in H.KEYS])
def test_fixture_reaches_every_site(oracle, key):
    sides, default = key
    res = H.oracle_run(sides, default)
    n, lane_max, waves = res["counts"], res["lane_max"], res["waves"]
    print(H.key_id(key), "lane_entries_max", int(lane_max.max()), "per arena", lane_max.tolist())
    print(H.key_id(key), "waves (arenas per wave: ticks on which every laid-out arena of the first wave queues, largest summed bound)", waves)
    print(H.key_id(key), n)
    print(H.key_id(key), "dones per step", [int(s["outs"][3].sum()) for s in res["steps"]], "arena-ticks", [s["tick_count"] for s in res["steps"]])
    assert lane_max.max() >= LANE_ENTRIES[sides], f"lane_entries_max {lane_max.max()}"
    nU = sum(sides)
    for a in range(H.N):   # every laid-out arena is as crowded as its layout says
        want = {0: nU - 1, 1: nU - 1, 2: max(sides), 3: nU + 1, 4: 1, 5: nU + 2 if a < 7 else sides[0], 6: 0}[a % 7]
        assert lane_max[a] >= want, f"arena {a} (layout {a % 7}): a lane queues at least {lane_max[a]}, the layout promises {want}"
    for G, w in waves.items():
        assert w["ticks"] >= 1 and w["best"] >= 1, f"wave_all_groups_queue at {G} arenas per wave"
    for site in H.SITES:
        if _needs(site, key):
            assert n[site] >= 1, f"{H.key_id(key)}: the fixture never reaches `{site}`"
    assert not res["faults"].any()
    assert res["steps"][-1]["tick_count"] < H.STEPS * H.SUB * H.N, "arenas leave their macro step early"
    assert res["steps"][1]["ticks"][H.K_FIRE[1]]["events"].any(), "step 1 meets its crowded tick mid-step"


@pytest.mark.parametrize("key", H.KEYS, ids=[H.key_id(k) for k in H.KEYS])
def test_untouched_arenas_equal_a_world_of_untouched_arenas(oracle, key):
    """the arenas of layout 6 beside the crowded ones: the oracle gives them what it gives them when NO arena is laid out"""
    sides, default = key
    got, want = H.oracle_run(sides, default), H.untouched_run(sides, default)
    sel = np.arange(H.N) % 7 == 6
    for step, (g, w) in enumerate(zip(got["steps"], want["steps"])):
        for x, y, field in zip(g["outs"], w["outs"], H.OUTS):
            assert np.array_equal(x[sel], y[sel]), f"step {step}: {field}"
        for k in w["state"]:
            assert np.array_equal(g["state"][k][sel], w["state"][k][sel]), f"step {step}: state {k}"
        for tg, tw in zip(g["ticks"], w["ticks"]):
            for k in ("po_a", "pm_a", "po_o", "pm_o", "events"):
                assert np.array_equal(tg[k][sel], tw[k][sel]), f"step {step}: {k}"
    assert (got["steps"][0]["state"]["ac_i"][sel][:, :, 0] != 0).all(), "nothing happens to a spawn state in 16 ticks"


def test_quad_fixture_reaches_every_site(oracle):
    """the 2-vs-2 fixture for the generic kernel (hh_k_world<4, 64, W, false> shares `tick`, QCAP = 8): 1 launch + 3 cannon candidates + 2 fuses on one lane"""
    res = H.quad_oracle_run()
    n, lane_max = res["counts"], res["lane_max"]
    print("2v2 lane_entries_max", int(lane_max.max()), "per arena", lane_max.tolist(), n)
    for a in range(H.QUAD_N):
        assert lane_max[a] >= H.QUAD_LANE[a % 4], f"arena {a} (layout {a % 4}): a lane queues at least {lane_max[a]}"
    assert lane_max.max() >= 6
    for site in H.QUAD_SITES:
        assert n[site] >= 1, f"2-vs-2: the fixture never reaches `{site}`"
    assert not res["faults"].any()
    assert res["outs"][2][:, H.QUAD_N - 1].any(), "the tail arena runs"


def test_edge_bearings_are_undecided(oracle):
    """layout 5: the launch target stands where the planar stage of the launch predicate cannot decide, inside the +-5 deg cannon cone"""
    for km, exact in ((0.6, True), (8.0, True), (8.0, False)):
        b = H.edge_bearing(km, exact)
        print(km, exact, b)
        assert -1.5 < b < -0.5
    assert H.edge_bearing(8.0, True) > -1.0 > H.edge_bearing(8.0, False)


def test_layout_4_is_a_decided_launch(oracle):
    st, _, _ = H.start((3, 3))
    f = st["ac_f"]
    for a in (4, 11, 18):
        pre, exact, _, _ = oracle.missile_cone_planar(f[a, 0:1, 0], f[a, 0:1, 1], f[a, 0:1, 2], f[a, 3:4, 0], f[a, 3:4, 1])
        assert pre[0] == 1 and exact[0] == 1
