"""The table of compiled world-kernel instances: which template instance of the seven world-kernel families (hh_k_world_quad, hh_k_world,
hh_k_hier, hh_k_hier_oct, hh_k_hier_oct_v, hh_k_hier_macro, hh_k_hier_macro_oct) runs under which switches, configuration, arena counts and
call path.  test_kernel_instances.py (CPU) proves the table names exactly the instances the library holds; test_gpu_kernel_instances.py runs
every row against the CPU oracle.

A row is a dict:

    instances   the compiled instances the row runs, spelled the way a profiler prints them ("hh_k_world_quad<1, 1, true, 8, true, true>")
    printed     what World.kernel_instance(which) prints for the row's world, or None where hh_kernel_instance cannot name what runs: the split
                step's hh_k_world<4, 64, 1, true> and the variant-row launches (it names the world's rollout / phase kernel instead).  The phase
                launches are printed as "hh_k_hier_oct<W, phase>": one string for the four instances of a row
    which       the argument of kernel_instance(): 0 rollout / step / phase launches, 1 hh_hl_rollout
    env         the HH_* switches that select the instance (every other switch of SWITCHES is set to "0")
    config      2-vs-2: a key of test_quad_select_paths.CONFIGS, or "l4-split"; HighLevelEnv: a key of HL_CONFIGS
    sizes       arena counts
    path        "rollout" | "split-step" | "phases" | "hl_rollout" | "variant-rows"

The switches force every form at small arena counts; which form the launcher picks by the arena count alone is checked at the boundaries
(test_gpu_kernel_instances.py::test_dispatch_boundaries_*).
"""
SWITCHES = ("HH_FORCE_W", "HH_APW", "HH_NO_QUAD", "HH_NO_SPEC", "HH_NO_TWO", "HH_NO_OCT", "HH_NO_DUAL", "HH_NO_OWT")
FAMILIES = ("hh_k_world_quad", "hh_k_world", "hh_k_hier", "hh_k_hier_oct", "hh_k_hier_oct_v", "hh_k_hier_macro", "hh_k_hier_macro_oct")

# ---- 2-vs-2: the fixtures of test_quad_select_paths.py.  8 = one full group of the 8-arena forms, 9 = a one-arena tail behind it (and a partial wave
# of the 16-arena forms), 17 = one full 16-arena wave and a one-arena tail
SIZES8, SIZES16 = (8, 9), (9, 17)
# configuration -> PRE of the instance compiled for it (0: none, the general instance)
PRESET = {"l3": 1, "l3-stay-done": 1, "l1": 2, "l2": 3, "l3-escape": 4, "l3-general": 0, "l3-escape-shaping": 0}
L4_SPLIT = dict(level=4, ext_opp_actions=True, auto_reset=True, horizon=70)   # frozen-policy opponents: hh_step_begin / hh_step_finish


def _q(W, pre, two, apw, dual, shape):
    b = ("false", "true")
    return f"hh_k_world_quad<{W}, {pre}, {b[two]}, {apw}, {b[dual]}, {b[shape]}>"


def _row(instances, printed, env, config, sizes, path, which=0):
    return dict(instances=tuple(instances), printed=printed, which=which, env=dict(env), config=config, sizes=tuple(sizes), path=path)


def _rollout(instance, env, config, sizes):
    return _row([instance], instance, env, config, sizes, "rollout")


QUAD_ROWS = []
for _cfg, _pre in PRESET.items():
    _shaping = _cfg == "l3-escape-shaping"   # the one configuration whose general instance keeps the pair table on the simulation wave (SHAPE = true)
    _shape = _pre != 0 or _shaping
    QUAD_ROWS += [
        # single wave: no output wave
        _rollout(_q(1, _pre, False, 16, False, True), dict(HH_NO_TWO="1"), _cfg, SIZES16),
        # two waves per SIMD: what large worlds run (above 16 arenas x SIMD count), single wave
        _rollout(_q(2, _pre, False, 16, False, True), dict(HH_FORCE_W="2"), _cfg, SIZES16),
        # simulation wave + output wave, 8 arenas per wave, helper lanes: the default of small worlds
        _rollout(_q(1, _pre, True, 8, True, _shape), dict(), _cfg, SIZES8),
        # the same without helper lanes
        _rollout(_q(1, _pre, True, 8, False, _shape), dict(HH_NO_DUAL="1"), _cfg, SIZES8),
        # simulation wave + output wave, 16 arenas per wave: compiled for the headline preset and the general configuration only
        _rollout(_q(1, 1, True, 16, False, True) if _pre == 1 else _q(1, 0, True, 16, False, _shaping), dict(HH_APW="16"), _cfg, SIZES16),
    ]
QUAD_ROWS += [
    # HH_NO_OWT=1: a configuration without shaping on the SHAPE = true general instances (pair table on the simulation wave)
    _rollout(_q(1, 0, True, 8, True, True), dict(HH_NO_OWT="1"), "l3-general", SIZES8),
    _rollout(_q(1, 0, True, 8, False, True), dict(HH_NO_OWT="1", HH_NO_DUAL="1"), "l3-general", SIZES8),
    _rollout(_q(1, 0, True, 16, False, True), dict(HH_NO_OWT="1", HH_APW="16"), "l3-general", SIZES16),
    # HH_NO_SPEC=1: a preset's configuration on the general instance
    _rollout(_q(1, 0, True, 8, True, False), dict(HH_NO_SPEC="1"), "l3", SIZES8),
    _rollout(_q(2, 0, False, 16, False, True), dict(HH_NO_SPEC="1", HH_FORCE_W="2"), "l3-escape", SIZES16),
    # HH_NO_QUAD=1: the generic LDS-exchange kernel
    _rollout("hh_k_world<4, 64, 1, false>", dict(HH_NO_QUAD="1"), "l3", SIZES16),
    _rollout("hh_k_world<4, 64, 2, false>", dict(HH_NO_QUAD="1", HH_FORCE_W="2"), "l3", SIZES16),
    # the split step of levels 4-5: hh_kernel_instance names the world's rollout kernel, not this one — the call path reaches it
    _row(["hh_k_world<4, 64, 1, true>"], None, dict(), "l4-split", SIZES16, "split-step"),
]

# ---- HighLevelEnv: 170 arenas (a partial last group at 8 and at 10 arenas per wave), 12 commander steps
HL_N, HL_STEPS = 170, 12
HL_CONFIGS = {
    "general": dict(horizon=60),                    # any configuration but the reference's default: HLD = false
    "default": dict(horizon=500),                   # the compiled-in default configuration: HLD = true
    "4v4": dict(horizon=60, n_agents=4, n_opps=4),  # more than three aircraft on a side: ten unit slots, LDS-exchange kernels only
}


def _oct4(W):
    return [f"hh_k_hier_oct<{W}, {ph}>" for ph in range(4)]   # HH_HL_BEGIN, HH_HL_AGENTS_ACT, HH_HL_TICK, HH_HL_END


def _hl(instances, printed, env, config, path):
    return _row(instances, printed, env, config, (HL_N,), path, which=1 if path == "hl_rollout" else 0)


def _macro(instance, env, config):
    return _hl([instance], instance, env, config, "hl_rollout")


_W2, _LDS, _LDS_W2, _LDS_10 = dict(HH_FORCE_W="2"), dict(HH_NO_OCT="1"), dict(HH_NO_OCT="1", HH_FORCE_W="2"), dict(HH_NO_OCT="1", HH_APW="16")
HIER_ROWS = [
    # register-exchange kernels (the default): one arena per 8-lane group; HH_APW plays no part
    _hl(_oct4(1), "hh_k_hier_oct<1, phase>", dict(), "general", "phases"),
    _hl(_oct4(1), "hh_k_hier_oct<1, phase>", dict(), "default", "phases"),
    _hl(_oct4(2), "hh_k_hier_oct<2, phase>", _W2, "general", "phases"),
    _hl(_oct4(2), "hh_k_hier_oct<2, phase>", _W2, "default", "phases"),
    _macro("hh_k_hier_macro_oct<1, false>", dict(), "general"),
    _macro("hh_k_hier_macro_oct<1, true>", dict(), "default"),
    _macro("hh_k_hier_macro_oct<2, false>", _W2, "general"),
    _macro("hh_k_hier_macro_oct<2, true>", _W2, "default"),
    # the variant-row launches (hh_hl_begin_variants / hh_hl_act_tick): hh_kernel_instance names the world's phase kernel, not these
    _hl(["hh_k_hier_oct_v<2, 7, 8>", "hh_k_hier_oct_v<2, 6, 8>"], None, dict(), "general", "variant-rows"),
    # LDS-exchange kernels (HH_NO_OCT=1): ten arenas per wave in the phase kernel; the macro step runs 8 per wave at this size unless HH_APW=16
    _hl(["hh_k_hier<6, 64, 1>"], "hh_k_hier<6, 64, 1>", _LDS, "general", "phases"),
    _hl(["hh_k_hier<6, 64, 1>"], "hh_k_hier<6, 64, 1>", _LDS, "default", "phases"),
    _hl(["hh_k_hier<6, 64, 2>"], "hh_k_hier<6, 64, 2>", _LDS_W2, "general", "phases"),
    _hl(["hh_k_hier<6, 64, 2>"], "hh_k_hier<6, 64, 2>", _LDS_W2, "default", "phases"),
    _hl(["hh_k_hier<6, 64, 1>"], "hh_k_hier<6, 64, 1>", _LDS_10, "general", "phases"),
    _hl(["hh_k_hier<6, 64, 1>"], "hh_k_hier<6, 64, 1>", _LDS_10, "default", "phases"),
    _macro("hh_k_hier_macro<6, 64, 1, false, 8>", _LDS, "general"),
    _macro("hh_k_hier_macro<6, 64, 1, true, 8>", _LDS, "default"),
    _macro("hh_k_hier_macro<6, 64, 2, false, 10>", _LDS_W2, "general"),
    _macro("hh_k_hier_macro<6, 64, 2, true, 10>", _LDS_W2, "default"),
    _macro("hh_k_hier_macro<6, 64, 1, false, 10>", _LDS_10, "general"),
    _macro("hh_k_hier_macro<6, 64, 1, true, 10>", _LDS_10, "default"),
    # ten unit slots
    _hl(["hh_k_hier<10, 64, 1>"], "hh_k_hier<10, 64, 1>", dict(), "4v4", "phases"),
    _macro("hh_k_hier_macro<10, 64, 1, false, 6>", dict(), "4v4"),
]

ROWS = QUAD_ROWS + HIER_ROWS


def switches(row):
    """every switch of SWITCHES with the row's value, "0" where the row does not set it"""
    return {k: row["env"].get(k, "0") for k in SWITCHES}


def family(instance):
    return instance.split("<")[0]


def table_instances():
    return {i for r in ROWS for i in r["instances"]}


def hl_settings():
    """the HighLevelEnv rows grouped by world: [(env, config, {path: row})] — the phase path and hh_hl_rollout of one setting run from the same tape"""
    out = []
    for r in HIER_ROWS:
        key = (tuple(sorted(r["env"].items())), r["config"])
        for k, paths in out:
            if k == key:
                assert r["path"] not in paths, f"two rows for {key} / {r['path']}"
                paths[r["path"]] = r
                break
        else:
            out.append((key, {r["path"]: r}))
    return [(dict(k[0]), k[1], paths) for k, paths in out]


def row_id(row):
    sw = ",".join(f"{k[3:]}={v}" for k, v in sorted(row["env"].items())) or "default"
    return f"{row['config']}-{row['path']}-{sw}"
