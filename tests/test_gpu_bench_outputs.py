"""-m gpu: `bench.py --dump-outputs DIR` writes what the timed launches computed, and the same arguments give the same arrays: the
warm-up and timed launches start from the state right after reset, however many launches the clock spin-up before them took."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, CHUNK, STEPS, WARMUP, SEED = 512, 40, 3, 1, 1234
NAMES = ("obs", "reward", "reward_valid", "done")


def _bench(d, spinup):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--arenas", str(N),
                        "--chunk", str(CHUNK), "--seed", str(SEED), "--spinup", spinup, "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_dumped_outputs_repeat_and_are_the_oracles_last_tick(tmp_path, oracle):
    a, b = _bench(tmp_path / "a", "0"), _bench(tmp_path / "b", "0.5")
    assert a["steps"] == STEPS and a["ms_per_step"] > 0 and "extra" not in a and "cpu_baseline" not in a
    files = a["dump_outputs"]["files"]
    assert sorted(files) == sorted(os.listdir(tmp_path / "a")) == sorted(f"{n}{s}.npy" for n in NAMES for s in ("", "_last"))
    got = {}
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32 and x.shape == y.shape and np.array_equal(x, y), f
        got[f[:-4]] = x
    assert got["obs_last"].shape == (N, 2, 26) and got["obs"].shape == (CHUNK, 256, 2, 26) and got["done"].shape == (CHUNK, 256)
    # the launches ran ticks [0, (WARMUP + STEPS) x CHUNK) of the keyed tape from reset: the oracle's last tick of the same tape is the dump's
    o = oracle.OracleWorld(oracle.make_config(n_arenas=N, level=3, seed=SEED, auto_reset=True))
    o.reset()
    want = o.rollout(oracle.action_tape_uniform(SEED, 0, 0, (WARMUP + STEPS) * CHUNK, N, o.n_ctrl))
    for name, w in zip(NAMES, want):
        assert np.array_equal(got[name + "_last"], w[-1].astype(np.float32)), name
    # the sampled arenas' series ends in rows of the last tick
    last = got["obs_last"].reshape(N, -1)
    for row in got["obs"][-1].reshape(256, -1):
        assert (last == row).all(axis=1).any()
