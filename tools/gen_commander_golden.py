"""
TEST INFRASTRUCTURE — golden vectors for the trainable commander (train_hier.py's CommanderGru, models/ac_models_hier.py:70-112).

Instantiates the REAL reference class behind the ray.rllib stand-ins of oracle/gen_policy_golden.py (install_ray_stubs: constructor
bookkeeping, SlimFC = nn.Linear + activation, add_time_dimension), loads deterministic synthetic weights
(hhmarl_2d_amd.commander.random_weights(SEED): only the seed is stored) and calls forward() + value_function() the way RLlib's sampler
does (time dimension 1, seq_lens ones, every agent's state_out fed back as its next state_in, zero states at an episode start).
Records into tests/golden/commander_gru.npz:
  (a) a K-step chain of N arenas x 3 agent rows on central_critic_observer's dict with zero action inputs: obs rows with zero blocks,
      all-zero (dead) rows, and arenas whose state is reset mid-chain (`fresh`); per step and row the state in / out, logits, value,
      a uniform and the float64 inverse-CDF action / logp of hh_commander_sample's definition on the reference's logits — logits and
      value at every step, the states out at CK_STEPS (the state in of step t + 1 is that of step t, or zero where `fresh`);
  (b) step 8 again with non-zero act_* inputs (the value branch's action columns);
  (c) one multi-step call (seq_lens = [L]) of one agent row, which must equal its step-by-step chain.
The fixture holds data only.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_commander_golden.py [--check]
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from gen_policy_golden import install_ray_stubs  # noqa: E402
from hhmarl_2d_amd import commander as CM  # noqa: E402
import commander_ref as CR  # noqa: E402

REF_ROOT = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "commander_gru.npz")
SEED, N_ARENAS, K, L_MULTI = 20261015, 16, 32, 16
CK_STEPS = (0, 7, 8, 15, 16, 31)   # steps whose state_out is stored (the whole chain's would be 2.4 MB of noise): teacher forcing
                                     # runs the steps that follow them, the free-running chain is compared at each


def reference_model():
    sys.dont_write_bytecode = True
    install_ray_stubs()
    if REF_ROOT not in sys.path:
        sys.path.insert(0, REF_ROOT)
    from models import ac_models_hier as M
    m = M.CommanderGru(None, None, 3, {}, "commander")
    sd = CM.random_weights(SEED)
    ref_keys = {k: list(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.eval()
    return m, ref_keys


def call(m, obs, crit_act, h, seq_lens=None):
    """obs [N, 3, 34], crit_act [N, 3], h [N, 3, 2, 200] (numpy f32) -> logits [N, 3, 3], value [N, 3], h_out [N, 3, 2, 200]"""
    N = obs.shape[0]
    o1, o2, o3, a1, a2, a3 = CR.observer_rows(torch.from_numpy(obs), torch.from_numpy(crit_act))
    inp = {"obs_1_own": o1, "obs_2": o2, "obs_3": o3, "act_1_own": a1, "act_2": a2, "act_3": a3}
    hf = torch.from_numpy(h).reshape(3 * N, 2, 200)
    with torch.no_grad():
        out, st = m(input_dict={"obs": inp}, state=[hf[:, 0], hf[:, 1]], seq_lens=torch.ones(3 * N, dtype=torch.int32))
        v = m.value_function()
    return (out.numpy().reshape(N, 3, 3), v.numpy().reshape(N, 3),
            torch.stack([st[0], st[1]], dim=1).numpy().reshape(N, 3, 2, 200))


def synth_obs(rng, N):
    o = rng.random((N, 3, 34), dtype=np.float32)
    o[rng.random((N, 3)) < 0.15, 4:24] = 0.0          # no opponent in sensing range: zero block
    o[rng.random((N, 3)) < 0.10, 24:] = 0.0
    o[rng.random((N, 3)) < 0.10] = 0.0                # dead agent: an all-zero row
    o[1, 2] = 0.0
    return o


def record():
    m, ref_keys = reference_model()
    rng = np.random.default_rng(SEED)
    N = N_ARENAS
    obs = np.stack([synth_obs(rng, N) for _ in range(K)])
    fresh = np.zeros((K, N), np.uint8)
    fresh[0] = 1
    fresh[8, 3] = fresh[12, [5, 9]] = fresh[20, 3] = fresh[27, 14] = 1    # episodes restarting mid-chain
    uni = rng.random((K, N, 3))
    h_in = np.zeros((K, N, 3, 2, 200), np.float32)
    h_out = np.zeros_like(h_in)
    logits = np.zeros((K, N, 3, 3), np.float32)
    value = np.zeros((K, N, 3), np.float32)
    h = np.zeros((N, 3, 2, 200), np.float32)
    zero_act = np.zeros((N, 3), np.float32)
    for t in range(K):
        h = np.where(fresh[t][:, None, None, None] != 0, 0.0, h).astype(np.float32)
        h_in[t] = h
        logits[t], value[t], h_out[t] = call(m, obs[t], zero_act, h)
        h = h_out[t]
    action, logp = CR.inverse_cdf(logits.astype(np.float64), uni)
    # (b) non-zero action inputs (on_postprocess_trajectory writes action / 2 into act_*)
    b_act = (rng.integers(0, 3, (N, 3)) / 2.0).astype(np.float32)
    b_obs, b_h = obs[8], h_in[8]
    b_logits, b_value, b_hout = call(m, b_obs, b_act, b_h)
    # (c) one sequence of L steps of arena 0 / agent 1 in one call (seq_lens = [L]); no reset of arena 0 before step L
    assert not fresh[1:L_MULTI, 0].any()
    o1 = torch.from_numpy(obs[:L_MULTI, 0, 0])
    inp = {"obs_1_own": o1, "obs_2": torch.from_numpy(obs[:L_MULTI, 0, 1]), "obs_3": torch.from_numpy(obs[:L_MULTI, 0, 2]),
           "act_1_own": torch.zeros((L_MULTI, 1)), "act_2": torch.zeros((L_MULTI, 1)), "act_3": torch.zeros((L_MULTI, 1))}
    with torch.no_grad():
        out, st = m(input_dict={"obs": inp}, state=[torch.zeros((1, 200)), torch.zeros((1, 200))], seq_lens=torch.tensor([L_MULTI]))
        mv = m.value_function()
    meta = {"seed": SEED, "n_arenas": N, "K": K, "L_multi": L_MULTI, "ref_keys": ref_keys, "b_step": 8,
            "source": "models/ac_models_hier.py:CommanderGru forward + value_function, sampler-style calls"}
    return dict(meta=np.array(json.dumps(meta)), obs=obs, fresh=fresh, uniforms=uni, ck_steps=np.array(CK_STEPS, np.int32), h_out_ck=h_out[list(CK_STEPS)],
                logits=logits, value=value, action=action.astype(np.int8), logp=logp, b_act=b_act, b_logits=b_logits, b_value=b_value, b_hout=b_hout,
                m_logits=out.numpy(), m_value=mv.numpy(), m_hact=st[0].numpy()[0], m_hval=st[1].numpy()[0])


def main():
    rec = record()
    if "--check" in sys.argv:
        g = np.load(OUT)
        bad = [k for k in rec if k != "meta" and not np.array_equal(g[k], rec[k])]
        if bad or json.loads(str(g["meta"])) != json.loads(str(rec["meta"])):
            print("MISMATCH:", bad)
            sys.exit(1)
        print(f"{OUT}: regenerated and identical")
        return
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
