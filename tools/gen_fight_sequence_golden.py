"""
TEST INFRASTRUCTURE — golden vectors for the fight networks in TRAINING form (models/ac_models_hetero.py: Fight1 181-291, Fight2 293-404).

Instantiates the REAL reference classes behind the ray.rllib stand-ins of oracle/gen_policy_golden.py (install_ray_stubs: constructor
bookkeeping, SlimFC = nn.Linear + activation, add_time_dimension = the reshape to [B, T, ...]), loads deterministic synthetic weights
(policy_nets.random_weights / random_critic_weights of SEED, the shared layer of each kind's own draw: only the seed is stored) and
calls forward() + value_function() the way RLlib's learner does: the rows of a padded batch, B x max_seq_len of them, with seq_lens such as
[20, 20, 7] and the last chunk's rows beyond its length all zero — observation, critic inputs and all.  att_act / att_val then attend over
the 20 steps of each chunk, the zero rows included as keys.
Records into tests/golden/fight_sequence_forward.npz, per kind: obs [S, L, D], critic rows [S, L, 57] (rollout.central_critic_rows'
layout), seq_lens, and the reference's logits [S, L, 26 | 24] and values [S, L].  The fixture holds arrays only.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_fight_sequence_golden.py [--check]   (HHMARL_REFERENCE = the reference checkout)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_policy_golden as G  # noqa: E402
from hhmarl_2d_amd import policy_nets as PN  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fight_sequence_forward.npz")
SEED, L = 20261016, 20
SEQ_LENS = {PN.FIGHT1: (20, 20, 7), PN.FIGHT2: (20, 1, 13, 20)}


def synth_rows(rng, kind, seq_lens):
    """obs_own [S, L, d1], critic rows [S, L, a1 + a2 + d1 + d2] with scaled actions, zero beyond each chunk's length"""
    d1, a1, d2, a2 = PN.CRITIC_DIMS[kind]
    S = len(seq_lens)
    own, other = rng.random((S, L, d1), dtype=np.float32), rng.random((S, L, d2), dtype=np.float32)
    other[rng.random((S, L)) < 0.15] = 0.0          # the friend already shot down: an all-zero observation
    act = np.zeros((S, L, 2, 4), np.int8)
    for c, w in enumerate(PN.ACTION_SPLIT):
        act[..., c] = rng.integers(0, w, (S, L, 2))
    sc = PN.scale_actions(act)
    crit = np.concatenate([sc[:, :, 0, :a1], sc[:, :, 1, :a2], own, other], axis=-1).astype(np.float32)
    pad = np.arange(L)[None, :] >= np.asarray(seq_lens)[:, None]
    own[pad] = 0.0
    crit[pad] = 0.0
    return own, crit


def record():
    M = G.reference_models()
    rng = np.random.default_rng(SEED)
    rec, meta = {}, {"seed": SEED, "max_seq_len": L, "source": "models/ac_models_hetero.py Fight1 / Fight2 forward + value_function, learner-style calls"}
    for kind, cls in ((PN.FIGHT1, M.Fight1), (PN.FIGHT2, M.Fight2)):
        name = PN.KIND_NAMES[kind]
        d1, a1, d2, a2 = PN.CRITIC_DIMS[kind]
        m = cls(None, None, PN.N_OUT[kind], {}, name)
        sd = dict(PN.random_weights(kind, SEED), **PN.random_critic_weights(kind, SEED))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.eval()
        own, crit = synth_rows(rng, kind, SEQ_LENS[kind])
        S = own.shape[0]
        flat = torch.from_numpy(crit.reshape(S * L, -1))
        inp = {"obs_1_own": torch.from_numpy(own.reshape(S * L, d1)), "act_1_own": flat[:, :a1], "act_2": flat[:, a1:a1 + a2],
               "obs_2": flat[:, a1 + a2 + d1:]}
        with torch.no_grad():
            out, _ = m(input_dict={"obs": inp}, state=[torch.zeros(S)], seq_lens=torch.tensor(SEQ_LENS[kind]))
            v = m.value_function()
        rec.update({f"{name}_obs": own, f"{name}_critic": crit, f"{name}_seq_lens": np.asarray(SEQ_LENS[kind], np.int32),
                    f"{name}_logits": out.numpy().reshape(S, L, -1), f"{name}_value": v.numpy().reshape(S, L)})
    rec["meta"] = np.array(json.dumps(meta))
    return rec


def main():
    if os.environ.get("HHMARL_REFERENCE"):
        G.REF_ROOT = os.environ["HHMARL_REFERENCE"]
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
