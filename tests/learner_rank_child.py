"""One rank of tests/test_gpu_learner_ranks.py, and what that test and tests/test_gpu_learner_sharded.py share: the shards (a level-3
world at its arena offset, a bank and a PPORollout with the sampler's logits recorded), two collect -> update_window -> publish rounds,
and the digest of what they leave — the result dicts and the SHA-256 of every parameter and of Adam's state.

As a program:  python learner_rank_child.py RANK WORLD_SIZE RENDEZVOUS_FILE OUT_FILE
joins a gloo group over the file rendezvous, trains its shard on cuda:0 as one of WORLD_SIZE ranks and writes the digest to OUT_FILE."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HORIZON, T = 10, 24
ARENAS, OFFSETS = (64, 16), (0, 64)         # the two shards of the rank test: the short one runs out of minibatches first
LEARNER = dict(num_sgd_iter=2, sgd_minibatch_size=64, optimizer="fused", grad_clip=0.5, shuffle_sequences=True)


def build_shard(n_arenas, arena_offset, mode="fight", batch_mode="truncate_episodes", seed=23):
    """-> (rollout, bank): level 3, horizon 10, T = 24, record_logits=True; nothing collected yet"""
    import torch
    from hhmarl_2d_amd.pilots import PolicyBank
    from hhmarl_2d_amd.rollout import PPORollout
    from hhmarl_2d_amd.world import World, make_config
    w = World(make_config(n_arenas=n_arenas, level=3, seed=seed, auto_reset=True, horizon=HORIZON, agent_mode=1 if mode == "escape" else 0,
                          arena_offset=arena_offset), device=0)
    bank = PolicyBank.trainable_init(torch.device("cuda", 0), mode=mode, seed=5, max_rows=2 * n_arenas)
    return PPORollout(w, bank, T, record_logits=True, batch_mode=batch_mode), bank


def make_learner(mode="fight", **kw):
    import torch
    from hhmarl_2d_amd.learner import PPOLearner
    return PPOLearner.trainable_init(torch.device("cuda", 0), mode=mode, seed=5, **kw)


def two_rounds(learner, rollouts, banks):
    """collect -> update_window -> publish, twice; rollouts and banks: one of each (a rank, or no group) or a list per local shard"""
    many = isinstance(rollouts, (list, tuple))
    results = []
    for _ in range(2):
        for ro in (rollouts if many else [rollouts]):
            ro.collect()
        results.append(learner.update_window(rollouts, banks))
        for bank in (banks if many else [banks]):
            learner.publish(bank)
    return results


def _walk(h, x, path):
    import torch
    if isinstance(x, dict):
        for k in sorted(x, key=str):
            _walk(h, x[k], f"{path}/{k}")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            _walk(h, v, f"{path}/{i}")
    elif isinstance(x, torch.Tensor):
        h.update(f"{path}:{x.dtype}:{tuple(x.shape)}".encode())
        h.update(x.detach().cpu().reshape(-1).contiguous().view(torch.uint8).numpy().tobytes())
    else:
        h.update(f"{path}={x!r}".encode())


def state_sha256(learner):
    """every parameter and buffer, Adam's m, v and t, kl_coeff and the update count; not the options (they name the group's size)"""
    sd = learner.state_dict()
    h = hashlib.sha256()
    _walk(h, {k: v for k, v in sd.items() if k != "options"}, "")
    return h.hexdigest()


def digest(learner, results):
    """what two ranks and their in-process twin must agree on, as text: the result dicts without rows_local (a rank's own row count, which
    differs between ranks by construction) and the state's SHA-256"""
    shared = [[{k: v for k, v in d.items() if k != "rows_local"} for d in res] for res in results]
    return json.dumps({"results": shared, "state_sha256": state_sha256(learner)}, sort_keys=True, indent=1) + "\n"


def main(argv):
    rank, world_size, rendezvous, out = int(argv[0]), int(argv[1]), argv[2], argv[3]
    for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
        if p not in sys.path:
            sys.path.insert(0, p)
    import datetime
    import torch
    import torch.distributed as dist
    from hhmarl_2d_amd.learner import ShardGroup
    dist.init_process_group("gloo", init_method=f"file://{rendezvous}", rank=rank, world_size=world_size, timeout=datetime.timedelta(seconds=60))
    group = ShardGroup(world_size=world_size)
    ro, bank = build_shard(ARENAS[rank], OFFSETS[rank])
    learner = make_learner(group=group, **LEARNER)
    results = two_rounds(learner, ro, bank)
    torch.cuda.synchronize()
    assert all(d["rows_local"] == T * ARENAS[rank] for res in results for d in res), results
    with open(out, "w") as f:
        f.write(digest(learner, results))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])
