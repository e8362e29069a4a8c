"""Host restatement of the whole-episode batches (test infrastructure): what RLlib 2.4 hands its learner with batch_mode =
"complete_episodes", for a sequence of collects after one start() — PPORollout's EpisodeBatch (train_hetero.py:212) and, with the
recurrent CommanderGru, CommanderRollout's CommanderEpisodeBatch (train_hier.py:182).  Episodes: the [T, N, ...] windows concatenated per
arena, cut after every done row (the next row is the next episode's reset row); adv / target: oracle/gae_ref.compute_advantages(last_r =
0.0) per episode and agent.  Sequences (max_seq_len set): chop_into_sequences (rllib/policy/rnn_sequencing.py) on each agent's
trajectory, one episode at a time — a new sequence at the episode's first row and after every max_seq_len rows — and the state-in view
of its agent collector: a sequence's state_in_k is state_in_k of its first row, which is the state the sampler's forward used at that
step.  The three agents of an arena share their episode's cut, so one sequence entry covers the arena row and its states [3, 2, 200];
RLlib's per-agent batch is the slice [:, a]."""
import numpy as np

IN_COLS = ("obs", "actions", "logp", "vf", "reward", "valid", "done", "state_in")
ROW_COLS = ("obs", "actions", "logp", "vf", "reward", "valid")
OUT_COLS = ROW_COLS + ("adv", "target", "done", "arena", "episode", "t")
TABLE = ("ep_start", "ep_len", "ep_arena")
SEQ_TABLE = ("seq_start", "seq_len", "seq_ep")


def restate(collects, max_seq_len=None, *, gamma=0.99, lam=1.0):
    """collects: dicts of one collect's [T, N, ...] buffers (obs / vf (/ state_in) cut to their first T rows; state_in only with
    max_seq_len).  gamma / lam: keyword only (the rollouts' defaults differ: PPORollout lam 0.95, CommanderRollout RLlib's 1.0).
    -> (one dict per collect: OUT_COLS of the episodes that end in it (arena-major, then episode, then time) and, with max_seq_len, the
        episode table TABLE (rows of this collect's batch), the sequence table SEQ_TABLE (seq_ep indexes this collect's episode table)
        and state_in [S, 3, 2, 200]; carried [N]: rows of every arena's running episode after the last collect)"""
    import gae_ref
    T, N = collects[0]["done"].shape
    cols = [k for k in IN_COLS if max_seq_len is not None or k != "state_in"]
    cat = {k: np.concatenate([c[k] for c in collects], axis=0) for k in cols}
    nA = cat["reward"].shape[2]
    start, ep = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    keys = OUT_COLS if max_seq_len is None else OUT_COLS + TABLE + SEQ_TABLE + ("state_in",)
    out = []
    for ci in range(len(collects)):
        parts = {k: [] for k in keys}
        rows = eps = 0
        for n in range(N):
            for g in np.nonzero(cat["done"][ci * T:(ci + 1) * T, n])[0] + ci * T:
                s0 = int(start[n])
                E = int(g) + 1 - s0
                sl = slice(s0, s0 + E)
                adv, tgt = np.zeros((E, nA), dtype=np.float32), np.zeros((E, nA), dtype=np.float32)
                for a in range(nA):
                    adv[:, a], tgt[:, a] = gae_ref.compute_advantages(cat["reward"][sl, n, a], cat["vf"][sl, n, a], 0.0, gamma, lam)
                for k in ROW_COLS:
                    parts[k].append(cat[k][sl, n])
                done = np.zeros(E, dtype=np.uint8)
                done[-1] = 1
                parts["adv"].append(adv)
                parts["target"].append(tgt)
                parts["done"].append(done)
                parts["arena"].append(np.full(E, n, dtype=np.int32))
                parts["episode"].append(np.full(E, ep[n], dtype=np.int32))
                parts["t"].append(np.arange(E, dtype=np.int32))
                if max_seq_len is not None:
                    L = int(max_seq_len)
                    parts["ep_start"].append(np.array([rows], dtype=np.int32))
                    parts["ep_len"].append(np.array([E], dtype=np.int32))
                    parts["ep_arena"].append(np.array([n], dtype=np.int32))
                    for j0 in range(0, E, L):   # chop_into_sequences: a new sequence at the episode's start and after every L rows
                        parts["seq_start"].append(np.array([rows + j0], dtype=np.int32))
                        parts["seq_len"].append(np.array([min(L, E - j0)], dtype=np.int32))
                        parts["seq_ep"].append(np.array([eps], dtype=np.int32))
                        parts["state_in"].append(cat["state_in"][s0 + j0, n][None])
                rows += E
                eps += 1
                ep[n] += 1
                start[n] = g + 1
        empty = {k: cat[k][:0, 0] for k in cols if k != "done"}
        empty.update({"adv": np.zeros((0, nA), np.float32), "target": np.zeros((0, nA), np.float32), "done": np.zeros(0, np.uint8)})
        out.append({k: np.concatenate(v, axis=0) if v else empty.get(k, np.zeros(0, np.int32)) for k, v in parts.items()})
    return out, (len(collects) * T - start).astype(np.int32)


def pad_sequences(batch, max_seq_len):
    """the learner's padded form of one restated batch: each column [S, L, ...] zero past seq_len, seq_lens [S], mask [S, L]"""
    L = int(max_seq_len)
    S = len(batch["seq_start"])
    mask = np.arange(L)[None, :] < batch["seq_len"][:, None]
    res = {"seq_lens": batch["seq_len"], "mask": mask, "state_in": batch["state_in"]}
    for k in ("obs", "actions", "logp", "vf", "adv", "target"):
        col = batch[k]
        p = np.zeros((S, L) + col.shape[1:], dtype=col.dtype)
        for s in range(S):
            n = batch["seq_len"][s]
            p[s, :n] = col[batch["seq_start"][s]:batch["seq_start"][s] + n]
        res[k] = p
    return res
