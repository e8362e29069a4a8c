"""References for the window batch (learner.window_cut / window_gather, PPOLearner.window_batch, CommanderLearner.window_sequences),
written from the contract in include/hh_learner.h and DESIGN.md section 24: plain loops and numpy / torch indexing on whatever device
the inputs live on, no kernel and no call into the code under test."""
import numpy as np
import torch


def window_cut_ref(done, L):
    """the three-condition loop: done [T, N] (array or tensor; any non-zero byte is a done) -> (seq_t0, seq_arena, seq_len) int32 arrays,
    arena-major, then time"""
    d = np.asarray(done.cpu() if isinstance(done, torch.Tensor) else done)
    T, N = d.shape
    t0s, arenas, lens = [], [], []
    for n in range(N):
        t0 = 0
        for t in range(T):
            if d[t, n] != 0 or t - t0 + 1 == L or t == T - 1:
                t0s.append(t0); arenas.append(n); lens.append(t - t0 + 1)
                t0 = t + 1
    return np.asarray(t0s, dtype=np.int32), np.asarray(arenas, dtype=np.int32), np.asarray(lens, dtype=np.int32)


def window_fragments(done):
    """the window's fragments as an episode table over arena-major rows r = n T + t: an arena's rows up to and including each done row,
    the last fragment ending at T-1 -> (ep_start, ep_len) int64 arrays"""
    d = np.asarray(done.cpu() if isinstance(done, torch.Tensor) else done)
    T, N = d.shape
    start, length = [], []
    for n in range(N):
        t0 = 0
        for t in range(T):
            if d[t, n] != 0 or t == T - 1:
                start.append(n * T + t0); length.append(t - t0 + 1)
                t0 = t + 1
    return np.asarray(start, dtype=np.int64), np.asarray(length, dtype=np.int64)


def gather_ref(src, t0, arena, ln, L, offset, width, per_seq, T_src=None):
    """hh_window_gather's contract on bytes: src a numpy array [rows, N, ...], of which the call may read T_src rows per arena (default:
    all) -> uint8 [S, L, width] ([S, width] with per_seq); an entry that names no rows of the window gives zeros"""
    Ts, N = src.shape[:2]
    T_src = Ts if T_src is None else T_src
    flat = np.ascontiguousarray(src).reshape(Ts * N, -1).view(np.uint8)
    rows = 1 if per_seq else L
    a, n, k = (np.asarray(x, dtype=np.int64) for x in (t0, arena, ln))
    ok = (a >= 0) & (k >= 0) & (k <= L) & (n >= 0) & (n < N) & (a + k <= T_src)
    j = np.arange(rows, dtype=np.int64)
    keep = ok[:, None] & (j[None, :] < k[:, None])
    r = np.where(keep, (a[:, None] + j[None, :]) * N + n[:, None], 0)
    out = flat[r.reshape(-1), offset:offset + width].reshape(len(a), rows, width).copy()
    out[~keep] = 0
    return out[:, 0] if per_seq else out


def _am(x, T):
    """[T.., N, ...] -> arena-major rows [N T, ...], r = n T + t, contiguous"""
    x = x[:T]
    return x.transpose(0, 1).reshape((x.shape[0] * x.shape[1],) + tuple(x.shape[2:])).contiguous()


def window_rows(ro):
    """a PPORollout-like object's window as an EpisodeBatch.rows()-style dict: arena-major rows of obs[:T], actions, logp, adv, target
    (and logits where recorded), ep_start / ep_len = the fragments"""
    T = ro.T
    out = {k: _am(getattr(ro, k), T) for k in ("obs", "actions", "logp", "adv", "target")}
    if getattr(ro, "record_logits", False):
        out["logits"] = _am(ro.logits, T)
    start, length = window_fragments(ro.done)
    dev = ro.obs.device
    out["ep_start"], out["ep_len"] = torch.from_numpy(start).to(dev), torch.from_numpy(length).to(dev)
    return out


def window_sequences_ref(ro, L):
    """a CommanderRollout-like object's window in CommanderEpisodeBatch.sequences()' format, cut at L: zero padded columns, seq_lens i32,
    mask bool, state_in = ro.state_in[seq_t0, seq_arena], logits where recorded"""
    T, dev = ro.T, ro.obs.device
    t0, arena, ln = (torch.from_numpy(x).to(dev).long() for x in window_cut_ref(ro.done, L))
    j = torch.arange(L, device=dev)
    mask = j[None, :] < ln[:, None]
    tt = torch.where(mask, t0[:, None] + j[None, :], torch.zeros_like(mask, dtype=torch.int64))
    out = {}
    for k in ("obs", "actions", "logp", "vf", "adv", "target") + (("logits",) if getattr(ro, "record_logits", False) else ()):
        g = getattr(ro, k)[tt, arena[:, None].expand_as(tt)]
        out[k] = torch.where(mask.reshape(mask.shape + (1,) * (g.dim() - 2)), g, torch.zeros((), dtype=g.dtype, device=dev))
    out["seq_lens"], out["mask"], out["state_in"] = ln.to(torch.int32), mask, ro.state_in[t0, arena]
    return out
