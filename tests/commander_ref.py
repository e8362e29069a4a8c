"""Test infrastructure: a plain-PyTorch restatement of the reference's CommanderGru (models/ac_models_hier.py:70-112) and of
hh_commander_sample's inverse-CDF draw, in float64 or float32, without ray.  Weights are the reference's state_dict
(hhmarl_2d_amd.commander.state_keys)."""
import numpy as np
import torch
import torch.nn.functional as F


def _lin(sd, name, x):
    w, b = sd[f"{name}._model.0.weight"], sd[f"{name}._model.0.bias"]
    return x @ w.T + b


def _gru(sd, rnn, x, h):
    """one step of torch.nn.GRU (gate rows r | z | n)"""
    gi = x @ sd[f"{rnn}.weight_ih_l0"].T + sd[f"{rnn}.bias_ih_l0"]
    gh = h @ sd[f"{rnn}.weight_hh_l0"].T + sd[f"{rnn}.bias_hh_l0"]
    ir, iz, inn = gi.split(200, dim=-1)
    hr, hz, hn = gh.split(200, dim=-1)
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(inn + r * hn)
    return (1.0 - z) * n + z * h


def to_torch(sd, dtype=torch.float64, device="cpu"):
    return {k: torch.as_tensor(np.asarray(v)).to(device=device, dtype=dtype) for k, v in sd.items()}


def forward(sd, obs1, obs2, obs3, act1, act2, act3, h_act, h_val):
    """sd: to_torch(...) weights; obs_k [B, 34], act_k [B, 1], h_* [B, 200] -> (logits [B, 3], value [B], h_act' [B, 200], h_val' [B, 200])"""
    x = torch.cat([torch.tanh(_lin(sd, "inp1", obs1[:, :4])), torch.tanh(_lin(sd, "inp2", obs1[:, 4:24])),
                   torch.tanh(_lin(sd, "inp3", obs1[:, 24:]))], dim=1)
    x_full = torch.tanh(_lin(sd, "inp4", obs1))
    ha = _gru(sd, "rnn_act", x_full, h_act)
    x_full = F.normalize(x_full + ha)
    logits = _lin(sd, "act_out", torch.tanh(_lin(sd, "shared_layer", torch.cat([x, x_full], dim=1))))
    v1, v2, v3 = torch.cat([obs1, act1], 1), torch.cat([obs2, act2], 1), torch.cat([obs3, act3], 1)
    z = torch.cat([torch.tanh(_lin(sd, "v1", v1)), torch.tanh(_lin(sd, "v2", v2)), torch.tanh(_lin(sd, "v3", v3))], dim=1)
    z_full = torch.tanh(_lin(sd, "v4", torch.cat([v1, v2, v3], 1)))
    hv = _gru(sd, "rnn_val", z_full, h_val)
    z_full = F.normalize(z_full + hv)
    value = _lin(sd, "val_out", torch.tanh(_lin(sd, "shared_layer", torch.cat([z, z_full], dim=1))))
    return logits, value.reshape(-1), ha, hv


def observer_rows(obs, crit_act=None):
    """central_critic_observer (train_hier.py:134-165) for every agent of every arena: obs [N, 3, 34], crit_act [N, 3] or None (zeros)
    -> (obs1, obs2, obs3, act1, act2, act3), each [3N, ...] in row order (arena, agent slot)"""
    N = obs.shape[0]
    if crit_act is None:
        crit_act = torch.zeros((N, 3), dtype=obs.dtype, device=obs.device)
    cols = [[], [], []]
    for s in range(3):
        order = [s] + [j for j in range(3) if j != s]
        for k, j in enumerate(order):
            cols[k].append((obs[:, j], crit_act[:, j:j + 1]))
    out_o = [torch.stack([c[0] for c in cols[k]], dim=1).reshape(3 * N, -1) for k in range(3)]
    out_a = [torch.stack([c[1] for c in cols[k]], dim=1).reshape(3 * N, -1) for k in range(3)]
    return out_o[0], out_o[1], out_o[2], out_a[0], out_a[1], out_a[2]


def arena_forward(sd, obs, h, crit_act=None):
    """obs [N, 3, 34], h [N, 3, 2, 200] -> (logits [N, 3, 3], value [N, 3], h_out [N, 3, 2, 200])"""
    N = obs.shape[0]
    o1, o2, o3, a1, a2, a3 = observer_rows(obs, crit_act)
    hf = h.reshape(3 * N, 2, 200)
    lg, v, ha, hv = forward(sd, o1, o2, o3, a1, a2, a3, hf[:, 0], hf[:, 1])
    return lg.reshape(N, 3, 3), v.reshape(N, 3), torch.stack([ha, hv], dim=1).reshape(N, 3, 2, 200)


def inverse_cdf(logits, u):
    """hh_commander_sample's draw in float64: m = max l, S = sum exp(l - m) in index order, t = u S, first i whose running sum
    exceeds t (the last if none); logp = (l_a - m) - log S.  logits [..., 3], u [...] -> (action int64, logp float64)"""
    lg = np.asarray(logits, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    m = lg.max(axis=-1, keepdims=True)
    e = np.exp(lg - m)
    S = e[..., 0] + e[..., 1] + e[..., 2]
    t = u * S
    cum = np.cumsum(e, axis=-1)
    a = np.where(cum[..., 0] > t, 0, np.where(cum[..., 1] > t, 1, 2))
    logp = np.take_along_axis(lg - m, a[..., None], axis=-1)[..., 0] - np.log(S)
    return a.astype(np.int64), logp
