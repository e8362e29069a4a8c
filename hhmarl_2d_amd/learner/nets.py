"""The trainable networks: the four 2-vs-2 architectures (TrainableNet) and the commander's (CommanderTrainable)"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import policy_nets as PN
from .loss import _heads_mode
from .ops import (ATTENTION_MODES, COMMANDER_STAGE_LAYERS, GRU_H, INPUT_MODES, _trunk_mode, attention_block, chunk_attention, commander_stage_tables,
                  dense_tanh, gru_sequence_pair, gru_sequence_torch, input_stage, residual_normalize, stage_groups, stage_layers, stage_tables)

# ------------------------------------------------------------------------------------------------------------------ the networks
class _FC(nn.Module):
    """a linear layer under the reference's parameter names (RLlib's SlimFC keeps its nn.Linear in `_model.0`)"""

    def __init__(self, n_in, n_out):
        super().__init__()
        self._model = nn.Sequential(nn.Linear(n_in, n_out))

    def forward(self, x):
        return self._model(x)


class TrainableNet(nn.Module):
    """One of the four trainable architectures (policy_nets: Fight1 / Fight2 / Esc1 / Esc2) in training form, written from the architecture
    tables of policy_nets.py; parameters named and shaped exactly as actor_keys(kind) + critic_keys(kind), so `state_dict()` goes
    straight into `PolicyBank.refresh`.

    forward(obs_own, critic_row) -> (logits, value):
      fight kinds:  obs_own [S, L, >= OBS_DIM] and critic_row [S, L, 57] are chunks of L consecutive steps of one agent; att_act / att_val
                    attend over the L steps of a chunk with no padding mask (a zero-padded row is a key like any other), then
                    normalize(x + att) per row.  2-D inputs [R, ...] are R chunks of length 1 — the sampler's forward.
                    -> logits [S, L, 26 | 24], value [S, L]
      escape kinds: rows [..., >= OBS_DIM], [..., 66] -> logits [..., 26 | 24], value [...]
    critic_row is rollout.central_critic_rows' layout: [own act | friend's act | own obs | friend's obs].

    attention = "torch" (the default) runs att_act / att_val through nn.MultiheadAttention and F.normalize.  "fused" (fight kinds only,
    float32 on the GPU) keeps the two projections as GEMMs and runs what lies between and after them through chunk_attention and
    residual_normalize; "block" (the same conditions) runs each whole block, projections included, as ONE attention_block.  The
    nn.MultiheadAttention objects stay the parameter holders, so state_dict() is the same in all three.

    inputs = "torch" (the default) slices, concatenates and runs inp1..inp3 and v1..v3 / inp1_val one by one.  "fused" (any kind, float32
    on the GPU) runs each side's layers as ONE input_stage that reads obs_own / critic_row as they are and writes the concatenated
    activations (stage_tables(kind)); the _FC modules stay the parameter holders.  Independent of `attention`.

    trunk = "torch" (the default) applies shared_layer and tanh to the actor's and to the critic's rows one after the other.  "fused" (any
    kind, float32 on the GPU) runs both through ONE dense_tanh (split-fp16 MFMA, bias and tanh in its epilogue); the _FC module stays
    the parameter holder, so state_dict(), tie and publish are the same, and a tied layer receives gradients only from the module that
    ran.  Independent of `attention` and `inputs`.

    heads = "torch" (the default) changes nothing.  "fused" (any kind, trunk="torch") marks the module for the learners' fused tail:
    `pre_heads(obs_own, critic_row) -> (za, zc)` is everything up to shared_layer's pre-activations, and heads_loss takes it from there
    with this module's act_out and val_out.  `forward` is the same code and returns the same bytes in both modes (the sampler-form
    forward, old_logits and the golden-file tests use it); state_dict() is the same."""

    def __init__(self, kind, attention="torch", inputs="torch", trunk="torch", heads="torch"):
        super().__init__()
        self.kind = int(kind)
        self.trunk = _trunk_mode(trunk)
        self.heads = _heads_mode(heads, self.trunk)
        if inputs not in INPUT_MODES:
            raise ValueError(f"inputs is one of {INPUT_MODES}, got {inputs!r}")
        self.inputs = inputs
        if attention not in ATTENTION_MODES:
            raise ValueError(f"attention is one of {ATTENTION_MODES}, got {attention!r}")
        if attention != "torch" and not PN.HAS_ATT[self.kind]:
            raise ValueError(f'attention="{attention}": {PN.KIND_NAMES[self.kind]} has no attention')
        self.attention = attention
        for i, (c0, c1, w) in enumerate(PN.INPUTS[kind]):
            setattr(self, f"inp{i + 1}", _FC(c1 - c0, w))
        self.shared_layer = _FC(500, 500)
        self.act_out = _FC(500, PN.N_OUT[kind])
        d1, a1, d2, a2 = PN.CRITIC_DIMS[kind]
        if PN.HAS_ATT[kind]:
            self.att_act = nn.MultiheadAttention(100, 2, batch_first=True)
            self.v1, self.v2, self.v3 = _FC(d1 + a1, 175), _FC(d2 + a2, 175), _FC(d1 + a1 + d2 + a2, 150)
            self.att_val = nn.MultiheadAttention(150, 2, batch_first=True)
        else:
            self.inp1_val = _FC(d1 + a1 + d2 + a2, 500)
        self.val_out = _FC(500, 1)

    @staticmethod
    def _attend_fused(att, h):
        """normalize(h + att(h, h, h)) with the in- and out-projection as GEMMs and the rest in two fused launches each way"""
        qkv = F.linear(h, att.in_proj_weight, att.in_proj_bias)
        out = F.linear(chunk_attention(qkv), att.out_proj.weight, att.out_proj.bias)
        return residual_normalize(h, out)

    @staticmethod
    def _attend_block(att, h):
        """normalize(h + att(h, h, h)) as one attention_block: one launch forward, two backward, the projections inside"""
        return attention_block(h, att.in_proj_weight, att.in_proj_bias, att.out_proj.weight, att.out_proj.bias)

    @staticmethod
    def _attend_torch(att, h):
        """normalize(h + att(h, h, h)) through nn.MultiheadAttention and F.normalize"""
        a, _ = att(h, h, h, need_weights=False)
        return F.normalize(h + a, dim=-1)

    def _front(self, obs_own, critic_row):
        """-> (h, y, flat): the actor's and the critic's rows as shared_layer sees them; flat: 2-D fight inputs, run as chunks of length 1"""
        kind = self.kind
        flat = PN.HAS_ATT[kind] and obs_own.dim() == 2
        if flat:
            obs_own, critic_row = obs_own[:, None], critic_row[:, None]
        # the front: h and y are the pieces that shared_layer sees side by side; a fight kind's last piece goes through its attention block first
        if self.inputs == "fused":
            tables, layers = stage_tables(kind), stage_layers(kind)
            h = list(input_stage(obs_own.contiguous(), *stage_groups(self, layers["actor"], tables["actor"])))
            y = list(input_stage(critic_row.contiguous(), *stage_groups(self, layers["critic"], tables["critic"])))
        else:
            d1, a1, d2, a2 = PN.CRITIC_DIMS[kind]
            x = obs_own[..., :PN.OBS_DIM[kind]]
            h = [torch.tanh(getattr(self, f"inp{i + 1}")(x[..., c0:c1])) for i, (c0, c1, _) in enumerate(PN.INPUTS[kind])]
            act_own, act_2 = critic_row[..., :a1], critic_row[..., a1:a1 + a2]
            o_own, o_2 = critic_row[..., a1 + a2:a1 + a2 + d1], critic_row[..., a1 + a2 + d1:]
            v1, v2 = torch.cat((o_own, act_own), dim=-1), torch.cat((o_2, act_2), dim=-1)
            v3 = torch.cat((v1, v2), dim=-1)
            if PN.HAS_ATT[kind]:
                y = [torch.cat((torch.tanh(self.v1(v1)), torch.tanh(self.v2(v2))), dim=-1), torch.tanh(self.v3(v3))]
            else:
                y = [torch.tanh(self.inp1_val(v3))]
        if PN.HAS_ATT[kind]:
            attend = {"fused": self._attend_fused, "block": self._attend_block, "torch": self._attend_torch}[self.attention]
            h[-1], y[-1] = attend(self.att_act, h[-1]), attend(self.att_val, y[-1])
        h, y = (t[0] if len(t) == 1 else torch.cat(t, dim=-1) for t in (h, y))
        return h, y, flat

    def pre_heads(self, obs_own, critic_row):
        """forward up to shared_layer's pre-activations -> (za, zc) [..., 500] (fight kinds: [S, L, 500], or [R, 500] for 2-D inputs):
        what heads_loss takes.  trunk="torch" only: dense_tanh keeps no pre-activation."""
        if self.trunk == "fused":
            raise ValueError('pre_heads needs trunk="torch": dense_tanh has the tanh inside')
        h, y, flat = self._front(obs_own, critic_row)
        za, zc = self.shared_layer(h), self.shared_layer(y)
        return (za.squeeze(1), zc.squeeze(1)) if flat else (za, zc)

    def forward(self, obs_own, critic_row):
        h, y, flat = self._front(obs_own, critic_row)
        if self.trunk == "fused":
            lin = self.shared_layer._model[0]
            h, y = dense_tanh((h, y), lin.weight, lin.bias)
            logits, value = self.act_out(h), self.val_out(y).squeeze(-1)
        else:
            logits = self.act_out(torch.tanh(self.shared_layer(h)))
            value = self.val_out(torch.tanh(self.shared_layer(y))).squeeze(-1)
        if flat:
            logits, value = logits[:, 0], value[:, 0]
        return logits, value

    def load_numpy(self, sd):
        """the weights of a dict of numpy arrays keyed like state_dict() (policy_nets.random_weights + random_critic_weights)"""
        own = self.state_dict()
        with torch.no_grad():
            for k, v in sd.items():
                own[k].copy_(torch.as_tensor(np.asarray(v)))
        return self


def tie(modules):
    """make every module hold the FIRST one's shared_layer: ONE parameter object for all (models/ac_models_hetero.py:22: one
    module-level SHARED_LAYER serves Fight1, Fight2, Esc1 and Esc2)"""
    for m in modules[1:]:
        m.shared_layer = modules[0].shared_layer
    return modules


# ------------------------------------------------------------------------------------------------------------------ the network
class _GRUWeights(nn.Module):
    """the four tensors of an nn.GRU(200, 200) layer under nn.GRU's names and its initialisation (uniform in +- 1 / sqrt(200))"""

    def __init__(self, n_in=GRU_H, hidden=GRU_H):
        super().__init__()
        k = hidden ** -0.5
        u = lambda *shape: nn.Parameter(torch.empty(shape).uniform_(-k, k))
        self.weight_ih_l0, self.weight_hh_l0 = u(3 * hidden, n_in), u(3 * hidden, hidden)
        self.bias_ih_l0, self.bias_hh_l0 = u(3 * hidden), u(3 * hidden)


class CommanderTrainable(nn.Module):
    """models/ac_models_hier.py:CommanderGru in training form, written from commander.state_keys() and the restatement of its forward in
    tests/commander_ref.py; `state_dict()` has exactly commander.state_keys()' keys and shapes, in that order, so it goes straight into
    `CommanderNet.refresh_weights`.  ONE shared_layer object serves the actor and the value branch.

    forward(obs_own [S, L, 34], critic_row [S, L, 105], state_in [S, 2, 200], seq_len [S], fused_gru=True) -> (logits [S, L, 3], value [S, L]):
    S sequences of L steps of one agent each, sequence s holding seq_len[s] steps and then padding; state_in[:, 0] / [:, 1] are the states
    rnn_act / rnn_val start from.  critic_row is rollout.central_critic_rows_hl's layout [a_own, a_o1, a_o2 | obs_own | obs_o1 | obs_o2];
    v1..v3 see [obs_k | act_k], v4 all three.  The GRU outputs are 0 at padded steps, whose logits and values mean nothing.
    fused_gru=True runs both GRUs through gru_sequence_pair (CUDA, float32, seq_len int32); False steps the same cell with torch ops on
    any device and dtype.  return_states=True appends (h_act, h_val) [S, 200] each: the states after each sequence's last step.
    inputs = "fused" (float32 on the GPU) runs inp1..inp4 and v1..v4 as one input_stage each (commander_stage_tables()) that read obs_own and
    critic_row as they are; the default "torch" slices, concatenates and runs the eight layers one by one.  state_dict() is the same.
    trunk = "fused" (float32 on the GPU) runs shared_layer, its bias and tanh over the actor's and the critic's rows as ONE dense_tanh; the
    default "torch" applies the layer twice.  state_dict() is the same; independent of `inputs`.
    heads = "fused" (trunk="torch"): TrainableNet's argument — `pre_heads(obs_own, critic_row, state_in, seq_len, fused_gru=True) -> (za, zc)`
    [S, L, 500] is the forward up to shared_layer's pre-activations, for heads_loss(n_comp=1); `forward` and state_dict() are unchanged."""

    def __init__(self, inputs="torch", trunk="torch", heads="torch"):
        super().__init__()
        self.trunk = _trunk_mode(trunk)
        self.heads = _heads_mode(heads, self.trunk)
        if inputs not in INPUT_MODES:
            raise ValueError(f"inputs is one of {INPUT_MODES}, got {inputs!r}")
        self.inputs = inputs
        self.shared_layer = _FC(500, 500)
        self.rnn_act, self.rnn_val = _GRUWeights(), _GRUWeights()
        self.inp1, self.inp2, self.inp3, self.inp4 = _FC(4, 50), _FC(20, 200), _FC(10, 50), _FC(34, 200)
        self.act_out = _FC(500, 3)
        self.v1, self.v2, self.v3, self.v4 = _FC(35, 100), _FC(35, 100), _FC(35, 100), _FC(105, 200)
        self.val_out = _FC(500, 1)

    def _front(self, obs_own, critic_row, state_in, seq_len, fused_gru):
        """-> (the actor's rows, the critic's rows as shared_layer sees them, y_a, y_v: the GRUs' outputs)"""
        if self.inputs == "fused":
            tables = commander_stage_tables()
            x, x_full = input_stage(obs_own.contiguous(), *stage_groups(self, COMMANDER_STAGE_LAYERS["actor"], tables["actor"]))
            z, z_full = input_stage(critic_row.contiguous(), *stage_groups(self, COMMANDER_STAGE_LAYERS["critic"], tables["critic"]))
        else:
            x = torch.cat((torch.tanh(self.inp1(obs_own[..., :4])), torch.tanh(self.inp2(obs_own[..., 4:24])),
                           torch.tanh(self.inp3(obs_own[..., 24:]))), dim=-1)
            x_full = torch.tanh(self.inp4(obs_own))
            a = critic_row[..., :3]
            o = [critic_row[..., 3 + 34 * k:3 + 34 * (k + 1)] for k in range(3)]
            v = [torch.cat((o[k], a[..., k:k + 1]), dim=-1) for k in range(3)]
            z = torch.cat([torch.tanh(m(vk)) for m, vk in zip((self.v1, self.v2, self.v3), v)], dim=-1)
            z_full = torch.tanh(self.v4(torch.cat(v, dim=-1)))
        ra, rv = self.rnn_act, self.rnn_val
        gi_a = x_full @ ra.weight_ih_l0.T + ra.bias_ih_l0
        gi_v = z_full @ rv.weight_ih_l0.T + rv.bias_ih_l0
        act = (gi_a, state_in[:, 0], ra.weight_hh_l0, ra.bias_hh_l0)
        val = (gi_v, state_in[:, 1], rv.weight_hh_l0, rv.bias_hh_l0)
        if fused_gru:
            y_a, y_v = gru_sequence_pair(act, val, seq_len)
        else:
            y_a, y_v = gru_sequence_torch(*act, seq_len), gru_sequence_torch(*val, seq_len)
        x_full = F.normalize(x_full + y_a, dim=-1)
        z_full = F.normalize(z_full + y_v, dim=-1)
        return torch.cat((x, x_full), dim=-1), torch.cat((z, z_full), dim=-1), y_a, y_v

    def pre_heads(self, obs_own, critic_row, state_in, seq_len, fused_gru=True):
        """forward up to shared_layer's pre-activations -> (za, zc) [S, L, 500]: what heads_loss(n_comp=1) takes.  trunk="torch" only."""
        if self.trunk == "fused":
            raise ValueError('pre_heads needs trunk="torch": dense_tanh has the tanh inside')
        xa, xc, _, _ = self._front(obs_own, critic_row, state_in, seq_len, fused_gru)
        return self.shared_layer(xa), self.shared_layer(xc)

    def forward(self, obs_own, critic_row, state_in, seq_len, fused_gru=True, return_states=False):
        xa, xc, y_a, y_v = self._front(obs_own, critic_row, state_in, seq_len, fused_gru)
        if self.trunk == "fused":
            lin = self.shared_layer._model[0]
            h, y = dense_tanh((xa, xc), lin.weight, lin.bias)
            logits, value = self.act_out(h), self.val_out(y).squeeze(-1)
        else:
            logits = self.act_out(torch.tanh(self.shared_layer(xa)))
            value = self.val_out(torch.tanh(self.shared_layer(xc))).squeeze(-1)
        if not return_states:
            return logits, value
        last = (seq_len.long() - 1).clamp(min=0)[:, None, None].expand(-1, 1, GRU_H)
        return logits, value, y_a.gather(1, last)[:, 0], y_v.gather(1, last)[:, 0]

    load_numpy = TrainableNet.load_numpy
