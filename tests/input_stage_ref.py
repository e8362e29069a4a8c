"""Case tables, inputs and float64 references for the input-stage tests (test_input_stage_host.py, test_gpu_input_stage.py): the ten
stages of the five trainable networks (four kinds and the commander, actor and critic side each) as learner.stage_tables /
commander_stage_tables describe them, with the layer shapes of the modules themselves.  The reference is CPU autograd of
learner.input_stage_torch in float64.  References are computed once per case and shared: callers must not write into what they get."""
import functools

import torch

from hhmarl_2d_amd import learner as LR
from hhmarl_2d_amd import policy_nets as PN

NETS = ("Fight1", "Fight2", "Esc1", "Esc2", "commander")
CASES = tuple((net, side) for net in NETS for side in ("actor", "critic"))
KIND = {v: k for k, v in PN.KIND_NAMES.items()}
ROWS = (1, 63, 65, 1300)        # one row; one short of two tiles of 32 + a ragged tail; two tiles + one row; 41 tiles: every lane mix of the walk
WRAP_ROWS = 71200               # 2225 tiles: more than the forward's grid and than the backward's partial-sum cap


@functools.lru_cache(maxsize=None)
def module(net):
    return LR.CommanderTrainable() if net == "commander" else LR.TrainableNet(KIND[net])


@functools.lru_cache(maxsize=None)
def case(net, side):
    """-> dict: width (of a source row), layers (module names), shapes ((n_out, K) per layer), segments, packs"""
    if net == "commander":
        tables, layers, width = LR.commander_stage_tables(), LR.COMMANDER_STAGE_LAYERS, {"actor": 34, "critic": 105}[side]
    else:
        kind = KIND[net]
        tables, layers = LR.stage_tables(kind), LR.stage_layers(kind)
        width = PN.OBS_DIM[kind] if side == "actor" else sum(PN.CRITIC_DIMS[kind])
    segments, packs = tables[side]
    shapes = tuple(tuple(getattr(module(net), nm)._model[0].weight.shape) for nm in layers[side])
    return dict(width=width, layers=layers[side], shapes=shapes, segments=segments, packs=packs)


@functools.lru_cache(maxsize=None)
def inputs(net, side, R, seed=0, src_ld=None):
    """src [R, src_ld or width] in [0, 1), per layer w = randn / sqrt(K) and b = 0.1 randn, per pack d_y = randn"""
    c = case(net, side)
    g = torch.Generator().manual_seed(1000 * seed + 31 * CASES.index((net, side)) + R)
    src = torch.rand((R, src_ld or c["width"]), generator=g)
    ws = tuple(torch.randn(shp, generator=g) / shp[1] ** 0.5 for shp in c["shapes"])
    bs = tuple(0.1 * torch.randn((shp[0],), generator=g) for shp in c["shapes"])
    d_packs = tuple(torch.randn((R, sum(c["shapes"][i][0] for i in p)), generator=g) for p in c["packs"])
    return src, ws, bs, d_packs


def run(net, side, inp, dtype, device, fn=None):
    """fn (default: the torch-op restatement) and its autograd in `dtype` on `device` -> (y, d_w, d_b), each a list with one float64 CPU
    tensor per layer (y: the layer's columns of its pack)"""
    c = case(net, side)
    src, ws, bs, d_packs = inp
    ws = [w.to(device=device, dtype=dtype).requires_grad_(True) for w in ws]
    bs = [b.to(device=device, dtype=dtype).requires_grad_(True) for b in bs]
    outs = (fn or LR.input_stage_torch)(src.to(device=device, dtype=dtype), list(zip(ws, bs, c["segments"])), c["packs"])
    torch.autograd.backward(outs, [d.to(device=device, dtype=dtype) for d in d_packs])
    ys = [None] * len(ws)
    for p, out in zip(c["packs"], outs):
        col = 0
        for i in p:
            ys[i] = out.detach()[..., col:col + c["shapes"][i][0]].double().cpu()
            col += c["shapes"][i][0]
    return ys, [w.grad.double().cpu() for w in ws], [b.grad.double().cpu() for b in bs]


@functools.lru_cache(maxsize=None)
def reference(net, side, R, seed=0):
    return run(net, side, inputs(net, side, R, seed), torch.float64, "cpu")


def rel_err(got, want):
    """max |difference| / max |reference| of one compared tensor"""
    return (got - want).abs().max().item() / want.abs().max().item()
