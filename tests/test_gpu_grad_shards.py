"""hh_grad_pack and hh_grad_combine on the MI355X against tests/grad_shards_ref.py, a numpy float64 restatement with the same order of
operations: every comparison is bit for bit.  Sizes around the float4 body, its scalar tail and the 4096-element tile, a 250000-element
tensor over many workgroups, a gradient that is only 4-byte aligned, an absent gradient, 65 tensors (two launches); 1, 2, 3 and 8 shards
with weights that include 0.0 and 1/3 and gradients that include -0.0, denormals and 1e-12."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_shards_ref as GR

pytestmark = pytest.mark.gpu
SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 250000)
ODD, ABSENT = 4, 2          # SIZES[ODD] (4095 elements) lies 4 bytes behind a 16-byte boundary; SIZES[ABSENT] has no gradient


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _values(rng, n):
    """float32 gradients of mixed scale with the values a sum must not lose: -0.0, +0.0, denormals, 1e-12, and large ones"""
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6.0, 2.0, n)).astype(np.float32)
    special = np.array([-0.0, 0.0, 1e-12, -1e-12, 1e-45, -1e-45, 3e-39, -7e-41, 1.17549435e-38, 3.0e38, -3.0e38], dtype=np.float32)
    k = min(n, 4 * len(special))
    x[rng.permutation(n)[:k]] = special[np.arange(k) % len(special)]
    return x


def _tensors(rng, sizes, odd=None, absent=None):
    """device tensors for `sizes` (the odd one a view 4 bytes into a 16-byte aligned block, the absent one None) and their host values"""
    host = [None if i == absent else _values(rng, n) for i, n in enumerate(sizes)]
    dev = []
    for i, h in enumerate(host):
        if h is None:
            dev.append(None)
        elif i == odd:
            block = torch.zeros((len(h) + 8,), dtype=torch.float32, device="cuda")
            assert block.data_ptr() % 16 == 0
            view = block[1:1 + len(h)]
            view.copy_(torch.from_numpy(h))
            assert view.data_ptr() % 16 == 4 and view.is_contiguous()
            dev.append(view)
        else:
            dev.append(torch.from_numpy(h).cuda())
            assert dev[-1].data_ptr() % 16 == 0
    return host, dev


@pytest.fixture(scope="module")
def shards():
    """eight shards' gradients of the SIZES tensors, packed once by the kernel and once by the reference: what the tests share (read only)"""
    from hhmarl_2d_amd import learner as LR
    rng = np.random.default_rng(2024)
    lay = LR.grad_layout(SIZES)
    assert lay == GR.layout(SIZES) and lay[2] % 4 == 0 and all(o % 4 == 0 for o in lay[1])
    host, got = [], torch.full((8, lay[2]), float("nan"), dtype=torch.float32, device="cuda")
    for r in range(8):
        h, d = _tensors(rng, SIZES, odd=ODD, absent=ABSENT if r == 0 else None)
        LR.grad_pack(d, got[r], lay)
        host.append(h)
    torch.cuda.synchronize()
    want = np.stack([GR.pack(h, lay) for h in host])
    return lay, host, got, want


def test_pack_is_the_reference_bucket_and_its_padding_is_plus_zero(shards):
    from hhmarl_2d_amd import learner as LR
    lay, host, got, want = shards
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), "every element of every bucket, NaN sentinels overwritten"
    ns, offs, E = lay
    b0 = _bits(got[0].cpu().numpy())
    for n, off, nxt in zip(ns, offs, offs[1:] + [E]):
        assert not b0[off + n:nxt].any(), "the padding behind a tensor is +0.0f"
    assert not b0[offs[ABSENT]:offs[ABSENT + 1]].any(), "an absent gradient is +0.0f"
    assert _bits(host[0][0])[0] == 0x80000000 and b0[offs[0]] == 0x80000000, "-0.0 travels as it is"
    # the torch twin writes the same bucket
    twin = LR.grad_pack_torch([None if h is None else torch.from_numpy(h) for h in host[0]], lay)
    assert np.array_equal(_bits(twin.numpy()), _bits(want[0]))


WEIGHTS = {1: [1.0], 2: [0.75, 0.25], 3: [1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0], 8: [0.0, 1.0 / 3.0, 0.125, 0.0, 1.0 / 7.0, 0.25, 1.0 / 3.0 - 0.125, 1.0 / 7.0 - 0.125]}


@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_combine_adds_the_shards_in_order(shards, W):
    from hhmarl_2d_amd import learner as LR
    lay, host, got, want = shards
    rng = np.random.default_rng(W)
    buckets = got[:W].contiguous()
    _, out = _tensors(rng, SIZES, odd=ODD)                    # the destinations hold other values before the call
    out[ABSENT] = None if W == 2 else out[ABSENT]              # a parameter that receives nothing is skipped
    LR.grad_combine(out, buckets, WEIGHTS[W], lay)
    torch.cuda.synchronize()
    ref = GR.combine(want[:W], WEIGHTS[W], lay)
    twin = LR.grad_combine_torch(torch.from_numpy(want[:W]), WEIGHTS[W], lay)
    for i, (o, r, t) in enumerate(zip(out, ref, twin)):
        if o is None:
            continue
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(r)), f"W {W}: tensor {i} of {SIZES[i]} elements"
        assert np.array_equal(_bits(t.numpy()), _bits(r)), f"W {W}: the torch twin, tensor {i}"
    if W == 1:          # one shard, weight 1.0: the input bytes, -0.0 and denormals included
        for i, o in enumerate(out):
            h = host[0][i] if host[0][i] is not None else np.zeros(SIZES[i], dtype=np.float32)
            assert np.array_equal(_bits(o.cpu().numpy()), _bits(h))
        flat = np.concatenate([h for h in host[0] if h is not None])
        assert (_bits(flat) == 0x80000000).any() and ((np.abs(flat) > 0) & (np.abs(flat) < 1.17549435e-38)).any()


def test_a_zero_weight_shard_leaves_the_other_shards_gradient():
    """the tail of a ragged update: weights (1.0, 0.0) and a zero bucket give shard 0's gradient (equal in value: -0.0 + 0.0 is +0.0)"""
    from hhmarl_2d_amd import learner as LR
    rng = np.random.default_rng(5)
    sizes = (4097, 5)
    lay = LR.grad_layout(sizes)
    host, dev = _tensors(rng, sizes)
    buckets = torch.zeros((2, lay[2]), dtype=torch.float32, device="cuda")
    LR.grad_pack(dev, buckets[0], lay)
    LR.grad_pack([None, None], buckets[1], lay)
    out = [torch.empty_like(d) for d in dev]
    LR.grad_combine(out, buckets, [1.0, 0.0], lay)
    torch.cuda.synchronize()
    for o, d in zip(out, dev):
        assert torch.equal(o, d)


def test_65_tensors_take_two_launches():
    from hhmarl_2d_amd import learner as LR
    rng = np.random.default_rng(65)
    sizes = [int(n) for n in rng.integers(1, 40, 65)]
    sizes[64] = 4099                                           # the second launch's only tensor, more than one tile
    lay = LR.grad_layout(sizes)
    host = [[_values(rng, n) for n in sizes] for _ in range(2)]
    buckets = torch.full((2, lay[2]), float("nan"), dtype=torch.float32, device="cuda")
    for r in range(2):
        LR.grad_pack([torch.from_numpy(h).cuda() for h in host[r]], buckets[r], lay)
    out = [torch.full((n,), float("nan"), dtype=torch.float32, device="cuda") for n in sizes]
    LR.grad_combine(out, buckets, [0.3, 0.7], lay)
    torch.cuda.synchronize()
    want = np.stack([GR.pack(h, lay) for h in host])
    assert np.array_equal(_bits(buckets.cpu().numpy()), _bits(want))
    for o, r in zip(out, GR.combine(want, [0.3, 0.7], lay)):
        assert np.array_equal(_bits(o.cpu().numpy()), _bits(r))


def test_refused_arguments_enqueue_nothing():
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    lib = L.lib()
    S = 7.5
    g = torch.full((16,), 2.0, dtype=torch.float32, device="cuda")
    bucket = torch.full((2, 24), S, dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda x: C.c_void_p(x.data_ptr())
    w = (C.c_double * 2)(0.5, 0.5)

    def desc(**kw):
        d = (L.HHGradTensor * 2)()
        d[0].g, d[0].n, d[0].off = g.data_ptr(), 5, 0
        d[1].g, d[1].n, d[1].off = g.data_ptr() + 32, 8, 8
        for k, val in kw.items():
            setattr(d[int(k[-1])], k[:-1], val)
        return d
    E = -1      # HH_E_ARG
    pack = lambda n=2, d=None, b=ptr(bucket), e=24: lib.hh_grad_pack(n, desc() if d is None else d, b, e, st)
    assert pack(n=0) == E and pack(n=-1) == E and lib.hh_grad_pack(2, None, ptr(bucket), 24, st) == E and pack(b=None) == E
    assert pack(b=C.c_void_p(bucket.data_ptr() + 4)) == E and pack(e=22) == E and pack(e=-4) == E and pack(e=12) == E
    assert pack(d=desc(off0=4)) == E and pack(d=desc(off1=6)) == E and pack(d=desc(off1=4)) == E and pack(d=desc(n1=20)) == E
    assert pack(d=desc(n0=-1)) == E and pack(d=desc(g1=g.data_ptr() + 2)) == E and pack(d=desc(off1=-4)) == E
    comb = lambda n=2, d=None, b=ptr(bucket), e=24, W=2, ww=w: lib.hh_grad_combine(n, desc() if d is None else d, b, e, W, ww, st)
    assert comb(n=-1) == E and lib.hh_grad_combine(2, None, ptr(bucket), 24, 2, w, st) == E and comb(b=None) == E and comb(ww=None) == E
    assert comb(W=0) == E and comb(W=65) == E and comb(b=C.c_void_p(bucket.data_ptr() + 8)) == E and comb(e=23) == E
    assert comb(d=desc(off1=6)) == E and comb(d=desc(n1=20)) == E and comb(d=desc(n0=-1)) == E and comb(d=desc(g0=g.data_ptr() + 1)) == E
    torch.cuda.synchronize()
    assert bool((bucket == S).all()) and bool((g == 2.0).all())
    # what succeeds without a launch: an empty list for combine, tensors without a gradient or elements
    assert lib.hh_grad_combine(0, None, ptr(bucket), 24, 2, w, st) == 0 and comb(d=desc(g0=None, n1=0)) == 0
    torch.cuda.synchronize()
    assert bool((bucket == S).all()) and bool((g == 2.0).all())
    # and the wrappers' own refusals
    lay = LR.grad_layout([5, 8])
    with pytest.raises(ValueError, match="bucket is a contiguous float32"):
        LR.grad_pack([g[:5], g[8:]], bucket[0, :20], lay)
    with pytest.raises(ValueError, match="one weight per shard"):
        LR.grad_combine([g[:5], g[8:]], torch.zeros((2, lay[2]), device="cuda"), [1.0], lay)
    with pytest.raises(ValueError, match="layout entry"):
        LR.grad_pack([g[:4], g[8:]], torch.zeros((lay[2],), device="cuda"), lay)
