"""The narrow-tile instances of hh_k_gru_seq_fwd / hh_k_gru_seq_bwd on the MI355X: every compiled tile (HH_GRU_TILE) writes the bytes
tile 16 writes, sequences of length 0 give exact zeros and disturb nothing, and hh_gru_seq_tile reports the tile a call uses.  A
sequence's arithmetic is its own fmaf chain in k order whatever sequences share its workgroup, so the comparison is of bytes."""
import pytest
import torch

pytestmark = pytest.mark.gpu
NAMES = ("y", "d_gi", "d_gh", "d_h0")
HH_E_ARG = -1                 # include/hh_abi.h
RULE = {13: 4, 854: 4, 1708: 4, 1709: 8, 3416: 8, 3417: 16}     # the tile chosen without HH_GRU_TILE


def _inputs(G, S, Lm, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *shape, s=1.0: (s * torch.randn(shape, generator=g)).cuda()
    parts = [(mk(S, Lm, 600), mk(S, 200, s=0.5), mk(600, 200, s=200 ** -0.5), mk(600, s=0.1)) for _ in range(G)]
    dys = [mk(S, Lm, 200) for _ in range(G)]
    return parts, dys


def _ragged(S, Lm, seed):
    """lengths in 1 .. L holding L (sequence 0) and, from two sequences on, 1 (sequence 1)"""
    n = torch.randint(1, Lm + 1, (S,), generator=torch.Generator().manual_seed(seed))
    n[0] = Lm
    if S > 1:
        n[1] = 1
    return n.to(torch.int32).cuda()


def _run(parts, dys, seq_len):
    """forward and backward of all GRUs -> per GRU {y, d_gi, d_gh, d_h0}"""
    from hhmarl_2d_amd import learner as LR
    ys, scratch = LR.gru_seq_forward(parts, seq_len)
    out = LR.gru_seq_backward(parts, ys, dys, seq_len, scratch)
    torch.cuda.synchronize()
    return [dict(zip(NAMES, (y,) + tuple(o))) for y, o in zip(ys, out)]


def _same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_the_library_has_the_narrow_instances():
    from hhmarl_2d_amd import _lib as L
    assert L.GRU_TILES[0] == 16 and len(L.GRU_TILES) >= 2 and set(L.GRU_TILES) <= {16, 8, 4}
    assert L.lib().hh_gru_seq_tile(13) in L.GRU_TILES


@pytest.mark.parametrize("G", (1, 2))
@pytest.mark.parametrize("Lm", (1, 20, 32))
def test_every_tile_writes_tile_16s_bytes(G, Lm, monkeypatch):
    """S = 1, 3, 4, 5, 16, 17, 33: under every tile width a last tile of one sequence, and a full tile in front of a ragged one"""
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    for S in (1, 3, 4, 5, 16, 17, 33):
        parts, dys = _inputs(G, S, Lm, 1000 * Lm + 10 * S + G)
        seq_len = _ragged(S, Lm, S + Lm)
        lens = seq_len.tolist()
        assert Lm in lens and (S == 1 or 1 in lens)
        monkeypatch.setenv("HH_GRU_TILE", "16")
        assert LR.gru_seq_tile(S) == 16
        want = _run(parts, dys, seq_len)
        assert all(torch.isfinite(v).all() for w in want for v in w.values()) and all(w["y"][0].abs().sum() > 0 for w in want)
        for tile in L.GRU_TILES[1:]:
            monkeypatch.setenv("HH_GRU_TILE", str(tile))
            assert LR.gru_seq_tile(S) == tile
            got = _run(parts, dys, seq_len)
            for g in range(G):
                for k in NAMES:
                    assert _same_bytes(got[g][k], want[g][k]), f"tile {tile}, G = {G}, S = {S}, L = {Lm}, GRU {g}: {k} differs from tile 16's"


def test_zero_length_sequences_give_zeros_and_disturb_nothing(monkeypatch):
    """S = 9 with four live sequences among zero-length ones (under tile 4 the last tile is all zero-length).  The zero-length sequences'
    gi, h0 and dy hold NaN: the contract says they are not read.  The live sequences' bytes equal a run of those sequences alone."""
    from hhmarl_2d_amd import _lib as L
    lens = [3, 0, 20, 0, 0, 1, 0, 0, 0]
    S, Lm, G = len(lens), 20, 2
    seq_len = torch.tensor(lens, dtype=torch.int32).cuda()
    live = [s for s, n in enumerate(lens) if n > 0]
    dead = [s for s, n in enumerate(lens) if n == 0]
    parts, dys = _inputs(G, S, Lm, 77)
    for (gi, h0, _, _), dy in zip(parts, dys):
        gi[dead], h0[dead], dy[dead] = float("nan"), float("nan"), float("nan")
    alone_parts = [(gi[live].contiguous(), h0[live].contiguous(), w, b) for gi, h0, w, b in parts]
    alone_dys = [dy[live].contiguous() for dy in dys]
    for tile in L.GRU_TILES:
        monkeypatch.setenv("HH_GRU_TILE", str(tile))
        got = _run(parts, dys, seq_len)
        alone = _run(alone_parts, alone_dys, seq_len[live].contiguous())
        for g in range(G):
            for k in NAMES:
                z = got[g][k][dead]
                assert _same_bytes(z, torch.zeros_like(z)), f"tile {tile}, GRU {g}: {k} of a zero-length sequence is not exactly +0"
                assert _same_bytes(got[g][k][live], alone[g][k]), f"tile {tile}, GRU {g}: {k} of a live sequence differs from the run without zero-length sequences"
            assert torch.isfinite(got[g]["y"]).all() and got[g]["y"][live[0], 0].abs().sum() > 0


def test_the_tile_query(monkeypatch):
    from hhmarl_2d_amd import _lib as L
    from hhmarl_2d_amd import learner as LR
    lib = L.lib()
    for tile in L.GRU_TILES:
        monkeypatch.setenv("HH_GRU_TILE", str(tile))
        assert lib.hh_gru_seq_tile(13) == tile and lib.hh_gru_seq_tile(854) == tile
    for bad in ("5", "32", "0", "x"):
        monkeypatch.setenv("HH_GRU_TILE", bad)
        assert lib.hh_gru_seq_tile(13) == HH_E_ARG
        assert b"HH_GRU_TILE" in lib.hh_last_error()
        with pytest.raises(RuntimeError, match="HH_GRU_TILE"):
            LR.gru_seq_tile(13)
        parts, _ = _inputs(1, 2, 4, 3)
        with pytest.raises(RuntimeError, match="HH_GRU_TILE"):
            LR.gru_seq_forward(parts, torch.tensor([4, 1], dtype=torch.int32).cuda())
    monkeypatch.delenv("HH_GRU_TILE", raising=False)
    for S, tile in RULE.items():
        assert LR.gru_seq_tile(S) == tile, f"without HH_GRU_TILE, {S} sequences run tile {tile} (DESIGN.md section 19)"
    assert LR.gru_seq_tile(1) in L.GRU_TILES and LR.gru_seq_tile(1 << 24) == 16
