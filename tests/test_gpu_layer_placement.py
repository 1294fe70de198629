"""The XCD-contiguous tile order of the conv-stage launches (sbk_conv_ffn_chain,
sbk_conv_ffn_tail: tile = sbk::xcd_tile(gridDim.x, blockIdx.x)).  The other
conv-chain tests launch fewer than 8 workgroups, for which the order is the
identity; the cases here launch 8 .. 24: multiples of 8, nwg % 8 != 0 with
tiles on both sides of the order's branch, one tile and 8 tiles per utterance,
and a last tile with one live row (T = 97, 5 * 97, 3 * 376 and 2 * 376 rows
are no multiple of the 48-frame tile).  D = 256, H = 512, kernel size 31, a
ragged key-padding mask, the out_proj bias given.

A fused launch is checked against the two launches it replaces at the
project's 2e-2 (test_gpu_conv_chain.py); ownership (every tile written by
exactly one workgroup, nothing past B * T) by sentinels; determinism bit for
bit.  The out_proj weight cases: a new wo tensor is followed (nothing derived
from wo may be served stale), and with wo confined to 144 x 144 the channels
144.. come out exactly zero."""
import pytest
import torch

from conftest import assert_close
from test_gpu_conv_chain import D, _Case as _ChainCase

H = 512
# (B, T): nwg = B * ceil(T / 48) = 8, 9, 15, 16, 17, 24
CASES = [(8, 40), (3, 100), (5, 97), (2, 376), (17, 5), (3, 376)]
SENTINEL, PAD = 776.0, 64  # exact in bf16


class _Case(_ChainCase):
    """test_gpu_conv_chain's case (K = 31, masked) with the tail launch beside the chain."""

    def __init__(self, dev, B, T, deff=None):
        super().__init__(dev, B, T, 31, False, True, H, deff=deff)

    def tail(self):
        from speechbrain_amd import _enc
        a, _ = self.blocks()
        return _enc.conv_ffn_tail(self.x, self.B, self.T, (self.o, self.wo, self.bo), self.cm.fused_params(), self.kpm,
                                  a, self.lns[3], "swish", 0.0, deff=self.deff)

    def tail_two_launches(self):
        from speechbrain_amd import _enc
        ln0, w1, b1, w2, b2, alpha, post_ln = self.blocks()[0]
        mid = self.cm.run_fused(self.x, self.B, self.T, self.kpm, pre=(self.o, self.wo, self.bo))
        _, u = _enc.ffn(mid, ln0, w1, b1, "swish", 0.0, w2, b2, alpha, post_ln=post_ln, next_ln=self.lns[3],
                        next_dtype=torch.float32, deff=self.deff)
        return u

    def into_sentinels(self):
        """Chain and tail into buffers of B * T + PAD rows filled with the sentinel."""
        from speechbrain_amd import _enc
        a, b = self.blocks()
        M = self.B * self.T
        dev = self.x.device
        out = torch.full((M + PAD, D), SENTINEL, device=dev)
        y = torch.full((M + PAD, 768), SENTINEL, device=dev, dtype=torch.bfloat16)
        u = torch.full((M + PAD, D), SENTINEL, device=dev)
        ln0, w1p, b1p, wc, bc, causal, ln1, w2, b2 = self.cm.fused_params()
        gp, bp, ep = a[6]
        act = _enc.ACT["swish"]
        _enc._conv_ffn_chain_into(out, y, self.x, self.B, self.T, self.o, self.wo, self.bo, ln0[0], ln0[1], ln0[2], w1p,
                                  b1p, wc, bc, causal, ln1[0], ln1[1], ln1[2], w2, b2, self.kpm, act, 0.0, a[0][0],
                                  a[0][1], a[0][2], a[1], a[2], a[3], a[4], a[5], gp, bp, ep, b[0][0], b[0][1], b[0][2],
                                  b[1], b[2], b[3], b[4], b[5], self.lns[3][0], self.lns[3][1], self.lns[3][2], self.wp, D)
        _enc._conv_ffn_tail_into(u, self.x, self.B, self.T, self.o, self.wo, self.bo, ln0[0], ln0[1], ln0[2], w1p, b1p,
                                 wc, bc, causal, ln1[0], ln1[1], ln1[2], w2, b2, self.kpm, act, 0.0, a[0][0], a[0][1],
                                 a[0][2], a[1], a[2], a[3], a[4], a[5], gp, bp, ep, self.lns[3][0], self.lns[3][1],
                                 self.lns[3][2], D)
        return out, y, u


_RUNS = {}


def _run(dev, B, T):
    """One case's inputs, fused results and two-launch references, computed once per module run."""
    if (B, T) not in _RUNS:
        c = _Case(dev, B, T)
        with torch.no_grad():
            _RUNS[(B, T)] = (c, c.fused(), c.tail(), c.two_launches(), c.tail_two_launches())
    return _RUNS[(B, T)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", CASES)
def test_fused_vs_two_launches(dev, B, T):
    _, (out, y), u, (ref, yref), uref = _run(dev, B, T)
    assert_close(out, ref, rtol=2e-2, name="conv chain out")
    assert_close(y.float(), yref.float(), rtol=2e-2, name="conv chain projection")
    assert_close(u, uref, rtol=2e-2, name="conv tail u")


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", CASES)
def test_every_tile_owned_once(dev, B, T):
    """Rows below B * T are all written (and hold the same bits as the plain
    call: a tile written by two workgroups would hold them too, one skipped
    keeps the sentinel), rows at or beyond B * T keep the sentinel."""
    c, (out0, y0), u0, _, _ = _run(dev, B, T)
    M = B * T
    with torch.no_grad():
        out, y, u = c.into_sentinels()
    for name, t, t0 in (("out", out, out0), ("y", y, y0), ("u", u, u0)):
        rows_kept = (t[:M].float() == SENTINEL).all(dim=1)
        assert not bool(rows_kept.any()), f"{name}: rows {rows_kept.nonzero().flatten().tolist()[:8]} never written"
        assert bool((t[M:].float() == SENTINEL).all()), f"{name}: rows at or beyond B * T written"
        assert torch.equal(t[:M], t0), f"{name}: differs from the plain call"


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(3, 100), (2, 376)])
def test_deterministic_and_graph_replay(dev, B, T):
    c, (out, y), u, _, _ = _run(dev, B, T)
    with torch.no_grad():
        out2, y2 = c.fused()
        u2 = c.tail()
        assert torch.equal(out, out2) and torch.equal(y, y2) and torch.equal(u, u2)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gout, gy = c.fused()
            gu = c.tail()
        for _ in range(2):
            gout.fill_(-1.0)
            gy.fill_(-1.0)
            gu.fill_(-1.0)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(gout, out) and torch.equal(gy, y) and torch.equal(gu, u)


@pytest.mark.gpu
def test_new_out_proj_weight_is_followed(dev):
    """A second run with other wo values in a new tensor follows the new weight."""
    from speechbrain_amd import _enc
    c = _Case(dev, 3, 100)
    with torch.no_grad():
        out_a, _ = c.fused()
        u_a = c.tail()
        c.wo = _enc.cast_bf16(torch.randn(D, D, device=dev) / 8)
        out_b, y_b = c.fused()
        u_b = c.tail()
        ref, yref = c.two_launches()
        uref = c.tail_two_launches()
    assert not torch.equal(out_a, out_b) and not torch.equal(u_a, u_b)
    assert_close(out_b, ref, rtol=2e-2, name="conv chain out, new wo")
    assert_close(y_b.float(), yref.float(), rtol=2e-2, name="conv chain projection, new wo")
    assert_close(u_b, uref, rtol=2e-2, name="conv tail u, new wo")


@pytest.mark.gpu
def test_out_proj_channel_slice(dev):
    """d_eff = 144: wo is non-zero only in its first 144 rows and columns (as
    every other weight); channels 144.. of the outputs are exactly zero."""
    c = _Case(dev, 3, 100, deff=144)
    assert float(c.wo[144:].float().abs().max()) == 0.0 and float(c.wo[:, 144:].float().abs().max()) == 0.0
    assert float(c.wo[:144, :144].float().abs().max()) > 0.0
    with torch.no_grad():
        out, y = c.fused()
        u = c.tail()
        ref, yref = c.two_launches()
        uref = c.tail_two_launches()
    assert_close(out, ref, rtol=2e-2, name="padded out")
    assert_close(y.float(), yref.float(), rtol=2e-2, name="padded projection")
    assert_close(u, uref, rtol=2e-2, name="padded tail u")
    assert float(out[:, 144:].abs().max()) == 0.0 and float(u[:, 144:].abs().max()) == 0.0


@pytest.fixture(scope="module")
def hostlib():
    import os
    from speechbrain_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from speechbrain_amd import _build
        _build.build()
    return _lib.lib()


def test_xcd_tile_is_a_contiguous_bijection(hostlib):
    """sbk_xcd_tile, nwg = 1 .. 600: orig -> tile is a permutation; the blocks
    of one residue orig % 8 own one contiguous run of tiles, in launch order;
    the runs of residues 0 .. 7 ascend and their sizes differ by at most one."""
    for nwg in range(1, 601):
        tiles = [hostlib.sbk_xcd_tile(nwg, i) for i in range(nwg)]
        assert sorted(tiles) == list(range(nwg)), nwg
        end = 0
        for r in range(8):
            run = tiles[r::8]
            assert run == list(range(end, end + len(run))), (nwg, r)
            assert len(run) in (nwg // 8, nwg // 8 + 1), (nwg, r)
            end += len(run)
        assert end == nwg
    assert hostlib.sbk_xcd_tile(8, 8) == -1 and hostlib.sbk_xcd_tile(8, -1) == -1 and hostlib.sbk_xcd_tile(0, 0) == -1
