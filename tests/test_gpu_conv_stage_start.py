"""The start of the conv stage (convstage.h, phase -1) in sbk_conv_ffn_chain and
sbk_conv_ffn_tail: o is staged first across the workgroup, wo arrives K-step by
K-step under the out_proj MFMAs, x is waited for only at the residual add.

The shapes are the staged-row edges, not the workload: one partial tile with
every halo row clamped (T = 1, 5, 33), the halo crossing the 48-frame tile
edge and a one-row last tile (T = 47, 48, 49), a middle tile with a live halo
on both sides (T = 97), an exact multiple of the tile (T = 96); kernel size 31
non-causal (15 rows of left halo) and causal (30), and kernel size 3; the
out_proj bias and the key-padding mask given and null; d_eff = 144.

Every case is checked against the two launches the fused one replaces
(sbk_conv_module_pre, which this start does not touch, then sbk_ffn_chain /
sbk_ffn) at the project's 2e-2 for a fused launch against its parts
(test_gpu_conv_chain.py).  Isolation and determinism are bit-exact."""
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu

D, H = 256, 512
TS = [1, 5, 33, 47, 48, 49, 96, 97]
CONVS = [(31, False), (31, True), (3, False)]  # (kernel size, causal)


class _Case:
    """Inputs and modules of one (B, T, K, causal) case; bias: bo given;
    masked: a ragged key-padding mask; deff < 256: channels deff.. zero-padded
    (x, o, weights, LayerNorm gains and biases)."""

    def __init__(self, dev, B, T, K, causal, bias=True, masked=True, deff=None):
        from speechbrain_amd import _enc
        from speechbrain_amd.lobes.models.transformer.Conformer import ConvolutionModule
        from speechbrain_amd.nnet.activations import Swish
        from speechbrain_amd.nnet.attention import PositionalwiseFeedForward
        torch.manual_seed(1000 * K + 10 * T + B + int(causal))
        self.B, self.T, self.deff = B, T, deff
        ch = (torch.arange(D) < (deff or D)).float().to(dev)
        self.cm = ConvolutionModule(D, K, causal=causal).to(dev).eval()
        self.fa = PositionalwiseFeedForward(H, input_size=D, activation=Swish).to(dev).eval()
        self.fb = PositionalwiseFeedForward(H, input_size=D, activation=Swish).to(dev).eval()
        with torch.no_grad():
            cm = self.cm
            for p in cm.parameters():
                p.add_(0.05 * torch.randn_like(p))
            for ln in (cm.layer_norm, cm.after_conv[0]):
                ln.weight.mul_(ch)
                ln.bias.mul_(ch)
            pw = cm.bottleneck[0]
            pw.weight.mul_(torch.cat([ch, ch])[:, None, None] * ch[None, :, None])
            pw.bias.mul_(torch.cat([ch, ch]))
            cm.conv.weight.mul_(ch[:, None, None])
            cm.conv.bias.mul_(ch)
            lin = cm.after_conv[2]
            lin.weight.mul_(ch[:, None] * ch[None, :])
            lin.bias.mul_(ch)
            for f in (self.fa, self.fb):
                f.ffn[0].weight.mul_(ch[None, :])
                f.ffn[3].weight.mul_(ch[:, None])
                f.ffn[3].bias.mul_(ch)
        if deff:
            self.cm._deff = self.fa._deff = self.fb._deff = deff
        self.x = ((torch.randn(B * T, D) * 2 + 0.3).to(dev) * ch).contiguous()
        self.o = (torch.randn(B * T, D, device=dev) * ch).to(torch.bfloat16)
        self.wo = _enc.cast_bf16(torch.randn(D, D, device=dev) / 16 * ch[:, None] * ch[None, :])
        self.bo = torch.randn(D, device=dev) * 0.1 * ch if bias else None
        self.kpm = None
        if masked:
            lens = torch.randint(1, T + 1, (B,))
            lens[0] = T
            self.kpm = (torch.arange(T)[None] >= lens[:, None]).to(torch.uint8).reshape(-1).to(dev)
        self.lns = [((torch.randn(D, device=dev) * 0.5 + 1) * ch, torch.randn(D, device=dev) * 0.1 * ch, 1e-5)
                    for _ in range(4)]
        self.wp = _enc.cast_bf16((torch.randn(768, D) / 16).to(dev) * ch[None, :])

    def blocks(self):
        return (self.fa.chain_block(self.lns[0], 0.5, post_ln=self.lns[1]), self.fb.chain_block(self.lns[2], 0.5))

    def rows(self, b):
        """(x, o, kpm) of utterance b alone, in buffers of their own."""
        T = self.T
        sl = slice(b * T, (b + 1) * T)
        return self.x[sl].clone(), self.o[sl].clone(), None if self.kpm is None else self.kpm[sl].clone()

    def fused(self, x=None, o=None, kpm=None, B=None):
        from speechbrain_amd import _enc
        a, b = self.blocks()
        if x is None:
            x, o, kpm, B = self.x, self.o, self.kpm, self.B
        return _enc.conv_ffn_chain(x, B, self.T, (o, self.wo, self.bo), self.cm.fused_params(), kpm, a, b, "swish", 0.0,
                                   self.lns[3], self.wp, deff=self.deff)

    def two_launches(self):
        from speechbrain_amd import _enc
        a, b = self.blocks()
        mid = self.cm.run_fused(self.x, self.B, self.T, self.kpm, pre=(self.o, self.wo, self.bo))
        return _enc.ffn_chain(mid, a, b, "swish", 0.0, self.lns[3], self.wp, deff=self.deff)

    def tail(self, x=None, o=None, kpm=None, B=None):
        from speechbrain_amd import _enc
        a, _ = self.blocks()
        if x is None:
            x, o, kpm, B = self.x, self.o, self.kpm, self.B
        return _enc.conv_ffn_tail(x, B, self.T, (o, self.wo, self.bo), self.cm.fused_params(), kpm, a, self.lns[3],
                                  "swish", 0.0, deff=self.deff)

    def tail_two_launches(self):
        from speechbrain_amd import _enc
        ln0, w1, b1, w2, b2, alpha, post_ln = self.blocks()[0]
        mid = self.cm.run_fused(self.x, self.B, self.T, self.kpm, pre=(self.o, self.wo, self.bo))
        _, u = _enc.ffn(mid, ln0, w1, b1, "swish", 0.0, w2, b2, alpha, post_ln=post_ln, next_ln=self.lns[3],
                        next_dtype=torch.float32, deff=self.deff)
        return u


def _check(c):
    with torch.no_grad():
        out, y = c.fused()
        ref, yref = c.two_launches()
        u = c.tail()
        uref = c.tail_two_launches()
    assert_close(out, ref, rtol=2e-2, name="conv chain out")
    assert_close(y.float(), yref.float(), rtol=2e-2, name="conv chain projection")
    assert_close(u, uref, rtol=2e-2, name="conv tail u")
    return out, u


@pytest.mark.parametrize("K,causal", CONVS)
@pytest.mark.parametrize("T", TS)
def test_staged_row_edges(dev, T, K, causal):
    """Two utterances, bo given, ragged mask: chain and tail against the two launches."""
    _check(_Case(dev, 2, T, K, causal))


@pytest.mark.parametrize("bias,masked", [(False, False), (False, True), (True, False)])
@pytest.mark.parametrize("K,causal", CONVS)
@pytest.mark.parametrize("T", [5, 49, 97])
def test_null_bias_and_mask(dev, T, K, causal, bias, masked):
    """bo null reads another vector in its place and must add nothing; kpm
    null masks nothing."""
    _check(_Case(dev, 2, T, K, causal, bias=bias, masked=masked))


@pytest.mark.parametrize("K,causal", CONVS)
@pytest.mark.parametrize("T", [33, 49, 97])
def test_padded_channels(dev, T, K, causal):
    """d_eff = 144: LayerNorm statistics over the first 144 channels, the
    zero-padded channels come out exactly zero."""
    out, u = _check(_Case(dev, 2, T, K, causal, deff=144))
    assert float(out[:, 144:].abs().max()) == 0.0 and float(u[:, 144:].abs().max()) == 0.0


@pytest.mark.parametrize("nan_utts", [(1, 2), (0,)])
@pytest.mark.parametrize("K,causal", CONVS)
@pytest.mark.parametrize("T", [33, 49, 97])
def test_utterances_are_isolated(dev, T, K, causal, nan_utts):
    """B = 3 with the utterances of `nan_utts` all-NaN in x and o: the rows of
    the others are finite and equal the B = 1 run of that utterance bit for
    bit (a clamped or re-ordered load that reached a neighbour would show)."""
    c = _Case(dev, 3, T, K, causal)
    alone = {b: c.rows(b) for b in range(3) if b not in nan_utts}
    for b in nan_utts:
        c.x[b * T:(b + 1) * T] = float("nan")
        c.o[b * T:(b + 1) * T] = float("nan")
    with torch.no_grad():
        out, y = c.fused()
        u = c.tail()
        for b, (xb, ob, kb) in alone.items():
            sl = slice(b * T, (b + 1) * T)
            out1, y1 = c.fused(xb, ob, kb, 1)
            u1 = c.tail(xb, ob, kb, 1)
            assert bool(torch.isfinite(out[sl]).all()) and bool(torch.isfinite(y[sl].float()).all())
            assert bool(torch.isfinite(u[sl]).all())
            assert torch.equal(out[sl], out1), f"chain out of utterance {b}"
            assert torch.equal(y[sl], y1), f"chain projection of utterance {b}"
            assert torch.equal(u[sl], u1), f"tail u of utterance {b}"


def test_head_rows_are_isolated(dev):
    """sbk_src_ffn_proj tiles the flat rows (a tile spans two utterances):
    all-NaN rows next to utterance 0 leave its out and y rows finite and equal
    to the run on its rows alone."""
    from speechbrain_amd import _enc
    from speechbrain_amd.nnet.activations import Swish
    from speechbrain_amd.nnet.attention import PositionalwiseFeedForward
    torch.manual_seed(7)
    B, T, Kin = 3, 37, 64
    a = torch.randn(B * T, Kin, device=dev).to(torch.bfloat16)
    a[T:] = float("nan")
    ws = _enc.cast_bf16(torch.randn(D, Kin, device=dev) / Kin ** 0.5)
    bs = torch.randn(D, device=dev) * 0.3
    f = PositionalwiseFeedForward(H, input_size=D, activation=Swish).to(dev).eval()
    lns = [(torch.randn(D, device=dev) * 0.5 + 1, torch.randn(D, device=dev) * 0.1, 1e-5) for _ in range(2)]
    wp = _enc.cast_bf16((torch.randn(768, D) / 16).to(dev))
    with torch.no_grad():
        out, y, _ = f.run_fused_src_proj(a, ws, bs, lns[0], 0.5, lns[1], wp)
        out1, y1, _ = f.run_fused_src_proj(a[:T].clone(), ws, bs, lns[0], 0.5, lns[1], wp)
    assert bool(torch.isfinite(out[:T]).all()) and bool(torch.isfinite(y[:T].float()).all())
    assert torch.equal(out[:T], out1) and torch.equal(y[:T], y1)


@pytest.mark.parametrize("K,causal", CONVS)
def test_deterministic_and_graph_replay(dev, K, causal):
    """Two calls, and one call inside a captured graph replayed twice, give
    the same bits (the order of the loads is not the order of the sums)."""
    c = _Case(dev, 2, 97, K, causal)
    with torch.no_grad():
        out, y = c.fused()  # weight images built outside the capture
        u = c.tail()
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
