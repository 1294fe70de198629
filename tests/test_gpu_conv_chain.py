"""sbk_conv_ffn_chain: the convolution module of layer i in front of the layer
chain (FFN2 + norm2 of layer i, FFN1 + norm1 + in_proj of layer i+1) in one
launch, against the two launches it replaces (sbk_conv_module_pre, then
sbk_ffn_chain).  The rounding points are the same and the summation order
differs, so the bound is the project's 2e-2 for fused-module tests
(test_conv_module_with_out_proj, test_ffn_chain_vs_two_launches)."""
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu

D = 256
# (B, T, K, causal, masked)
SHAPES = [(1, 5, 31, False, False),   # one tile, halo entirely outside the utterance
          (3, 37, 31, False, True),   # several utterances, halo crossing utterance ends
          (2, 50, 7, True, False),    # causal, two tiles, short kernel
          (2, 97, 31, False, True),   # three tiles, the last with one live row
          (2, 96, 31, False, True)]   # exact tile multiple


class _Case:
    """Inputs and modules of one (B, T, K, causal, masked, H) case; deff < 256:
    channels deff.. zero-padded (x, weights, LayerNorm gains and biases)."""

    def __init__(self, dev, B, T, K, causal, masked, H, deff=None):
        from speechbrain_amd import _enc
        from speechbrain_amd.lobes.models.transformer.Conformer import ConvolutionModule
        from speechbrain_amd.nnet.activations import Swish
        from speechbrain_amd.nnet.attention import PositionalwiseFeedForward
        torch.manual_seed(K + T + H)
        self.B, self.T, self.deff = B, T, deff
        ch = (torch.arange(D) < (deff or D)).float().to(dev)
        self.cm = ConvolutionModule(D, K, causal=causal).to(dev).eval()
        self.fa = PositionalwiseFeedForward(H, input_size=D, activation=Swish).to(dev).eval()
        self.fb = PositionalwiseFeedForward(H, input_size=D, activation=Swish).to(dev).eval()
        with torch.no_grad():
            for p in self.cm.parameters():
                p.add_(0.05 * torch.randn_like(p))
            cm = self.cm
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
        self.bo = torch.randn(D, device=dev) * 0.1 * ch
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

    def fused(self):
        from speechbrain_amd import _enc
        a, b = self.blocks()
        return _enc.conv_ffn_chain(self.x, self.B, self.T, (self.o, self.wo, self.bo), self.cm.fused_params(),
                                   self.kpm, a, b, "swish", 0.0, self.lns[3], self.wp, deff=self.deff)

    def two_launches(self):
        from speechbrain_amd import _enc
        a, b = self.blocks()
        mid = self.cm.run_fused(self.x, self.B, self.T, self.kpm, pre=(self.o, self.wo, self.bo))
        return _enc.ffn_chain(mid, a, b, "swish", 0.0, self.lns[3], self.wp, deff=self.deff)


@pytest.mark.parametrize("H", [512, 1024])
@pytest.mark.parametrize("B,T,K,causal,masked", SHAPES)
def test_fused_vs_two_launches(dev, B, T, K, causal, masked, H):
    c = _Case(dev, B, T, K, causal, masked, H)
    with torch.no_grad():
        out, y = c.fused()
        ref, yref = c.two_launches()
    assert out.data_ptr() != c.x.data_ptr()
    assert_close(out, ref, rtol=2e-2, name="conv chain out")
    assert_close(y.float(), yref.float(), rtol=2e-2, name="conv chain projection")


@pytest.mark.parametrize("B,T,K,causal,masked", [(3, 37, 31, False, True), (2, 97, 31, False, True)])
def test_padded_channels(dev, B, T, K, causal, masked):
    """d_eff = 144: channels 144.. zero-padded; LayerNorm statistics over the
    first 144 in every LayerNorm of the fused kernel, zeros stay zeros."""
    c = _Case(dev, B, T, K, causal, masked, 512, deff=144)
    with torch.no_grad():
        out, y = c.fused()
        ref, yref = c.two_launches()
    assert_close(out, ref, rtol=2e-2, name="padded out")
    assert_close(y.float(), yref.float(), rtol=2e-2, name="padded projection")
    assert float(out[:, 144:].abs().max()) == 0.0


@pytest.mark.parametrize("B,T", [(2, 97), (3, 37), (1, 5)])
def test_dead_rows_untouched(dev, B, T):
    """Tiles whose frames run past T (and the last utterance's past B*T)
    store nothing there: rows at or beyond B*T keep their sentinel, and
    every row below is written."""
    from speechbrain_amd import _enc
    c = _Case(dev, B, T, 31, False, True, 512)
    a, b = c.blocks()
    M, pad = B * T, 64
    out = torch.full((M + pad, D), 777.0, device=dev)
    y = torch.full((M + pad, 768), 777.0, device=dev, dtype=torch.bfloat16)
    ln0, w1p, b1p, wc, bc, causal, ln1, w2, b2 = c.cm.fused_params()
    gp, bp, ep = a[6]
    with torch.no_grad():
        _enc._conv_ffn_chain_into(out, y, c.x, B, T, c.o, c.wo, c.bo, ln0[0], ln0[1], ln0[2], w1p, b1p, wc, bc, causal,
                                  ln1[0], ln1[1], ln1[2], w2, b2, c.kpm, _enc.ACT["swish"], 0.0, a[0][0], a[0][1],
                                  a[0][2], a[1], a[2], a[3], a[4], a[5], gp, bp, ep, b[0][0], b[0][1], b[0][2], b[1],
                                  b[2], b[3], b[4], b[5], c.lns[3][0], c.lns[3][1], c.lns[3][2], c.wp, D)
        ref, yref = c.two_launches()
    assert bool((out[M:] == 777.0).all()) and bool((y[M:] == 777.0).all())
    assert_close(out[:M], ref, rtol=2e-2, name="rows below B*T")
    assert_close(y[:M].float(), yref.float(), rtol=2e-2, name="projection rows below B*T")


def test_graph_replay(dev):
    c = _Case(dev, 2, 97, 31, False, True, 1024)
    with torch.no_grad():
        out, y = c.fused()  # weight images built outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gout, gy = c.fused()
        for _ in range(2):
            gout.fill_(-1.0)
            gy.fill_(-1.0)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(gout, out) and torch.equal(gy, y)


def test_encoder_conv_chain_on_vs_off(dev):
    from speechbrain_amd.lobes.models.transformer import Conformer as C
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    torch.manual_seed(0)
    tr = TransformerASR(tgt_vocab=10, input_size=640, d_model=256, nhead=4, num_encoder_layers=3,
                        num_decoder_layers=0, d_ffn=1024, dropout=0.0, encoder_module="conformer",
                        attention_type="RelPosMHAXL", normalize_before=True, causal=False,
                        kernel_size=31).to(dev).eval()
    src = torch.randn(2, 100, 640, device=dev)
    lens = torch.tensor([1.0, 0.7], device=dev)
    prev = C.USE_CONV_CHAIN
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        try:
            C.USE_CONV_CHAIN = True
            y_on = tr.encode(src, lens)
            C.USE_CONV_CHAIN = False
            y_off = tr.encode(src, lens)
        finally:
            C.USE_CONV_CHAIN = prev
    assert_close(y_on, y_off, rtol=2e-2, name="encoder with the conv module in the chain launch")
