"""The end of the encoder stack in one launch, and the kept linear_pos table.

sbk_conv_ffn_tail: the last layer's convolution module in front of its FFN2 +
norm2 + the encoder's closing LayerNorm, against the two launches it replaces
(sbk_conv_module_pre, then sbk_ffn with post-LN and fp32 next-LN).  The
rounding points are the same and the summation order differs, so the bound is
the project's 2e-2 for a fused launch against the launches it replaces
(test_gpu_conv_chain.py).

sbk_src_ffn_proj: the src Linear (and the key padding mask) in front of layer
0's FFN1 + norm1 + in_proj, against sbk_gemm followed by sbk_ffn_proj, same
bound; the mask must equal sbk_length_mask's bit for bit.

ConformerEncoder.projected_pos: the projection of the relative table is kept
for the longest T seen; shorter calls get row slices that must equal a fresh
GEMM on their own table bit for bit."""
import pytest
import torch

from conftest import assert_close
from test_gpu_conv_chain import SHAPES, D, _Case

pytestmark = pytest.mark.gpu


def _tail(c, u=None):
    from speechbrain_amd import _enc
    a, _ = c.blocks()
    if u is None:
        return _enc.conv_ffn_tail(c.x, c.B, c.T, (c.o, c.wo, c.bo), c.cm.fused_params(), c.kpm, a, c.lns[3],
                                  "swish", 0.0, deff=c.deff)
    ln0, w1p, b1p, wc, bc, causal, ln1, w2, b2 = c.cm.fused_params()
    gp, bp, ep = a[6]
    _enc._conv_ffn_tail_into(u, c.x, c.B, c.T, c.o, c.wo, c.bo, ln0[0], ln0[1], ln0[2], w1p, b1p, wc, bc, causal,
                             ln1[0], ln1[1], ln1[2], w2, b2, c.kpm, _enc.ACT["swish"], 0.0, a[0][0], a[0][1], a[0][2],
                             a[1], a[2], a[3], a[4], a[5], gp, bp, ep, c.lns[3][0], c.lns[3][1], c.lns[3][2],
                             c.deff or D)
    return u


def _tail_two_launches(c):
    from speechbrain_amd import _enc
    ln0, w1, b1, w2, b2, alpha, post_ln = c.blocks()[0]
    mid = c.cm.run_fused(c.x, c.B, c.T, c.kpm, pre=(c.o, c.wo, c.bo))
    _, u = _enc.ffn(mid, ln0, w1, b1, "swish", 0.0, w2, b2, alpha, post_ln=post_ln, next_ln=c.lns[3],
                    next_dtype=torch.float32, deff=c.deff)
    return u


@pytest.mark.parametrize("H", [512, 1024])
@pytest.mark.parametrize("B,T,K,causal,masked", SHAPES)
def test_tail_vs_two_launches(dev, B, T, K, causal, masked, H):
    """Into a buffer with 64 sentinel rows past B*T: tiles whose frames run
    past an utterance's end (and the last one's past B*T) store nothing."""
    c = _Case(dev, B, T, K, causal, masked, H)
    M = B * T
    buf = torch.full((M + 64, D), 777.0, device=dev)
    with torch.no_grad():
        _tail(c, buf)
        ref = _tail_two_launches(c)
    assert ref.dtype == torch.float32
    assert bool((buf[M:] == 777.0).all())
    assert_close(buf[:M], ref, rtol=2e-2, name="tail u")


@pytest.mark.parametrize("B,T,K,causal,masked", [(3, 37, 31, False, True), (2, 97, 31, False, True)])
def test_tail_padded_channels(dev, B, T, K, causal, masked):
    """d_eff = 144: statistics over the first 144 channels in every LayerNorm
    of the launch, the zero-padded channels come out exactly zero."""
    c = _Case(dev, B, T, K, causal, masked, 512, deff=144)
    with torch.no_grad():
        u = _tail(c)
        ref = _tail_two_launches(c)
    assert_close(u, ref, rtol=2e-2, name="padded tail u")
    assert float(u[:, 144:].abs().max()) == 0.0


def test_tail_graph_replay(dev):
    c = _Case(dev, 2, 97, 31, False, True, 1024)
    with torch.no_grad():
        u = _tail(c)  # weight images built outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gu = _tail(c)
        for _ in range(2):
            gu.fill_(-1.0)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(gu, u)


# ---- the head: src Linear (+ key padding mask) + FFN1 + norm1 + in_proj in one launch

class _Head:
    """Inputs of one (B, T, Kin, H) case; deff < 256: output channels deff..
    zero-padded (rows of Ws, bias, LayerNorm gains and biases, FFN weights)."""

    def __init__(self, dev, B, T, Kin, H, deff=None):
        from speechbrain_amd import _enc
        from speechbrain_amd.nnet.activations import Swish
        from speechbrain_amd.nnet.attention import PositionalwiseFeedForward
        torch.manual_seed(B * 1000 + T + Kin + H)
        self.B, self.T, self.M, self.deff = B, T, B * T, deff
        ch = (torch.arange(D) < (deff or D)).float().to(dev)
        self.a = torch.randn(B * T, Kin, device=dev).to(torch.bfloat16)
        self.ws = _enc.cast_bf16(torch.randn(D, Kin, device=dev) / Kin ** 0.5 * ch[:, None])
        self.bs = torch.randn(D, device=dev) * 0.3 * ch
        self.f = PositionalwiseFeedForward(H, input_size=D, activation=Swish).to(dev).eval()
        with torch.no_grad():
            self.f.ffn[0].weight.mul_(ch[None, :])
            self.f.ffn[3].weight.mul_(ch[:, None])
            self.f.ffn[3].bias.mul_(ch)
        if deff:
            self.f._deff = deff
        self.lns = [((torch.randn(D, device=dev) * 0.5 + 1) * ch, torch.randn(D, device=dev) * 0.1 * ch, 1e-5)
                    for _ in range(2)]
        self.wp = _enc.cast_bf16((torch.randn(768, D) / 16).to(dev) * ch[None, :])

    def fused(self, rel_len=None):
        return self.f.run_fused_src_proj(self.a, self.ws, self.bs, self.lns[0], 0.5, self.lns[1], self.wp,
                                         rel_len=rel_len, T=self.T)

    def two_launches(self):
        from speechbrain_amd import _enc
        x = _enc.gemm(self.a, self.ws, bias=self.bs, out_dtype=torch.float32)
        return self.f.run_fused_proj(x, self.lns[0], 0.5, self.lns[1], self.wp)

    def into(self, out, y, kpm, rel_len):
        from speechbrain_amd import _enc
        f = self.f
        w1, w2 = f.kernel_weights(torch.bfloat16)
        _enc._src_ffn_proj_into(out, y, kpm, self.a, self.ws, self.bs, rel_len, self.T, self.lns[0][0],
                                self.lns[0][1], self.lns[0][2], w1, f.ffn[0].bias.detach(), _enc.ACT["swish"], 0.0, w2,
                                f.ffn[3].bias.detach(), 0.5, None, None, 0.0, self.lns[1][0], self.lns[1][1],
                                self.lns[1][2], self.wp, self.deff or D)


@pytest.mark.parametrize("H", [512, 1024])
@pytest.mark.parametrize("Kin", [64, 640])
@pytest.mark.parametrize("B,T", [(1, 5), (3, 37), (2, 97), (2, 96)])
def test_head_vs_two_launches(dev, B, T, Kin, H):
    """Into buffers with 64 sentinel rows past M, which stay untouched in
    out, y and the mask."""
    c = _Head(dev, B, T, Kin, H)
    M = c.M
    out = torch.full((M + 64, D), 777.0, device=dev)
    y = torch.full((M + 64, 768), 777.0, device=dev, dtype=torch.bfloat16)
    kpm = torch.full((M + 64,), 9, device=dev, dtype=torch.uint8)
    rel = torch.linspace(1.0, 0.4, B, device=dev)
    from speechbrain_amd import _enc
    with torch.no_grad():
        c.into(out, y, kpm, rel)
        ref, yref = c.two_launches()
    assert bool((out[M:] == 777.0).all()) and bool((y[M:] == 777.0).all()) and bool((kpm[M:] == 9).all())
    assert_close(out[:M], ref, rtol=2e-2, name="head out")
    assert_close(y[:M].float(), yref.float(), rtol=2e-2, name="head projection")
    assert torch.equal(kpm[:M].view(B, T), _enc.length_mask(rel, T))


@pytest.mark.parametrize("B,T", [(3, 37), (2, 97)])
def test_head_padded_channels(dev, B, T):
    """d_eff = 144 with a zero-row-padded Ws: the padded columns are exactly 0."""
    c = _Head(dev, B, T, 640, 512, deff=144)
    with torch.no_grad():
        out, y, kpm = c.fused()
        ref, yref = c.two_launches()
    assert kpm is None
    assert_close(out, ref, rtol=2e-2, name="padded head out")
    assert_close(y.float(), yref.float(), rtol=2e-2, name="padded head projection")
    assert float(out[:, 144:].abs().max()) == 0.0


def test_head_graph_replay(dev):
    c = _Head(dev, 2, 97, 640, 1024)
    rel = torch.tensor([1.0, 0.6], device=dev)
    with torch.no_grad():
        out, y, kpm = c.fused(rel)  # weight images built outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            gout, gy, gk = c.fused(rel)
        for _ in range(2):
            gout.fill_(-1.0)
            gy.fill_(-1.0)
            gk.fill_(7)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(gout, out) and torch.equal(gy, y) and torch.equal(gk, kpm)


@pytest.mark.parametrize("T", [5, 37, 97])
def test_head_mask_equals_length_mask(dev, T):
    from speechbrain_amd import _enc
    rel = torch.tensor([1.0, 0.7, 0.5, 0.0, (T // 2) / T, 1e-7], device=dev)
    c = _Head(dev, rel.shape[0], T, 64, 512)
    with torch.no_grad():
        _, _, kpm = c.fused(rel)
        assert kpm.shape == (rel.shape[0], T) and torch.equal(kpm, _enc.length_mask(rel, T))
        buf = torch.full((c.M,), 9, device=dev, dtype=torch.uint8)
        c.into(torch.empty(c.M, D, device=dev), torch.empty(c.M, 768, device=dev, dtype=torch.bfloat16), buf, None)
    assert bool((buf == 9).all()), "rel_len=None stores no mask"


def test_head_refuses_partial_k_steps(dev):
    """Kin = 96 is no whole number of 64-wide K-steps: not supported, and the
    encoder then takes the two launches."""
    from speechbrain_amd import _enc
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    assert _enc.src_ffn_proj_supported(256, 640, 1024, 768) and _enc.src_ffn_proj_supported(256, 64, 512, 768)
    assert not _enc.src_ffn_proj_supported(256, 96, 1024, 768)
    assert not _enc.src_ffn_proj_supported(256, 832, 1024, 768)
    torch.manual_seed(0)
    tr = TransformerASR(tgt_vocab=10, input_size=96, d_model=256, nhead=4, num_encoder_layers=1,
                        num_decoder_layers=0, d_ffn=512, dropout=0.0, encoder_module="conformer",
                        attention_type="RelPosMHAXL", normalize_before=True, causal=False, kernel_size=31).to(dev).eval()
    assert not tr.encoder.takes_src(96, torch.bfloat16) and tr.encoder.takes_src(640, torch.bfloat16)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        y = tr.encode(torch.randn(2, 20, 96, device=dev), torch.tensor([1.0, 0.5], device=dev))
    assert y.shape == (2, 20, 256) and bool(torch.isfinite(y).all())


def _asr(dev, d_model, layers):
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    torch.manual_seed(0)
    return TransformerASR(tgt_vocab=10, input_size=640, d_model=d_model, nhead=4, num_encoder_layers=layers,
                          num_decoder_layers=0, d_ffn=1024, dropout=0.0, encoder_module="conformer",
                          attention_type="RelPosMHAXL", normalize_before=True, causal=False,
                          kernel_size=31).to(dev).eval()


@pytest.mark.parametrize("d_model,layers", [(256, 3), (144, 3), (256, 1)])
def test_encoder_fused_ends_on_vs_off(dev, d_model, layers):
    """The whole encoder (d 256, and d 144 on the padded shadow; one layer:
    no chain launch between the ends) with the fused end against the
    launches it replaces."""
    from speechbrain_amd.lobes.models.transformer import Conformer as C
    tr = _asr(dev, d_model, layers)
    src = torch.randn(2, 100, 640, device=dev)
    lens = torch.tensor([1.0, 0.7], device=dev)
    prev = C.USE_FUSED_ENDS
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        try:
            C.USE_FUSED_ENDS = True
            y_on = tr.encode(src, lens)
            C.USE_FUSED_ENDS = False
            y_off = tr.encode(src, lens)
        finally:
            C.USE_FUSED_ENDS = prev
    assert y_on.shape == (2, 100, d_model)
    assert_close(y_on, y_off, rtol=2e-2, name="encoder with the fused end")


# ---- the kept linear_pos projection

def _fresh_pk(tr, T, dev):
    from speechbrain_amd import _enc
    pos = tr.positional_encoding.table(T, dev, torch.bfloat16).reshape(-1, 256)
    return _enc.gemm(pos, tr.encoder.stacked_pos_weight(torch.bfloat16), out_dtype=torch.bfloat16)


def _encode(tr, T, dev, B=2):
    src = torch.randn(B, T, 640, device=dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        return tr.encode(src, torch.tensor([1.0, 0.7], device=dev))


def _entry(tr, dev):
    return tr.encoder._pk.get((str(dev), torch.bfloat16))


def test_pos_cache_slices_equal_a_fresh_gemm(dev):
    tr = _asr(dev, 256, 2)
    _encode(tr, 128, dev)
    big = _entry(tr, dev)
    assert big is not None and big[1] == 128
    assert torch.equal(big[2], _fresh_pk(tr, 128, dev))
    for T in (5, 50, 97):
        pos = tr.positional_encoding.table(T, dev, torch.bfloat16).reshape(-1, 256)
        pk = tr.encoder.projected_pos(pos, T, torch.bfloat16, big[0][0])
        assert _entry(tr, dev)[2] is big[2], "a shorter T must not replace the entry"
        assert pk.data_ptr() == big[2][128 - T].data_ptr() and pk.shape[0] == 2 * T - 1
        assert torch.equal(pk, _fresh_pk(tr, T, dev)), T
    # and the encoder's output through a slice equals the one without the cache
    from speechbrain_amd.lobes.models.transformer import Conformer as C
    torch.manual_seed(1)
    y_hit = _encode(tr, 50, dev)
    prev = C.USE_POS_CACHE
    try:
        C.USE_POS_CACHE = False
        torch.manual_seed(1)
        y_off = _encode(tr, 50, dev)
    finally:
        C.USE_POS_CACHE = prev
    assert torch.equal(y_hit, y_off)


def test_pos_cache_follows_the_weights_and_a_longer_T(dev):
    tr = _asr(dev, 256, 2)
    _encode(tr, 50, dev)
    first = _entry(tr, dev)
    _encode(tr, 97, dev)
    longer = _entry(tr, dev)
    assert longer[1] == 97 and torch.equal(longer[2], _fresh_pk(tr, 97, dev))
    with torch.no_grad():
        tr.encoder.layers[1].mha_layer.linear_pos.weight.add_(0.25)
    _encode(tr, 50, dev)
    again = _entry(tr, dev)
    assert again[1] == 50 and again[0] != first[0]
    assert torch.equal(again[2], _fresh_pk(tr, 50, dev))
    assert not torch.equal(again[2], first[2])


def test_pos_cache_is_not_filled_inside_a_capture(dev):
    tr = _asr(dev, 256, 2)
    src = torch.randn(2, 50, 640, device=dev)
    lens = torch.tensor([1.0, 0.7], device=dev)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        ref = tr.encode(src, lens)  # weight copies and images built outside the capture
        tr.encoder._pk.clear()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y = tr.encode(src, lens)
        assert _entry(tr, dev) is None
        y.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(y, ref)


def test_pos_cache_untouched_by_training(dev):
    tr = _asr(dev, 256, 2).train()
    src = torch.randn(2, 20, 640, device=dev)
    y = tr.encode(src, torch.tensor([1.0, 0.7], device=dev))
    assert y.requires_grad
    assert tr.encoder._pk == {}
