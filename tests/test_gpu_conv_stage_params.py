"""The parameters of the conv stage's middle phases (convstage.h) in
sbk_conv_ffn_chain and sbk_conv_ffn_tail: the depthwise taps and the conv bias
come packed from an image (sbk_dw_image, cached per tensor and version), phase
1's bias from LDS, and every phase's parameter vectors are issued one phase
early and waited for by count.

The shapes are where that can go wrong, not the workload's: one clamped row,
the 48-frame tile edge and a middle tile (T = 1, 47, 48, 49, 97); kernel size
31 non-causal and causal (an odd tap count, the zero 32nd tap), 3 (15
zero-padded tap pairs) and 15 (the last live pair half zero); the conv bias, b2
and the key-padding mask given and null (a null one reads another vector in
its place and must add nothing); d_eff = 144.

Every case is checked against the two launches the fused one replaces
(sbk_conv_module_pre, which reads the fp32 taps itself, then sbk_ffn_chain /
sbk_ffn) at the project's 2e-2 for a fused launch against its parts
(test_gpu_conv_stage_start.py).  The image, its cache and determinism are
bit-exact."""
import pytest
import torch

from test_gpu_conv_stage_start import D, _Case, _check

pytestmark = pytest.mark.gpu

TS = [1, 47, 48, 49, 97]
CONVS = [(31, False), (31, True), (3, False), (15, False)]  # (kernel size, causal)


def _case(dev, T, K, causal, cbias=True, b2=True, masked=True, deff=None):
    """_Case with the conv bias and / or b2 (after_conv's Linear bias) dropped."""
    c = _Case(dev, 2, T, K, causal, masked=masked, deff=deff)
    if not cbias:
        c.cm.conv.bias = None
    if not b2:
        c.cm.after_conv[2].bias = None
    return c


@pytest.mark.parametrize("K,causal", CONVS)
@pytest.mark.parametrize("T", TS)
def test_tile_and_tap_edges(dev, T, K, causal):
    """Two utterances, every parameter given, ragged mask: chain and tail against the two launches."""
    _check(_case(dev, T, K, causal))


@pytest.mark.parametrize("cbias,b2,masked", [(False, True, True), (True, False, True), (True, True, False),
                                             (False, False, False)])
@pytest.mark.parametrize("K,causal", CONVS)
@pytest.mark.parametrize("T", [47, 97])
def test_null_parameters(dev, T, K, causal, cbias, b2, masked):
    """A null conv bias is a zero bias row of the image; null b2 / kpm are
    loaded from another vector and zeroed after the wait."""
    c = _case(dev, T, K, causal, cbias=cbias, b2=b2, masked=masked)
    conv = c.cm.fused_params()
    assert (conv[4] is None) == (not cbias) and (conv[8] is None) == (not b2)
    _check(c)


@pytest.mark.parametrize("K,causal", CONVS)
@pytest.mark.parametrize("T", [49, 97])
def test_padded_channels(dev, T, K, causal):
    """d_eff = 144: the padded channels' taps and biases are zero and their outputs exactly zero."""
    out, u = _check(_case(dev, T, K, causal, deff=144))
    assert float(out[:, 144:].abs().max()) == 0.0 and float(u[:, 144:].abs().max()) == 0.0


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("K", [31, 30, 15, 3, 1])
def test_dw_image_words(dev, K, bias):
    """Word c of row j = bf16(tap 2j) | bf16(tap 2j + 1) << 16 of channel c
    (round to nearest even, as torch's cast), zero for taps >= K; row 16 the
    fp32 bias bits, or zero."""
    from speechbrain_amd import _enc
    from speechbrain_amd._lib import lib
    torch.manual_seed(K)
    wc = (torch.randn(K, D, device=dev) / 4).contiguous()
    bc = torch.randn(D, device=dev) if bias else None
    img = _enc.dw_image(wc, bc)
    assert img.dtype == torch.int32 and img.numel() == lib().sbk_dw_image_elems(D) == 17 * D
    taps = torch.zeros(32, D, device=dev)
    taps[:K] = wc
    h = taps.to(torch.bfloat16).view(torch.int16).to(torch.int64) & 0xFFFF  # (32, D) bf16 bits
    want = h[0::2] | (h[1::2] << 16)
    want = torch.where(want >= 2 ** 31, want - 2 ** 32, want).to(torch.int32)  # the word as int32
    got = img.view(17, D)
    assert torch.equal(got[:16], want)
    assert torch.equal(got[16], bc.view(torch.int32) if bias else torch.zeros(D, device=dev, dtype=torch.int32))


def test_dw_image_refuses_bad_arguments(dev):
    from speechbrain_amd._lib import lib, ptr
    wc = torch.randn(31, D, device=dev)
    img = torch.empty(17 * D, device=dev, dtype=torch.int32)
    L = lib()
    assert L.sbk_dw_image_elems(144) == -1
    for args in ((None, None, 31, D, ptr(img)), (ptr(wc), None, 31, D, None), (ptr(wc), None, 32, D, ptr(img)),
                 (ptr(wc), None, 0, D, ptr(img)), (ptr(wc), None, 31, 144, ptr(img)),
                 (ptr(wc), None, 31, D, ptr(img[1:]))):
        assert L.sbk_dw_image(*args, None) == 1001


def test_image_cache_follows_the_weights(dev):
    """No change: the second call reuses the image.  An in-place change of
    conv.weight or conv.bias (a version bump) rebuilds it, and the fused
    output follows the two-launch reference again."""
    from speechbrain_amd import _enc
    c = _case(dev, 49, 31, False)
    with torch.no_grad():
        out0, _ = _check(c)
        _, _, _, wc, bc, *_ = c.cm.fused_params()
        img = _enc.dw_image(wc, bc)
        p0 = img.data_ptr()
        _check(c)
        _, _, _, wc1, bc1, *_ = c.cm.fused_params()
        assert wc1 is wc and bc1 is bc and _enc.dw_image(wc1, bc1).data_ptr() == p0
        c.cm.conv.weight.mul_(-1.5)
        out1, _ = _check(c)
        assert not torch.equal(out1, out0)
        c.cm.conv.bias.add_(0.25)
        out2, _ = _check(c)
        assert not torch.equal(out2, out1)


@pytest.mark.parametrize("K,causal", CONVS)
def test_deterministic_and_graph_replay(dev, K, causal):
    """Two calls, and one call inside a captured graph replayed twice, give the same bits."""
    c = _case(dev, 97, K, causal)
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
