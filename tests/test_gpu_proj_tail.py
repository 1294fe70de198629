"""The projection tail of the fused layer kernels (csrc/ffn.hip, ffn_body with
PROJ: y = next-LN(out) . Wp^T in bf16, the in_proj of the next layer), in
every instance that has one — ffn_proj, ffn_chain, conv_ffn_chain and
src_ffn_proj — against a float64 restatement on the bf16-rounded weights, at
the project's 2e-2 for fused-module tests (conftest.assert_close, as
test_gpu_conv_chain.py states it).  All shapes are D = 256 with M = 50 rows:
one full 48-row workgroup (stores interleaved into the projection steps) and
one with two live rows (stores at the block ends); np = 768 is three column
blocks: the hand-over of a block's y to the next block's steps and the last
block's stores.

Column placement is checked exactly: with Wp[n, n % 256] = 2^-(n // 256) each
y value is one bf16 value times a power of two, so y[:, 256 k + c] must be
y[:, c] * 2^-k bit for bit, and y[:, :256] is next-LN(out) rounded to bf16."""
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close
from test_gpu_layer_phases import _case, _conv_args, ln64

pytestmark = pytest.mark.gpu

D, M = 256, 50
SENT, PADR = 777.0, 64


def _act64(h, act):
    return h * torch.sigmoid(h) if act == "swish" else F.gelu(h)  # erf form, as act_fn<ACT_GELU>


def _block(gen, H, deff, dev):
    """One FFN block's parameters (channels deff.. zero-padded): the float64
    copies of the bf16-rounded weights and the device tensors the kernels take."""
    ch = (torch.arange(D) < deff).float()
    w1 = (torch.randn(H, D, generator=gen) / 16 * ch[None, :]).to(torch.bfloat16)
    w2 = (torch.randn(D, H, generator=gen) / 16 * ch[:, None]).to(torch.bfloat16)
    b1 = torch.randn(H, generator=gen) * 0.1
    b2 = torch.randn(D, generator=gen) * 0.1 * ch
    return dict(w1=w1, w2=w2, b1=b1, b2=b2, dev=tuple(t.to(dev).contiguous() for t in (w1, b1, w2, b2)))


def _ln(gen, deff):
    ch = (torch.arange(D) < deff).float()
    return ((torch.randn(D, generator=gen) * 0.5 + 1) * ch, torch.randn(D, generator=gen) * 0.1 * ch, 1e-5)


def _to(ln, dev):
    return (ln[0].to(dev), ln[1].to(dev), ln[2])


def _ffn64(x, ln0, blk, alpha, act, deff):
    h = ln64(x, *ln0, deff=deff) @ blk["w1"].double().T + blk["b1"].double()
    return x.double() + alpha * (_act64(h, act) @ blk["w2"].double().T + blk["b2"].double())


def _wp(gen, np_, deff, dev):
    ch = (torch.arange(D) < deff).float()
    wp = (torch.randn(np_, D, generator=gen) / 16 * ch[None, :]).to(torch.bfloat16)
    return wp, wp.to(dev).contiguous()


def _rows(gen, deff):
    ch = (torch.arange(D) < deff).float()
    return ((torch.randn(M, D, generator=gen) * 2 + 0.3) * ch).contiguous()


def _report(name, out, y, ref_out, ref_y):
    print(f"{name}: out max err {float((out.double().cpu() - ref_out).abs().max()):.3e} (max |ref| "
          f"{float(ref_out.abs().max()):.2f}), y max err {float((y.double().cpu() - ref_y).abs().max()):.3e} "
          f"(max |ref| {float(ref_y.abs().max()):.2f})")


# ------------------------------------------------------------------- ffn_proj
@pytest.mark.parametrize("act,np_,deff", [("swish", 256, 256), ("swish", 768, 256), ("gelu", 256, 256),
                                          ("gelu", 768, 256), ("swish", 768, 144)])
def test_ffn_proj_vs_float64(dev, act, np_, deff):
    from speechbrain_amd import _enc
    H = 256
    gen = torch.Generator().manual_seed(5)
    x, blk = _rows(gen, deff), _block(gen, H, deff, dev)
    ln0, lnn = _ln(gen, deff), _ln(gen, deff)
    wp, wpd = _wp(gen, np_, deff, dev)
    ref_out = _ffn64(x, ln0, blk, 0.5, act, deff)
    ref_y = ln64(ref_out, *lnn, deff=deff) @ wp.double().T
    w1, b1, w2, b2 = blk["dev"]
    out, y = _enc.ffn_proj(x.to(dev), _to(ln0, dev), w1, b1, act, 0.0, w2, b2, 0.5, _to(lnn, dev), wpd, deff=deff)
    _report(f"ffn_proj {act} np {np_} deff {deff}", out, y, ref_out, ref_y)
    assert_close(out, ref_out.float(), rtol=2e-2, name="ffn_proj out")
    assert_close(y.float(), ref_y.float(), rtol=2e-2, name="ffn_proj y")
    if deff < D:
        assert torch.equal(out[:, deff:], torch.zeros_like(out[:, deff:]))


# ----------------------------------------------------- column placement, exact
def test_projection_column_placement_exact(dev):
    """One non-zero per row of Wp, a power of two: every product is exact and
    there is one per sum, so y[:, c] = bf16(u[:, c]) and y[:, 256 k + c] =
    y[:, c] * 2^-k with no rounding (values of order 1, far from the
    subnormals).  u = next-LN(out) is computed by the kernel in fp32 from the
    fp32 `out` it stores and rounded to bf16 once: against float64 LayerNorm of
    that same `out`, the difference is the rounding, at most half a bf16 ulp
    (2^-9 relative), plus the fp32 LayerNorm's own error (~1e-6 relative,
    which can turn a value on a rounding boundary: still under one ulp).  The
    bound is one ulp, 2^-8 |u|, plus 1e-5 for values near zero."""
    from speechbrain_amd import _enc
    H, NP = 256, 768
    gen = torch.Generator().manual_seed(6)
    x, blk = _rows(gen, D), _block(gen, H, D, dev)
    ln0, lnn = _ln(gen, D), _ln(gen, D)
    n = torch.arange(NP)
    wp = torch.zeros(NP, D)
    wp[n, n % 256] = 2.0 ** -(n // 256).float()
    w1, b1, w2, b2 = blk["dev"]
    out, y = _enc.ffn_proj(x.to(dev), _to(ln0, dev), w1, b1, "swish", 0.0, w2, b2, 0.5, _to(lnn, dev),
                           wp.to(torch.bfloat16).to(dev).contiguous())
    y = y.float().cpu()
    for k in (1, 2):
        assert torch.equal(y[:, 256 * k:256 * (k + 1)], y[:, :256] * 2.0 ** -k), f"column block {k}"
    u = ln64(out.cpu(), *lnn)
    err = (y[:, :256].double() - u).abs()
    print(f"column placement: max |y - LN64(out)| {float(err.max()):.3e}, max |u| {float(u.abs().max()):.3f}")
    assert bool((err <= 2.0 ** -8 * u.abs() + 1e-5).all()), f"max err {float(err.max()):.3e}"
    assert float(u.abs().max()) > 1.0  # the check is not vacuous


# ----------------------------------------------------- other projection paths
def test_ffn_chain_proj_vs_float64(dev):
    from speechbrain_amd import _enc
    from speechbrain_amd._enc import lib, ptr, stream_of
    H, NP = 256, 768
    gen = torch.Generator().manual_seed(7)
    x, a, b = _rows(gen, D), _block(gen, H, D, dev), _block(gen, H, D, dev)
    ln0a, lnp, ln0b, lnn = (_ln(gen, D) for _ in range(4))
    wp, wpd = _wp(gen, NP, D, dev)
    zp = ln64(_ffn64(x, ln0a, a, 0.5, "swish", D), *lnp)
    ref_out = _ffn64(zp, ln0b, b, 0.5, "swish", D)
    ref_y = ln64(ref_out, *lnn) @ wp.double().T
    out = torch.full((M + PADR, D), SENT, device=dev)
    y = torch.full((M + PADR, NP), SENT, device=dev, dtype=torch.bfloat16)
    xd = x.to(dev)
    (w1, b1, w2, b2), (w1b, b1b, w2b, b2b) = a["dev"], b["dev"]
    g0, b0, e0 = _to(ln0a, dev)
    gp, bp, ep = _to(lnp, dev)
    g0b, b0b, e0b = _to(ln0b, dev)
    gn, bn, en = _to(lnn, dev)
    img = _enc.ffn_image(w1, w2, w1b, w2b, wpd)
    rc = lib().sbk_ffn_chain(ptr(xd), M, D, D, H, _enc.ACT["swish"], 0.0, ptr(g0), ptr(b0), e0, ptr(b1), ptr(b2), 0.5,
                             ptr(gp), ptr(bp), ep, ptr(g0b), ptr(b0b), e0b, ptr(b1b), ptr(b2b), 0.5, ptr(out), ptr(gn),
                             ptr(bn), en, None, 1, ptr(img), img.numel(), NP, ptr(y), stream_of(xd))
    assert rc == 0
    assert torch.equal(out[M:], torch.full_like(out[M:], SENT)) and torch.equal(y[M:], torch.full_like(y[M:], SENT))
    _report("ffn_chain np 768", out[:M], y[:M], ref_out, ref_y)
    assert_close(out[:M], ref_out.float(), rtol=2e-2, name="ffn_chain out")
    assert_close(y[:M].float(), ref_y.float(), rtol=2e-2, name="ffn_chain y")


@pytest.mark.parametrize("B,T,K", [(2, 50, 31),   # a tile with two live rows next to the other utterance's rows
                                   (2, 96, 31)])  # only full tiles
def test_conv_ffn_chain_proj_vs_float64(dev, B, T, K):
    """Row by row against the float64 layer boundary of
    test_gpu_layer_phases.py (its cached case and reference): a row of
    utterance 1 written by utterance 0's last workgroup would differ."""
    from speechbrain_amd import _enc
    c, (ref_out, ref_y, _) = _case(dev, B, T, K, False, D)
    a, b = c.blocks()
    Mc = B * T
    out = torch.full((Mc + PADR, D), SENT, device=dev)
    y = torch.full((Mc + PADR, 768), SENT, device=dev, dtype=torch.bfloat16)
    gp, bp, ep = a[6]
    with torch.no_grad():
        _enc._conv_ffn_chain_into(out, y, c.x, B, T, *_conv_args(c), _enc.ACT["swish"], 0.0, a[0][0], a[0][1], a[0][2],
                                  a[1], a[2], a[3], a[4], a[5], gp, bp, ep, b[0][0], b[0][1], b[0][2], b[1], b[2], b[3],
                                  b[4], b[5], c.lns[3][0], c.lns[3][1], c.lns[3][2], c.wp, D)
    assert torch.equal(out[Mc:], torch.full_like(out[Mc:], SENT)) and torch.equal(y[Mc:], torch.full_like(y[Mc:], SENT))
    _report(f"conv_ffn_chain B {B} T {T} K {K}", out[:Mc], y[:Mc], ref_out, ref_y)
    assert_close(out[:Mc], ref_out.float(), rtol=2e-2, name="conv chain out")
    assert_close(y[:Mc].float(), ref_y.float(), rtol=2e-2, name="conv chain y")


def test_src_ffn_proj_vs_float64(dev):
    from speechbrain_amd import _enc
    H, NP, Kin = 256, 768, 64
    gen = torch.Generator().manual_seed(8)
    blk = _block(gen, H, D, dev)
    ln0, lnn = _ln(gen, D), _ln(gen, D)
    wp, wpd = _wp(gen, NP, D, dev)
    av = torch.randn(M, Kin, generator=gen).to(torch.bfloat16)
    ws = (torch.randn(D, Kin, generator=gen) / 4).to(torch.bfloat16)
    bs = torch.randn(D, generator=gen) * 0.3
    x = av.double() @ ws.double().T + bs.double()
    ref_out = _ffn64(x, ln0, blk, 0.5, "swish", D)
    ref_y = ln64(ref_out, *lnn) @ wp.double().T
    out = torch.full((M + PADR, D), SENT, device=dev)
    y = torch.full((M + PADR, NP), SENT, device=dev, dtype=torch.bfloat16)
    w1, b1, w2, b2 = blk["dev"]
    g0, b0, e0 = _to(ln0, dev)
    gn, bn, en = _to(lnn, dev)
    _enc._src_ffn_proj_into(out, y, None, av.to(dev).contiguous(), ws.to(dev).contiguous(), bs.to(dev), None, 1, g0, b0,
                            e0, w1, b1, _enc.ACT["swish"], 0.0, w2, b2, 0.5, None, None, 0.0, gn, bn, en, wpd, D)
    assert torch.equal(out[M:], torch.full_like(out[M:], SENT)) and torch.equal(y[M:], torch.full_like(y[M:], SENT))
    _report("src_ffn_proj Kin 64", out[:M], y[:M], ref_out, ref_y)
    assert_close(out[:M], ref_out.float(), rtol=2e-2, name="src_ffn_proj out")
    assert_close(y[:M].float(), ref_y.float(), rtol=2e-2, name="src_ffn_proj y")
