"""The positional-band ring of relpos_flash_dma_kernel<true> (csrc/attention.hip).

The kernel keeps the band in LDS as a ring of two 64-row segments: chunk c
reads segments c and c + 1, and segment c + 2 is staged over segment c after
barrier B.  A row read from the wrong half, a segment staged too early or too
late, or a wrong clamp would all put another band row under a score.  So the
band rows here are a function of their row index (every row distinct), and
the LDS-DMA kernel (bf16, dh = 64, aligned operands) is compared with the
general relpos_flash_kernel<bf16_t, 64, false> on the same values (reached by
giving pk a row stride that is no multiple of 8), and both with a float64
reference.

Shapes (B = 2, H = 4): T = 64 (one chunk, no ring step), 65 (two chunks, the
first ring step, a last chunk of one key), 129 and 200 (both parities, every
query tile's first band row different), 376 (the encoder's length; six
chunks).  At every T the first query tile stages its last segment and the
last query tile its first segment through the clamped path (band rows past
2T - 2, before 0); T = 376 is the case named for it.  Each with and without a
key-padding mask; the mask pads a suffix of utterance 1 that covers a whole
chunk wherever the length leaves one (T >= 65).

Bound: the one tests/test_gpu_selfattn_paths.py uses for bf16 kernels on
ordinary values, 2e-2 max(1, |ref|), between the two kernels and between each
kernel and the reference.  test_wrong_band_rows_are_visible shows on the CPU
that exchanging one 16-row block of the band with the block 64 rows on moves
the reference by more than four times that bound, at every shape."""
import math

import pytest
import torch

gpu = pytest.mark.gpu

B, H, DH = 2, 4, 64
D = H * DH
TS = (64, 65, 129, 200, 376)
SCALE = 1.0 / math.sqrt(D)


def _band(T):
    """(2T - 1, D) band rows, each a function of its row index."""
    r = torch.arange(2 * T - 1, dtype=torch.float64)[:, None]
    e = torch.arange(D, dtype=torch.float64)[None, :]
    return (1.5 * torch.cos(0.37 * (r + 1.0) * (e % 8 + 1.0) + 0.61 * e)).to(torch.bfloat16)


_CACHE = {}


def _inputs(T):
    if T not in _CACHE:
        g = torch.Generator().manual_seed(1000 + T)
        qkv = torch.randn(B * T, H, 3, DH, generator=g)
        qkv[:, :, 2] *= 2.0
        qkv = qkv.to(torch.bfloat16)
        pbu, pbv = 0.5 * torch.randn(D, generator=g), 0.5 * torch.randn(D, generator=g)
        valid = T - 1 if T == 65 else T - 70 if T > 65 else T - 5  # utterance 1's length under the mask
        kpm = torch.zeros(B, T, dtype=torch.bool)
        kpm[1, valid:] = True
        _CACHE[T] = (qkv, _band(T), pbu, pbv, kpm)
    return _CACHE[T]


def _reference(T, masked, pk=None):
    """out (B*T, D) in float64 from the bf16 operands."""
    qkv, pk0, pbu, pbv, kpm = _inputs(T)
    pk = (pk0 if pk is None else pk).double().view(2 * T - 1, H, DH)
    x = qkv.double().view(B, T, H, 3, DH)
    q, k, v = x[:, :, :, 0], x[:, :, :, 1], x[:, :, :, 2]
    ac = torch.einsum("bihd,bjhd->bhij", q + pbu.double().view(H, DH), k)
    bd_all = torch.einsum("bihd,rhd->bhir", q + pbv.double().view(H, DH), pk)
    idx = (T - 1 - torch.arange(T)[:, None] + torch.arange(T)[None, :]).expand(B, H, T, T)
    s = (ac + bd_all.gather(-1, idx)) * SCALE
    if masked:
        s = s.masked_fill(kpm[:, None, None, :], -math.inf)
    return torch.einsum("bhij,bjhd->bihd", s.softmax(-1), v).reshape(B * T, D)


_REF = {}


def _ref(T, masked):
    if (T, masked) not in _REF:
        _REF[T, masked] = _reference(T, masked)
    return _REF[T, masked]


def _bound(ref):
    return 2e-2 * ref.abs().clamp(min=1.0)


@pytest.mark.parametrize("T", TS)
def test_wrong_band_rows_are_visible(T):
    """The reference moves by more than 4 bounds when band rows T - 8 .. T + 7
    (around the diagonal, read by every query tile) change places with the
    rows 64 on (or the band's last 16 rows, where it ends sooner): the
    comparison below can see a 16-row tile taken from the other half of the
    ring."""
    pk = _inputs(T)[1].clone()
    a, b = T - 8, T - 8 + min(64, 2 * T - 1 - 16 - (T - 8))
    blk = pk[a:a + 16].clone()
    pk[a:a + 16] = pk[b:b + 16]
    pk[b:b + 16] = blk
    ref = _ref(T, False)
    moved = ((_reference(T, False, pk) - ref).abs() / _bound(ref)).max()
    assert float(moved) > 4.0, (T, float(moved))


def _launch(T, masked, dev, general):
    from speechbrain_amd import _enc
    qkv, pk, pbu, pbv, kpm = _inputs(T)
    qkv_d = qkv.view(B * T, 3 * D).to(dev)
    if general:  # a pk row stride of D + 4 elements sends the call to relpos_flash_kernel
        pk_d = torch.zeros(2 * T - 1, D + 4, dtype=torch.bfloat16, device=dev)[:, :D]
        pk_d.copy_(pk)
    else:
        pk_d = pk.to(dev)
    assert (pk_d.stride(0) % 8 != 0) == general and qkv_d.data_ptr() % 16 == 0 and pk_d.data_ptr() % 16 == 0
    kpm_d = kpm.to(torch.uint8).to(dev) if masked else None
    out, probs = _enc.relpos_attention(qkv_d, pk_d, pbu.to(dev), pbv.to(dev), kpm_d, B, T, H, DH, SCALE)
    assert probs is None and out.dtype == torch.bfloat16 and out.shape == (B * T, D)
    return out.double().cpu()


@gpu
@pytest.mark.parametrize("masked", (False, True), ids=("nomask", "kpm"))
@pytest.mark.parametrize("T", TS)
def test_band_ring_matches_general_kernel(dev, T, masked):
    ref = _ref(T, masked)
    dma, gen = _launch(T, masked, dev, False), _launch(T, masked, dev, True)
    assert torch.isfinite(dma).all() and torch.isfinite(gen).all()
    for tag, got, want in (("dma vs general", dma, gen), ("dma vs float64", dma, ref), ("general vs float64", gen, ref)):
        ratio = (got - want).abs() / _bound(want)
        worst = int(ratio.argmax())
        print(f"band_ring T={T} {'kpm' if masked else 'nomask'} {tag}: max err {float((got - want).abs().max()):.3e}, "
              f"worst err / bound {float(ratio.max()):.3f}, {int((got != want).sum())} of {got.numel()} differ")
        assert float(ratio.max()) <= 1.0, (f"{tag}: row {worst // D} (b {worst // D // T}, query {worst // D % T}), "
                                           f"head {worst % D // DH}: {float(got.flatten()[worst])} vs "
                                           f"{float(want.flatten()[worst])}")
