"""The phases of the fused layer kernels that are not GEMM (csrc/ffn.hip
row_ln, csrc/convstage.h LN0 / GLU / depthwise conv / LN1 + Swish) against
float64 torch:

* row_ln alone: sbk_ffn with zero W1, W2, b2 and both LayerNorms on returns
  out = LNp(x) and u = LNn(LNp(x)) in fp32; bound: the project's fp32 parity
  bound, 1e-4 of the largest reference value;
* sbk_conv_ffn_chain / sbk_conv_ffn_tail against a float64 restatement of one
  layer boundary on the bf16-rounded weights, at the 2e-2 of
  test_gpu_conv_chain.py; rows the launch does not own keep their sentinel;
* (CPU) the Swish instances of ffn.hip keep no scratch and fit 256 VGPRs."""
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 256
gpu = pytest.mark.gpu


def ln64(t, g, b, eps, deff=D):
    """LayerNorm in float64 over the first deff columns, zeros in the rest
    (tests/test_padded_shadow.py's ln_eff: what the kernels' d_eff / npad compute)."""
    t = t.double()
    y = F.layer_norm(t[..., :deff], (deff,), g[:deff].double(), b[:deff].double(), eps)
    return torch.cat([y, torch.zeros_like(t[..., deff:])], dim=-1)


# ---------------------------------------------------------------- row_ln alone
def _rows(kind, M, deff, gen):
    if kind == "normal":
        x = torch.randn(M, D, generator=gen)
    elif kind == "mean30":
        x = 30.0 + torch.randn(M, D, generator=gen)
    else:  # constant rows, each a multiple of 0.5: sums and means are exact in fp32, variance 0
        x = (0.5 * torch.arange(1, M + 1, dtype=torch.float32))[:, None].expand(M, D).clone()
    x[:, deff:] = 0.0
    return x.contiguous()


@gpu
@pytest.mark.parametrize("kind,deff,affine", [("normal", 256, False), ("mean30", 256, False), ("const", 256, True),
                                              ("normal", 144, True), ("mean30", 144, True), ("normal", 256, True)])
def test_row_ln_alone(dev, kind, deff, affine):
    from speechbrain_amd import _enc
    M, H = 50, 256
    gen = torch.Generator().manual_seed(11)
    x = _rows(kind, M, deff, gen)
    ch = (torch.arange(D) < deff).float()

    def ln(seed):
        g = torch.Generator().manual_seed(seed)
        if affine:
            return ((torch.randn(D, generator=g) * 0.5 + 1) * ch, torch.randn(D, generator=g) * 0.3 * ch, 1e-5)
        return (ch.clone(), torch.zeros(D), 1e-5)

    lp, ln_ = ln(1), ln(2)
    ref_out = ln64(x, *lp, deff=deff)
    ref_u = ln64(ref_out, *ln_, deff=deff)
    to = lambda t: tuple(v.to(dev) if isinstance(v, torch.Tensor) else v for v in t)  # noqa: E731
    w1 = torch.zeros(H, D, device=dev, dtype=torch.bfloat16)
    w2 = torch.zeros(D, H, device=dev, dtype=torch.bfloat16)
    out, u = _enc.ffn(x.to(dev), to(ln(3)), w1, torch.zeros(H, device=dev), "swish", 0.0, w2, torch.zeros(D, device=dev), 0.5,
                      post_ln=to(lp), next_ln=to(ln_), next_dtype=torch.float32, deff=deff)
    for name, got, ref in (("out = LNp(x)", out, ref_out), ("u = LNn(LNp(x))", u, ref_u)):
        err = float((got.double().cpu() - ref).abs().max())
        big = float(ref.abs().max())
        print(f"{kind} deff {deff} affine {affine}: {name} max err {err:.3e}, largest reference value {big:.3e}")
        assert err <= 1e-4 * big, f"{name}: {err:.3e} > 1e-4 * {big:.3e}"
    if deff < D:
        assert float(out[:, deff:].abs().max()) == 0.0 and float(u[:, deff:].abs().max()) == 0.0


# ------------------------------------------- one layer boundary in float64
def _bf(w):
    return w.detach().to(torch.bfloat16).double().cpu()


def _ffn64(f, x, ln0, alpha, deff):
    h = ln64(x, *ln0, deff=deff) @ _bf(f.ffn[0].weight).T + f.ffn[0].bias.detach().double().cpu()
    h = h * torch.sigmoid(h)
    return x + alpha * (h @ _bf(f.ffn[3].weight).T + f.ffn[3].bias.detach().double().cpu())


def _boundary64(c, B, T, K, kpm, deff):
    """out_proj + residual, conv module (LN0, pointwise + GLU, depthwise conv,
    LN1, Swish, pointwise, mask), FFN2 + norm2, FFN1, norm1 + projection, and
    the closing LayerNorm of the tail: (out, y, u_tail) in float64."""
    cpu = lambda t: t.detach().double().cpu()  # noqa: E731
    lns = [(cpu(g), cpu(b), e) for g, b, e in c.lns]
    cm = c.cm
    xa = cpu(c.x) + cpu(c.o) @ cpu(c.wo).T + cpu(c.bo)
    u = ln64(xa, cpu(cm.layer_norm.weight), cpu(cm.layer_norm.bias), cm.layer_norm.eps, deff)
    h = u @ _bf(cm.bottleneck[0].weight.reshape(2 * D, D)).T + cpu(cm.bottleneck[0].bias)
    g = (h[:, :D] * torch.sigmoid(h[:, D:])).reshape(B, T, D)
    padl = (K - 1) // 2
    gp = F.pad(g.transpose(1, 2), (padl, K - 1 - padl))  # zeros outside the utterance
    cv = F.conv1d(gp, _bf(cm.conv.weight), cpu(cm.conv.bias), groups=D).transpose(1, 2).reshape(B * T, D)
    ln1 = cm.after_conv[0]
    n = ln64(cv, cpu(ln1.weight), cpu(ln1.bias), ln1.eps, deff)
    v = (n * torch.sigmoid(n)) @ _bf(cm.after_conv[2].weight).T + cpu(cm.after_conv[2].bias)
    if kpm is not None:
        v = v.masked_fill(kpm.cpu().bool()[:, None], 0.0)
    xc = xa + v
    zp = ln64(_ffn64(c.fa, xc, lns[0], 0.5, deff), *lns[1], deff=deff)
    out = _ffn64(c.fb, zp, lns[2], 0.5, deff)
    y = ln64(out, *lns[3], deff=deff) @ cpu(c.wp).T
    return out, y, ln64(zp, *lns[3], deff=deff)


_REFS = {}


def _case(dev, B, T, K, masked, deff):
    """The inputs of test_gpu_conv_chain.py's cases, the key-padding mask of
    relative lengths (1.0, 0.6), and the float64 reference — built once."""
    key = (B, T, K, masked, deff)
    if key not in _REFS:
        from test_gpu_conv_chain import _Case
        c = _Case(dev, B, T, K, False, False, 512, deff=None if deff == D else deff)
        kpm = None
        if masked:
            lim = torch.floor(torch.tensor([1.0, 0.6]) * T)
            kpm = (torch.arange(T)[None].float() > lim[:, None]).to(torch.uint8).reshape(-1).to(dev)
        c.kpm = kpm
        with torch.no_grad():
            _REFS[key] = (c, _boundary64(c, B, T, K, kpm, deff))
    return _REFS[key]


SHAPES = [(2, 47, 31),   # one tile with a dead row
          (2, 50, 31),   # two tiles, the halo across their edge, a nearly empty second tile
          (2, 97, 31),   # a last tile of one row
          (2, 50, 15)]   # the other padL branch of the residual relocation
SENT, PADR = 777.0, 64


def _conv_args(c):
    ln0, w1p, b1p, wc, bc, causal, ln1, w2, b2 = c.cm.fused_params()
    return (c.o, c.wo, c.bo, ln0[0], ln0[1], ln0[2], w1p, b1p, wc, bc, causal, ln1[0], ln1[1], ln1[2], w2, b2, c.kpm)


@gpu
@pytest.mark.parametrize("deff", [256, 144])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,T,K", SHAPES)
def test_conv_ffn_chain_vs_float64(dev, B, T, K, masked, deff):
    from speechbrain_amd import _enc
    c, (ref_out, ref_y, _) = _case(dev, B, T, K, masked, deff)
    a, b = c.blocks()
    M = B * T
    out = torch.full((M + PADR, D), SENT, device=dev)
    y = torch.full((M + PADR, 768), SENT, device=dev, dtype=torch.bfloat16)
    gp, bp, ep = a[6]
    with torch.no_grad():
        _enc._conv_ffn_chain_into(out, y, c.x, B, T, *_conv_args(c), _enc.ACT["swish"], 0.0, a[0][0], a[0][1], a[0][2],
                                  a[1], a[2], a[3], a[4], a[5], gp, bp, ep, b[0][0], b[0][1], b[0][2], b[1], b[2], b[3],
                                  b[4], b[5], c.lns[3][0], c.lns[3][1], c.lns[3][2], c.wp, deff)
    # rows the launch does not own: untouched
    assert torch.equal(out[M:], torch.full_like(out[M:], SENT)) and torch.equal(y[M:], torch.full_like(y[M:], SENT))
    print(f"chain B {B} T {T} K {K} masked {masked} deff {deff}: out max err "
          f"{float((out[:M].double().cpu() - ref_out).abs().max()):.3e} (max |ref| {float(ref_out.abs().max()):.2f}), "
          f"y max err {float((y[:M].double().cpu() - ref_y).abs().max()):.3e} (max |ref| {float(ref_y.abs().max()):.2f})")
    assert_close(out[:M], ref_out.float(), rtol=2e-2, name="chain out")
    assert_close(y[:M].float(), ref_y.float(), rtol=2e-2, name="chain projection")
    if deff < D:
        assert torch.equal(out[:M, deff:], torch.zeros_like(out[:M, deff:]))


@gpu
@pytest.mark.parametrize("deff", [256, 144])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("B,T,K", SHAPES)
def test_conv_ffn_tail_vs_float64(dev, B, T, K, masked, deff):
    from speechbrain_amd import _enc
    c, (_, _, ref_u) = _case(dev, B, T, K, masked, deff)
    a, _ = c.blocks()
    M = B * T
    u = torch.full((M + PADR, D), SENT, device=dev)
    gp, bp, ep = a[6]
    with torch.no_grad():
        _enc._conv_ffn_tail_into(u, c.x, B, T, *_conv_args(c), _enc.ACT["swish"], 0.0, a[0][0], a[0][1], a[0][2], a[1],
                                 a[2], a[3], a[4], a[5], gp, bp, ep, c.lns[3][0], c.lns[3][1], c.lns[3][2], deff)
    assert torch.equal(u[M:], torch.full_like(u[M:], SENT))
    print(f"tail B {B} T {T} K {K} masked {masked} deff {deff}: u max err "
          f"{float((u[:M].double().cpu() - ref_u).abs().max()):.3e} (max |ref| {float(ref_u.abs().max()):.2f})")
    assert_close(u[:M], ref_u.float(), rtol=2e-2, name="tail u")
    if deff < D:
        assert torch.equal(u[:M, deff:], torch.zeros_like(u[:M, deff:]))


# ------------------------------------------------ register and scratch limits
SWISH_KERNELS = ["17conv_chain_kernelILi1EE", "16conv_tail_kernelILi1EE", "14src_ffn_kernelILi1EE",
                 "10ffn_kernelILi256ELi1ELb0ELb0EE", "10ffn_kernelILi256ELi1ELb0ELb1EE",
                 "10ffn_kernelILi256ELi1ELb1ELb0EE", "10ffn_kernelILi256ELi1ELb1ELb1EE"]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_swish_instances_keep_no_scratch(tmp_path):
    """gfx950 assembly of ffn.hip with the product flags (as
    test_asm_hazards.py obtains it); only the resource lines are read."""
    from speechbrain_amd import _build
    src = os.path.join(ROOT, "speechbrain_amd", "csrc", "ffn.hip")
    out = str(tmp_path / "ffn.s")
    flags = [f for f in _build.CFLAGS if f != "-fPIC"]
    cmd = [_build.HIPCC, *flags, "--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stderr[-2000:]}"
    res = {}
    name = None
    for line in open(out):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.match(r"\s*\.amdhsa_(private_segment_fixed_size|next_free_vgpr)\s+(\d+)", line)
        if m and name:
            res[name][m.group(1)] = int(m.group(2))
    for key in SWISH_KERNELS:
        hits = [n for n in res if key in n]
        assert len(hits) == 1, (key, hits)
        r = res[hits[0]]
        assert r["private_segment_fixed_size"] == 0, (hits[0], r)
        assert r["next_free_vgpr"] <= 256, (hits[0], r)
