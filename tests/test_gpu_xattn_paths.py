"""csrc/xattn.hip across its query-/key-blocked kernels, their 64-key chunk
loops and the per-row fallback kernels: the attention core driven directly
through _autograd.RelPosCrossAttnFn against a float64 CPU restatement of the
same algebra (core_ref below, anchored to oracle.conformer.rel_pos_mha_cross
by a CPU test), outputs, weights and every gradient.

Which kernel an id runs.  The host dispatch of xattn_fwd / xattn_bwd:

    pass                        blocked kernel when                      else
    forward                     Lk <= 1024, dh <= 128, dh % 4 == 0 and   xattn_fwd_kernel
      xattn_fwd_qb_kernel       q, k, v (+ pk) 4-element aligned
    backward row pass           Lk <= 1024 and k, v, dO aligned          xattn_bwd_rows_kernel
      xattn_bwd_rows_qb_kernel  (same dh rule)
    backward band-row pass      pk aligned (same dh rule)                xattn_bwd_qv_kernel
      xattn_bwd_qv_qb_kernel
    backward key-row pass       q, dO aligned (same dh rule)             xattn_bwd_kv_kernel
      xattn_bwd_kv_qb_kernel
    backward band-column pass   xattn_bwd_pk_kernel always               -

The last id component is the alignment of the operands.  A misaligned operand
is a contiguous view one element into a larger buffer: is_contiguous() holds,
so the autograd function hands it to the kernels as it is, and every pass
that stages it 4 elements at a time takes its fallback.

    none  everything aligned: every pass blocked (subject to the shape, below)
    q     q misaligned:  forward and key-row pass fall back; row pass and
          band-row pass stay blocked
    k     k misaligned:  forward and row pass fall back; band-row and key-row
          pass stay blocked
    pk    pk misaligned: forward and band-row pass fall back; row and key-row
          pass stay blocked
    all   q, k, v, pk and the gradient handed to backward misaligned: every
          pass falls back

The shape component overrides "blocked" where the table says so:
k1025 / k1030 (Lk > 1024) send the forward and the row pass to their fallbacks
at any alignment, the band-row and key-row passes stay blocked; d160 / d256
(dh > 128) and d30 (dh % 4 != 0) send every pass to its fallback.  Rel-pos ids
(q<Lq>_k<Lk>_d<dh>[_mpf]) use the band kernels, "nopos" ids run with
pk = None (no band passes).

Bounds are max |error| / max(1, max |reference|) per tensor, the convention
and the numbers of test_nopos_core_dropout_vs_autograd: fp32 1e-5 for
weights and out, 2e-5 for gradients (a float32 CPU evaluation of core_ref
stays within 6.6e-7 of float64 at these shapes, so a kernel that needs more
is wrong); bf16 operands are rounded first and the reference is fed the
rounded values, so only output rounding separates the two (weights 1e-4, out
1e-2, dq / dk / dv / dpk 2e-2, the fp32 dpbu / dpbv 2e-5)."""
import functools
import math
import zlib
from types import SimpleNamespace

import pytest
import torch

from conftest import assert_close
import oracle.conformer as OC

gpu = pytest.mark.gpu


def core_ref(q, k, v, pk, u, vb, kpm, am, B, Lq, Lk, H, dh, scale, mpf, D=None):
    """The attention core of RelPosMHAXL for separate q / k / v (attention.py:
    581-633 with the cross-length rel_shift) from plain torch ops: q (B*Lq, d),
    k / v (B*Lk, d), pk (P, d), u / vb the (dh, H) biases read as (H, dh), kpm
    (B, Lk) bool, am additive and broadcastable to (B, H, Lq, Lk) or None, D a
    dropout scale (keep / (1 - p)) on the probabilities.  pk None: plain scaled
    dot-product attention.  Returns (out (B*Lq, d), weights (B, H, Lq, Lk))."""
    q4, k4, v4 = q.view(B, Lq, H, dh), k.view(B, Lk, H, dh), v.view(B, Lk, H, dh)
    if pk is None:
        score = torch.einsum("bihd,bjhd->bhij", q4, k4)
    else:
        P = pk.shape[0]
        ac = torch.einsum("bihd,bjhd->bhij", q4 + u, k4)
        bd = OC.rel_shift_cross(torch.einsum("bihd,whd->bhiw", q4 + vb, pk.view(P, H, dh)), mpf)
        score = ac + bd
    score = score * scale
    if am is not None:
        score = score + am
    if kpm is not None:
        score = score.masked_fill(kpm.view(B, 1, 1, Lk), -float("inf"))
    attn = torch.softmax(score, -1)
    if D is not None:
        attn = attn * D
    return torch.einsum("bhij,bjhd->bihd", attn, v4).reshape(B * Lq, H * dh), attn


def test_core_ref_matches_oracle(golden):
    """core_ref on the oracle's own projections, through out_proj, is
    oracle.conformer.rel_pos_mha_cross (pinned to the reference's outputs by
    test_oracle_golden) in float64 to 1e-12, on the multi-head fixture cases."""
    F = torch.nn.functional
    g = golden("xattn")
    for t in ("c0", "c1", "c2", "c3", "c4", "c5"):
        E, H, vbias, Lq, Lk, same_kv, mpf, has_kpm, am_kind = (int(x) for x in g[f"{t}.meta"])
        pre = f"{t}.sd."
        sd = {n[len(pre):]: torch.from_numpy(g[n]).double() for n in g.files if n.startswith(pre)}
        query, key = torch.from_numpy(g[f"{t}.q"]).double(), torch.from_numpy(g[f"{t}.k"]).double()
        value = key if same_kv else torch.from_numpy(g[f"{t}.v"]).double()
        pe = torch.from_numpy(g[f"{t}.pe"]).double()
        kpm = torch.from_numpy(g[f"{t}.kpm"]) if has_kpm else None
        am = torch.from_numpy(g[f"{t}.am"]) if am_kind else None
        ro, ra = OC.rel_pos_mha_cross(query, key, value, pe, sd, "", H, bool(vbias), bool(mpf), kpm, am)
        B, dh = query.shape[0], E // H
        wq, wk, wv = sd["in_proj_weight"].chunk(3, dim=0)
        q = F.linear(query, wq).reshape(B * Lq, E)
        k = F.linear(key, wk).reshape(B * Lk, E)
        v = F.linear(value, wv)
        if vbias:
            v = v + sd["value_bias_weight"].view(1, 1, E)
        pk = F.linear(pe, sd["linear_pos.weight"]).reshape(-1, E)
        add = None
        if am is not None:
            add = am.view(1, 1, Lq, Lk) if am.ndim == 2 else am.view(-1, H, Lq, Lk)
            if add.dtype == torch.bool:
                add = torch.zeros(add.shape, dtype=torch.float64).masked_fill(add, -float("inf"))
            else:
                add = add.double()
        o, a = core_ref(q, k, v.reshape(B * Lk, E), pk, sd["pos_bias_u"].reshape(H, dh),
                        sd["pos_bias_v"].reshape(H, dh), None if kpm is None else kpm.bool(), add, B, Lq, Lk, H, dh,
                        1.0 / math.sqrt(E), bool(mpf))
        out = F.linear(o, sd["out_proj.weight"], sd["out_proj.bias"]).view(B, Lq, E)
        assert torch.isfinite(ro).all() and torch.isfinite(ra).all(), t
        assert float((out - ro).abs().max()) <= 1e-12, t
        assert float((a - ra).abs().max()) <= 1e-12, t


# (B, Lq, Lk, H, dh, mask_pos_future): each shape sits on a boundary of the
# 16-row query blocks / 64-key chunks or of the host dispatch
RELPOS = {
    "q16_k64_d16": (2, 16, 64, 2, 16, False),          # exactly one query block, one chunk
    "q17_k65_d16_mpf": (2, 17, 65, 2, 16, True),       # one past both
    "q33_k129_d16_mpf": (2, 33, 129, 4, 16, True),     # three blocks, three chunks, ragged by one
    "q50_k200_d36": (2, 50, 200, 2, 36, False),        # dh % 8 == 4: the LDS row pad in the output dims
    "q150_k70_d32": (2, 150, 70, 2, 32, False),        # q_len > k_len: wrap rows over ten blocks, two chunks
    # mask_pos_future zeroes exactly the wrap elements (both are j - i > P - q_len), so this one checks
    # that nothing of them leaks, and the next one the wrap rows themselves up to r = i + 4
    "q150_k20_d32_mpf": (2, 150, 20, 2, 32, True),
    "q150_k20_d32": (2, 150, 20, 2, 32, False),
    # q_len < k_len with the last of four 64-column band chunks still in use (columns reach
    # q_len + k_len - 2 = 195 of 199; for q_len << k_len the upper band chunks hold only zeros), and two
    # 64-row query chunks in the key-blocked pass
    "q97_k100_d16": (2, 97, 100, 2, 16, False),
    "q20_k1024_d128": (1, 20, 1024, 1, 128, False),    # Lk == XQ_LKMAX, dh == XQ_DMAX: the 158,464-byte launch
    "q17_k1025_d64_mpf": (1, 17, 1025, 2, 64, True),   # Lk > XQ_LKMAX: forward and row pass fall back
    "q40_k100_d160": (2, 40, 100, 1, 160, False),      # dh > XQ_DMAX: every pass falls back
    "q40_k100_d30": (2, 40, 100, 2, 30, False),        # dh % 4 != 0: every pass falls back
}
# the cases that also run with every misalignment (the third has wrap rows)
RELPOS_ALIGNED = ("q33_k129_d16_mpf", "q50_k200_d36", "q150_k70_d32")
# (B, Lq, Lk, H, dh), pk = None
NOPOS = {
    "q37_k150_d64": (2, 37, 150, 2, 64),
    "q20_k1030_d64": (1, 20, 1030, 1, 64),
    "q33_k129_d256": (2, 33, 129, 1, 256),
}
ALIGN = {"none": (), "q": ("q",), "k": ("k",), "pk": ("pk",), "all": ("q", "k", "v", "pk", "do")}
TOL = {
    "fp32": dict(attn=1e-5, out=1e-5, dq=2e-5, dk=2e-5, dv=2e-5, dpk=2e-5, dpbu=2e-5, dpbv=2e-5),
    "bf16": dict(attn=1e-4, out=1e-2, dq=2e-2, dk=2e-2, dv=2e-2, dpk=2e-2, dpbu=2e-5, dpbv=2e-5),
}
DTYPE = {"fp32": torch.float32, "bf16": torch.bfloat16}


@functools.lru_cache(maxsize=None)
def _case(name, dt):
    """Seeded CPU inputs of a case (float32 values, rounded to bf16 for dt ==
    "bf16"), shared by every alignment of it."""
    pos = name in RELPOS
    B, Lq, Lk, H, dh, mpf = RELPOS[name] if pos else NOPOS[name] + (False,)
    d = H * dh
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    rnd = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    c = SimpleNamespace(name=name, dt=dt, pos=pos, B=B, Lq=Lq, Lk=Lk, H=H, dh=dh, mpf=mpf, scale=1 / math.sqrt(d))
    c.q, c.k, c.v = rnd(B * Lq, d), rnd(B * Lk, d), rnd(B * Lk, d)
    c.pk = rnd(2 * Lk - 1, d) if pos else None
    c.pbu = 0.3 * rnd(dh, H) if pos else None
    c.pbv = 0.3 * rnd(dh, H) if pos else None
    c.am = 0.5 * rnd(B, H, Lq, Lk)
    c.R = rnd(B * Lq, d)
    # batch 0 full, the others padded by more than one key chunk where Lk allows
    c.kpm = torch.zeros(B, Lk, dtype=torch.bool)
    c.kpm[1:, Lk - min(70, Lk - 1):] = True
    if dt == "bf16":
        for n in ("q", "k", "v", "pk", "R"):
            setattr(c, n, getattr(c, n).to(torch.bfloat16).float())
    return c


def _ref(c, D=None):
    """Float64 core_ref and autograd of sum(R * out) for a case: weights, out
    and the gradients (dpbu / dpbv in the (dh, H) parameter shape)."""
    leaves = {n: getattr(c, n).double().requires_grad_(True) for n in ("q", "k", "v")}
    if c.pos:
        leaves.update({n: getattr(c, n).double().requires_grad_(True) for n in ("pk", "pbu", "pbv")})
    u = leaves["pbu"].reshape(c.H, c.dh) if c.pos else None
    vb = leaves["pbv"].reshape(c.H, c.dh) if c.pos else None
    out, attn = core_ref(leaves["q"], leaves["k"], leaves["v"], leaves.get("pk"), u, vb, c.kpm, c.am.double(), c.B,
                         c.Lq, c.Lk, c.H, c.dh, c.scale, c.mpf, D)
    (out * c.R.double()).sum().backward()
    r = {"attn": attn.detach(), "out": out.detach()}
    r.update({"d" + n: t.grad for n, t in leaves.items()})
    for n, t in r.items():
        assert torch.isfinite(t).all(), (c.name, n)
    return r


@functools.lru_cache(maxsize=None)
def _ref0(name, dt):
    return _ref(_case(name, dt))


def _place(t, dev, dtype, misaligned):
    """t on the device, contiguous, its pointer aligned to 4 elements or one
    element past such an alignment."""
    base = torch.empty(t.numel() + int(misaligned), device=dev, dtype=dtype)
    x = (base[1:] if misaligned else base).view(t.shape)
    x.copy_(t)
    assert x.is_contiguous() and (x.data_ptr() % (4 * x.element_size()) != 0) == bool(misaligned)
    return x


@functools.lru_cache(maxsize=None)
def _run(dev, name, dt, align, p=0.0, seed=None):
    """One forward + backward of the HIP core; the results on the CPU in
    float64 (cached: the aligned run is shared with the fallback checks)."""
    from speechbrain_amd import _autograd as A
    from speechbrain_amd import _enc
    c, mis, dtype = _case(name, dt), ALIGN[align], DTYPE[dt]
    q, k, v = (_place(getattr(c, n), dev, dtype, n in mis).requires_grad_(True) for n in ("q", "k", "v"))
    pk = pbu = pbv = None
    if c.pos:
        pk = _place(c.pk, dev, dtype, "pk" in mis).requires_grad_(True)
        pbu, pbv = c.pbu.to(dev).requires_grad_(True), c.pbv.to(dev).requires_grad_(True)
    am = _enc.attn_mask_arg(c.am.to(dev), c.B, c.Lq, c.H, dev, Lk=c.Lk)
    if seed is not None:
        torch.manual_seed(seed)
    o, attn = A.RelPosCrossAttnFn.apply(q, k, v, pk, pbu, pbv, c.kpm.to(dev).to(torch.uint8), am, c.B, c.Lq, c.Lk,
                                        c.H, c.dh, c.scale, c.mpf, p)
    got = {"attn": attn.detach().double().cpu(), "out": o.detach().double().cpu()}
    R = _place(c.R, dev, dtype, "do" in mis)
    seen = []
    o.register_hook(lambda gr: seen.append(gr.data_ptr()))
    o.backward(R)
    assert seen == [R.data_ptr()]  # backward was handed R itself, (mis)aligned as built
    leaves = dict(dq=q, dk=k, dv=v, dpk=pk, dpbu=pbu, dpbv=pbv)
    got.update({n: t.grad.double().cpu() for n, t in leaves.items() if t is not None})
    assert o.dtype == dtype and q.grad.dtype == dtype
    if c.pos:
        assert pbu.grad.shape == (c.dh, c.H) and pbv.grad.shape == (c.dh, c.H) and pbu.grad.dtype == torch.float32
    return got


def _compare(tag, got, ref, tol):
    """Every tensor of ref against got at tol[name] of max(1, max |ref|);
    prints each error / bound ratio, then asserts all of them."""
    bad = []
    for n, r in ref.items():
        assert got[n].shape == r.shape, (tag, n, got[n].shape, r.shape)
        err = float((got[n] - r).abs().max()) / max(1.0, float(r.abs().max()))
        print(f"xattn_paths {tag} {n}: err {err:.3e} bound {tol[n]:.0e} ratio {err / tol[n]:.3f}")
        if not err <= tol[n]:
            bad.append((n, err, tol[n]))
    assert not bad, (tag, bad)


def _check(dev, name, dt, align):
    got = _run(dev, name, dt, align)
    _compare(f"{name}-{dt}-{align} vs float64", got, _ref0(name, dt), TOL[dt])
    if align != "none":  # a reference mistake that fits both kernels would pass the line above
        _compare(f"{name}-{dt}-{align} vs aligned run", got, _run(dev, name, dt, "none"), TOL[dt])


@gpu
@pytest.mark.parametrize("name,align", [(n, "none") for n in RELPOS] +
                         [(n, a) for n in RELPOS_ALIGNED for a in ("q", "k", "pk", "all")])
def test_relpos_core_fp32(dev, name, align):
    """Weights, out and dq / dk / dv / dpk / dpbu / dpbv of the rel-pos core
    against float64; the runs with a misaligned operand also against the
    aligned run of the same inputs."""
    _check(dev, name, "fp32", align)


@gpu
@pytest.mark.parametrize("name,align", [("q37_k150_d64", "all"), ("q20_k1030_d64", "none"),
                                        ("q33_k129_d256", "none")])
def test_nopos_core_fp32(dev, name, align):
    """The no-position core (pk = None) on its fallback kernels beyond one
    key chunk: misaligned operands, Lk > 1024, and the widest head (256)."""
    _check(dev, name, "fp32", align)


@gpu
@pytest.mark.parametrize("name", ["q33_k129_d16_mpf", "q150_k70_d32"])
@pytest.mark.parametrize("align", ["none", "all"])
def test_relpos_core_bf16(dev, name, align):
    """bf16 operands (rounded first; the reference sees the rounded values):
    fp32 weights at 1e-4, bf16 out at 1e-2, bf16 gradients at 2e-2 and the
    fp32 bias gradients at the fp32 bound."""
    _check(dev, name, "bf16", align)


@gpu
def test_relpos_core_dropout(dev):
    """Attention dropout on the rel-pos path over three key chunks, blocked
    and fallback kernels under one seed: the returned weights are
    P · keep / (1 - p), every gradient equals autograd under that mask (read
    off the weights), the dropped fraction is p, and both sets of kernels
    draw the same mask (a function of seed and element index)."""
    name, p = "q33_k129_d16_mpf", 0.25
    c = _case(name, "fp32")
    live = (~c.kpm).view(c.B, 1, 1, c.Lk).expand(c.B, c.H, c.Lq, c.Lk)
    keeps = {}
    for align in ("none", "all"):
        got = _run(dev, name, "fp32", align, p, 77)
        keep = got["attn"] != 0
        keeps[align] = keep
        assert float(_ref0(name, "fp32")["attn"][live].min()) > 1e-30  # no live probability underflows to 0
        frac = 1.0 - float(keep[live].double().mean())
        print(f"xattn_paths {name}-dropout-{align}: dropped fraction {frac:.4f}")
        assert abs(frac - p) <= 0.03, (align, frac)
        _compare(f"{name}-dropout-{align} vs float64", got, _ref(c, keep.double() / (1 - p)), TOL["fp32"])
    assert torch.equal(keeps["none"][live], keeps["all"][live])


@gpu
def test_relpos_cross_module_multi_chunk(dev):
    """RelPosMHAXL with key != value over three query blocks and three key
    chunks (beyond what tests/golden/xattn.npz reaches) against
    oracle.conformer.rel_pos_mha_cross in float64 on the module's weights:
    output, weights, input and parameter gradients at 1e-4."""
    from speechbrain_amd.nnet.attention import RelPosMHAXL
    torch.manual_seed(11)
    E, H, B, Lq, Lk = 64, 4, 2, 33, 129
    m = RelPosMHAXL(E, num_heads=H, vbias=True, mask_pos_future=True).to(dev)
    with torch.no_grad():
        m.value_bias_weight.normal_()
    q = torch.randn(B, Lq, E, device=dev, requires_grad=True)
    k = torch.randn(B, Lk, E, device=dev, requires_grad=True)
    v = torch.randn(B, Lk, E, device=dev, requires_grad=True)
    pe = torch.randn(1, 2 * Lk - 1, E, device=dev)
    kpm = torch.zeros(B, Lk, dtype=torch.bool, device=dev)
    kpm[1, Lk - 70:] = True
    o, attn = m(q, k, v, pos_embs=pe, key_padding_mask=kpm)
    R = torch.randn_like(o)
    (o * R).sum().backward()
    sd = {n: t.detach().cpu().double().requires_grad_(True) for n, t in m.state_dict().items()}
    q2, k2, v2 = (t.detach().cpu().double().requires_grad_(True) for t in (q, k, v))
    o2, a2 = OC.rel_pos_mha_cross(q2, k2, v2, pe.cpu().double(), sd, "", H, True, True, kpm.cpu())
    assert torch.isfinite(o2).all()
    (o2 * R.cpu().double()).sum().backward()
    assert_close(o, o2, name="out")
    assert_close(attn, a2, name="weights")
    assert_close(q.grad, q2.grad, name="grad q")
    assert_close(k.grad, k2.grad, name="grad k")
    assert_close(v.grad, v2.grad, name="grad v")
    names = [n for n, _ in m.named_parameters()]
    assert names
    for n, prm in m.named_parameters():
        assert_close(prm.grad, sd[n].grad, name=f"grad {n}")
