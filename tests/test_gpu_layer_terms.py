"""The fused layer launches (csrc/ffn.hip ffn_kernel, conv_chain_kernel,
conv_tail_kernel, src_ffn_kernel; csrc/convstage.h) term by term, through the
C ABI into sentinel-padded buffers:

* exact probes (test_exact_*): inputs of layer_ref.probe_case, for which no
  rounding point rounds and the stage before the first further LayerNorm is
  known in closed form (layer_ref.probe_expected).  One launch per hidden chunk
  k, the second GEMM one-hot on that chunk.  `out` of sbk_ffn / sbk_ffn_proj:
  torch.equal.  Outputs behind a further LayerNorm against float64 LayerNorm
  of the exact stage: fp32 at 1e-4 of the largest reference value
  (test_row_ln_alone's bound), bf16 at 2^-8 |ref| + 1e-5
  (test_projection_column_placement_exact's bound).  ACT_NONE, and ACT_LRELU
  with slope 0.5 (a negative hidden value halves exactly).
* reference cases (test_reference): layer_ref.ref_cases() against
  layer_ref.reference (float64 on the kernels' rounding points) at
  layer_ref.bound: fp32 outputs per tensor max|err| / max(1, max|ref|) <=
  max(1e-5, 8 E32), bf16 outputs elementwise |err| <= 2^-8 |ref| + that bound
  times max(1, max|ref|).  No bound comes from a kernel run.
* negative controls (test_negative_control): the launch with a term zeroed
  against the reference that keeps it must be rejected by the same helper.
* limits (test_limits): the largest H by ffn_lds (154368 + 4 H per block of
  b1 <= 160 KiB) and sbk_ffn_supported (H <= 2048).

The instantiation behind every id: layer_ref.instantiation (table in
layer_ref's docstring); test_layer_ref_cpu.py::test_every_instantiation_is_launched
counts the 28.  Observed deviations on the MI355X: DESIGN.md section 7."""
import pytest
import torch

import layer_ref as R

pytestmark = pytest.mark.gpu

D = R.D
SENT, PADR = 777.0, 64
SBK_ERR_ARG = 1001


# --------------------------------------------------------------- the launches
def glu_perm():
    """Rows of the conv stage's pointwise weight in the kernels' order: groups of
    16 value rows followed by their 16 gate rows (ConvolutionModule.kernel_weights)."""
    idx = []
    for q in range(D // 16):
        idx += list(range(q * 16, (q + 1) * 16)) + list(range(D + q * 16, D + (q + 1) * 16))
    return torch.tensor(idx)


def launch(c, dev):
    """Case c through its C entry point into buffers of M + PADR rows filled
    with a sentinel.  Returns (rc, {name: rows [:M]}, every buffer untouched
    past row M, every buffer untouched altogether)."""
    from speechbrain_amd import _enc
    from speechbrain_amd._enc import lib, ptr, stream_of
    assert _enc.glu_group() == 16
    to = lambda t: None if t is None else t.to(dev).contiguous()  # noqa: E731
    M, H, NP, deff = c["M"], c["H"], c["np"], c["deff"]
    act, slope = _enc.ACT[R.ACT_ABI[c["act"]]], float(c["slope"])
    A, B = c["A"], c.get("B")
    w1, b1, w2, b2 = to(A["w1"]), to(A["b1"]), to(A["w2"]), to(A["b2"])
    g0, b0, e0 = to(A["ln0"][0]), to(A["ln0"][1]), float(A["ln0"][2])
    gp, bp, ep = (to(A["post_ln"][0]), to(A["post_ln"][1]), float(A["post_ln"][2])) if A.get("post_ln") else (None, None, 0.0)
    gn, bn, en = (to(c["next_ln"][0]), to(c["next_ln"][1]), float(c["next_ln"][2])) if c.get("next_ln") else (None, None, 0.0)
    w1b = b1b = w2b = b2b = g0b = b0b = None
    e0b, alphab = 0.0, 0.0
    if B is not None:
        w1b, b1b, w2b, b2b = to(B["w1"]), to(B["b1"]), to(B["w2"]), to(B["b2"])
        g0b, b0b, e0b, alphab = to(B["ln0"][0]), to(B["ln0"][1]), float(B["ln0"][2]), float(B["alpha"])
    wp = to(c.get("wp"))
    img = _enc.ffn_image(w1, w2, w1b, w2b, wp)
    bufs = {}
    if c["launch"] != "conv_ffn_tail":
        bufs["out"] = torch.full((M + PADR, D), SENT, device=dev)
    if NP:
        bufs["yp"] = torch.full((M + PADR, NP), SENT, device=dev, dtype=torch.bfloat16)
    elif gn is not None:
        bufs["u"] = torch.full((M + PADR, D), SENT, device=dev, dtype=torch.bfloat16 if c["u_bf16"] else torch.float32)
    out, yp, u = bufs.get("out"), bufs.get("yp"), bufs.get("u")
    alpha = float(A["alpha"])
    L = c["launch"]
    if L in ("ffn", "ffn_proj"):
        x = to(c["x"])
        if L == "ffn":
            rc = lib().sbk_ffn(ptr(x), M, D, deff, H, ptr(g0), ptr(b0), e0, ptr(img), img.numel(), ptr(b1), act, slope,
                               ptr(b2), alpha, ptr(gp), ptr(bp), ep, ptr(out), ptr(gn), ptr(bn), en, ptr(u),
                               int(c["u_bf16"]), stream_of(x))
        else:
            rc = lib().sbk_ffn_proj(ptr(x), M, D, deff, H, ptr(g0), ptr(b0), e0, ptr(img), img.numel(), ptr(b1), act, slope,
                                    ptr(b2), alpha, ptr(gp), ptr(bp), ep, ptr(out), ptr(gn), ptr(bn), en, None, 1, NP,
                                    ptr(yp), stream_of(x))
    elif L == "ffn_chain":
        x = to(c["x"])
        rc = lib().sbk_ffn_chain(ptr(x), M, D, deff, H, act, slope, ptr(g0), ptr(b0), e0, ptr(b1), ptr(b2), alpha, ptr(gp),
                                 ptr(bp), ep, ptr(g0b), ptr(b0b), e0b, ptr(b1b), ptr(b2b), alphab, ptr(out), ptr(gn), ptr(bn),
                                 en, ptr(u), int(c["u_bf16"]) if u is not None else 1, ptr(img), img.numel(), NP, ptr(yp),
                                 stream_of(x))
    elif L == "src_ffn_proj":
        s = c["src"]
        a, ws, bs, rel = to(s["a"]), to(s["ws"]), to(s["sbias"]), to(s["rel_len"])
        simg = _enc.src_image(ws)
        if rel is not None:
            bufs["kpm_out"] = torch.full((M + PADR,), 7, device=dev, dtype=torch.uint8)
        rc = lib().sbk_src_ffn_proj(ptr(a), c["Kin"], ptr(simg), simg.numel(), ptr(bs), ptr(rel), int(s["T"]),
                                    ptr(bufs.get("kpm_out")), M, D, deff, H, ptr(g0), ptr(b0), e0, ptr(img), img.numel(),
                                    ptr(b1), act, slope, ptr(b2), alpha, ptr(gp), ptr(bp), ep, ptr(out), ptr(gn), ptr(bn),
                                    en, NP, ptr(yp), stream_of(a))
    else:
        cv = c["conv"]
        x, o, wo, bo = to(c["x"]), to(cv["o"]), to(cv["wo"]), to(cv["bo"])
        perm = glu_perm()
        w1p, b1p = to(cv["w1"][perm]), to(cv["b1"][perm])
        wc, bc, cw2, cb2, kpm = to(cv["taps"]), to(cv["bc"]), to(cv["w2"]), to(cv["b2"]), to(cv["kpm"])
        cg0, cb0, ce0 = to(cv["ln0"][0]), to(cv["ln0"][1]), float(cv["ln0"][2])
        cg1, cb1, ce1 = to(cv["ln1"][0]), to(cv["ln1"][1]), float(cv["ln1"][2])
        cimg, woimg, dwimg = _enc.conv_image(w1p, cw2), _enc.wo_image(wo), _enc.dw_image(wc, bc)
        head = (ptr(x), ptr(o), ptr(woimg), ptr(bo), cv["B"], cv["T"], D, deff, ptr(cg0), ptr(cb0), ce0, ptr(cimg),
                cimg.numel(), ptr(b1p), ptr(dwimg), None, cv["K"], int(cv["causal"]), ptr(cg1), ptr(cb1), ce1, ptr(cb2),
                ptr(kpm), H, act, slope, ptr(g0), ptr(b0), e0, ptr(b1), ptr(b2), alpha, ptr(gp), ptr(bp), ep)
        if L == "conv_ffn_chain":
            rc = lib().sbk_conv_ffn_chain(*head, ptr(g0b), ptr(b0b), e0b, ptr(b1b), ptr(b2b), alphab, ptr(out), ptr(gn),
                                          ptr(bn), en, ptr(img), img.numel(), NP, ptr(yp), stream_of(x))
        else:
            rc = lib().sbk_conv_ffn_tail(*head, ptr(gn), ptr(bn), en, ptr(u), ptr(img), img.numel(), stream_of(x))
    torch.cuda.synchronize()
    sent = {k: (7 if k == "kpm_out" else SENT) for k in bufs}
    pad_ok = all(bool((v[M:] == sent[k]).all()) for k, v in bufs.items())
    untouched = all(bool((v == sent[k]).all()) for k, v in bufs.items())
    return rc, {k: v[:M] for k, v in bufs.items()}, pad_ok, untouched


def check_reference(c, got, ref, verbose=True):
    """The worst excess over the bound (<= 1 passes) of got against ref."""
    worst = 0.0
    for name, r in ref.items():
        if name == "kpm_out":
            worst = max(worst, 0.0 if torch.equal(got[name].cpu(), r) else float("inf"))
            continue
        bnd = R.bound(c, name)
        ex, dev_ = R.excess(got[name], r, bnd, name in R.bf16_out(c))
        if verbose:
            print(f"{c['id']} {name}: deviation {dev_:.3e} (max |ref| {float(r.abs().max()):.3f}), bound {bnd:.3e}"
                  f"{' + 2^-8 |ref|' if name in R.bf16_out(c) else ''}, {ex:.3f} of it")
        worst = max(worst, ex)
    return worst


# ------------------------------------------------------------ reference cases
@pytest.mark.parametrize("c", R.ref_cases(), ids=lambda c: c["id"])
def test_reference(dev, c):
    ref = R.cached_reference(c)
    rc, got, pad_ok, _ = launch(c, dev)
    assert rc == 0
    assert pad_ok, "rows past M written"
    assert set(got) == set(ref)
    worst = check_reference(c, got, ref)
    assert worst <= 1.0, f"{c['id']}: {worst:.3f} of the bound"
    if c["deff"] < D:  # zero-padded channels stay zero
        for name in ("out", "u"):
            if name in got:
                assert float(got[name][:, c["deff"]:].float().abs().max()) == 0.0, name
    if "kpm_out" in got:
        from speechbrain_amd import _enc
        s = c["src"]
        assert torch.equal(got["kpm_out"], _enc.length_mask(s["rel_len"].to(dev), s["T"]).reshape(-1))


# ----------------------------------------------------------- negative controls
def _zeroed(c, term):
    c2, kw = R.altered(c, term)
    assert not kw
    if term == "conv.bc":  # the kernel takes a null conv bias as zeros; pass zeros all the same
        c2["conv"]["bc"] = torch.zeros(D)
    return c2


NEG = [("ffn_chain-swish-H1024-np768-d144-M97", "A.b1"), ("ffn_chain-swish-H1024-np768-d144-M97", "B.b2"),
       ("conv_ffn_chain-swish-H1024-np768-d256-B2T97K31m", "conv.bc"), ("conv_ffn_tail-swish-H1024-np0-d256-B2T97K31m", "conv.bc"),
       ("ffn-swish-H1024-np0-d144-M49-ubf", "A.b1"), ("conv_ffn_chain-swish-H1024-np768-d256-B2T97K31m", "B.b2")]


@pytest.mark.parametrize("cid,term", NEG)
def test_negative_control(dev, cid, term):
    """The kernel runs with the term zeroed, the reference keeps it: the
    comparison of test_reference must reject the result (and accept the
    launch of the unchanged case, which test_reference checks)."""
    c = next(x for x in R.ref_cases() if x["id"] == cid)
    rc, got, pad_ok, _ = launch(_zeroed(c, term), dev)
    assert rc == 0 and pad_ok
    worst = check_reference(c, got, R.cached_reference(c))
    print(f"{cid} without {term}: {worst:.1f} of the bound")
    assert worst > 1.0


# ---------------------------------------------------------------- exact probes
def check_probe(c, dev):
    exp, exact = R.probe_expected(c)
    rc, got, pad_ok, _ = launch(c, dev)
    assert rc == 0, c["id"]
    assert pad_ok, f"{c['id']}: rows past M written"
    assert set(got) == set(exp), c["id"]
    for name, r in exp.items():
        g = got[name].cpu()
        if name == "kpm_out":
            assert torch.equal(g, r), f"{c['id']} kpm_out"
        elif name in exact:
            bad = (g.double() != r)
            assert not bool(bad.any()), (f"{c['id']} {name}: {int(bad.sum())} elements differ, first at "
                                         f"{bad.nonzero()[0].tolist()}: {float(g[tuple(bad.nonzero()[0])])} != "
                                         f"{float(r[tuple(bad.nonzero()[0])])}")
        elif g.dtype == torch.bfloat16:
            err = (g.double() - r).abs()
            assert bool((err <= 2.0 ** -8 * r.abs() + 1e-5).all()), f"{c['id']} {name}: max err {float(err.max()):.3e}"
        else:
            err, big = float((g.double() - r).abs().max()), float(r.abs().max())
            assert err <= 1e-4 * big, f"{c['id']} {name}: {err:.3e} > 1e-4 * {big:.3e}"
    return got


def single_probes(launch_, act, H):
    return [R.probe_case(launch_, act, H, k, M=M, np_=256 if launch_ == "ffn_proj" else 0, u_bf16=bool(k % 2))
            for M in (1, 47, 48, 49, 97) for k in range(H // 256)]


def chain_probes(act, H, np_):
    return [R.probe_case("ffn_chain", act, H, k, M=M, np_=np_, which=which, u_bf16=bool(k % 2))
            for M in (49, 97) for which in ("A", "B") for k in range(H // 256)]


def conv_probes(launch_, act, H):
    return [R.probe_case(launch_, act, H, k, B=2, T=T, np_=256 if launch_ == "conv_ffn_chain" else 0, which=which)
            for T in (47, 49, 97) for which in (("A", "B") if launch_ == "conv_ffn_chain" else ("A",))
            for k in range(H // 256)]


def src_probes(act, Kin, rel, H=512):
    return [R.probe_case("src_ffn_proj", act, H, k, M=50 if Kin == 64 else 98, np_=256, Kin=Kin, rel=rel)
            for k in range(H // 256)]


SINGLE = [(l, a, H) for l in ("ffn", "ffn_proj") for a in ("none", "lrelu") for H in (256, 768, 1024, 2048)]
CHAIN = [(a, H, n) for a in ("none", "lrelu") for H in (256, 768, 1024) for n in (256, 0)]
CONV = [(l, a, H) for l in ("conv_ffn_chain", "conv_ffn_tail") for a in ("none", "lrelu") for H in (256, 1024)]
SRC = [(a, K, r) for a in ("none", "lrelu") for K in (64, 256, 768) for r in (False, True)]


def all_probes():
    """Every probe case of this module (test_layer_ref_cpu.py reads them)."""
    for p in SINGLE:
        yield from single_probes(*p)
    for p in CHAIN:
        yield from chain_probes(*p)
    for p in CONV:
        yield from conv_probes(*p)
    for p in SRC:
        yield from src_probes(*p)


@pytest.mark.parametrize("launch_,act,H", SINGLE)
def test_exact_single(dev, launch_, act, H):
    for c in single_probes(launch_, act, H):
        check_probe(c, dev)


@pytest.mark.parametrize("act,H,np_", CHAIN)
def test_exact_chain(dev, act, H, np_):
    for c in chain_probes(act, H, np_):
        check_probe(c, dev)


@pytest.mark.parametrize("launch_,act,H", CONV)
def test_exact_conv(dev, launch_, act, H):
    for c in conv_probes(launch_, act, H):
        check_probe(c, dev)


@pytest.mark.parametrize("act,Kin,rel", SRC)
def test_exact_src(dev, act, Kin, rel):
    for c in src_probes(act, Kin, rel):
        got = check_probe(c, dev)
        if rel:  # bit for bit what sbk_length_mask writes
            from speechbrain_amd import _enc
            s = c["src"]
            assert torch.equal(got["kpm_out"], _enc.length_mask(s["rel_len"].to(dev), s["T"]).reshape(-1))


# ---------------------------------------------------------------------- limits
def lds_bytes(H, blocks):
    """ffn_lds of csrc/ffn.hip: the 2-slot ring, Xn and two hidden buffers
    (bf16), the row-reduction scratch and the 8 parameter rows, and b1 per block."""
    return (2 * 256 * 64 + 48 * (256 + 16) + 2 * 48 * (256 + 16)) * 2 + 12 * 48 * 4 + 8 * 256 * 4 + blocks * H * 4


def largest_h(blocks):
    return max(h for h in range(256, 2048 + 1, 256) if lds_bytes(h, blocks) <= 160 * 1024)


def test_limits(dev):
    from speechbrain_amd._enc import lib
    assert lds_bytes(0, 1) == 154368
    assert largest_h(1) == 2048 and largest_h(2) == 1024
    assert lib().sbk_ffn_supported(256, 2048) == 1 and lib().sbk_ffn_supported(256, 2304) == 0
    # H = 1024 runs: the families' own reference cases (their bound is derived on their inputs)
    for cid, name, kw in (("ffn_chain-swish-H1024-np768-d144-M97", "ffn_chain", dict(M=49)),
                          ("conv_ffn_chain-swish-H1024-np768-d256-B2T97K31m", "conv_ffn_chain", dict(B=2, T=49))):
        ok = next(x for x in R.ref_cases() if x["id"] == cid)
        assert ok["H"] == largest_h(2)
        rc, got, pad_ok, untouched = launch(ok, dev)
        assert rc == 0 and pad_ok and not untouched
        assert check_reference(ok, got, R.cached_reference(ok)) <= 1.0
        over = R.make_case(name, "swish", largest_h(2) + 256, 256, **kw)  # refused: no bound needed
        rc, _, _, untouched = launch(over, dev)
        assert rc == SBK_ERR_ARG, (name, rc)
        assert untouched, f"{name}: a refused launch wrote its outputs"
