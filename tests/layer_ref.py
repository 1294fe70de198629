"""float64 restatement of the fused layer launches (csrc/ffn.hip: ffn_kernel,
conv_chain_kernel, conv_tail_kernel, src_ffn_kernel; csrc/convstage.h) on the
kernels' rounding points, with the inputs, the exact probes, the E32 table and
the bounds of test_gpu_layer_terms.py (test infrastructure, CPU only;
test_layer_ref_cpu.py pins it to the other restatements).

    rows   x                                   sbk_ffn / sbk_ffn_proj / sbk_ffn_chain
           a . Ws^T + sbias                    sbk_src_ffn_proj (a, Ws bf16; fp32 sum)
           conv_stage(x, o, ...)               sbk_conv_ffn_chain / sbk_conv_ffn_tail
    block  Xn = bf16(LN0(rows))
           Hs = bf16(act(Xn . W1^T + b1))
           z  = rows + alpha (Hs . W2^T + b2)  -> post-LN (block A of a chain; one block: optional)
    chain  block B on block A's result (fp32)
    tail   out = z;  u = next-LN(out) (fp32, or bf16 with u_bf16)
           yp = bf16(bf16(u) . Wp^T)           with a projection
    conv_stage
           xa = x + o . wo^T + bo              o, wo bf16; fp32
           U  = bf16(LN0c(xa))
           G  = bf16(val * sigmoid(gate)),  [val | gate] = U . W1c^T + b1c
           C  = bc + sum_k bf16(tap_k) G[t + k - padL]   zeros outside the utterance
           V  = bf16(swish(LN1(C)))
           xc = xa + mask0(V . W2c^T + b2c)

`rounding=True` rounds to bf16 (nearest even) at the points marked bf16(.)
above and nowhere else; `rounding=False` is the plain algebra on the weights
as given.  `dtype` is the arithmetic between the rounding points (float64; the
float32 evaluation is what the E32 table measures).  Values are rounded
float64 -> float32 -> bf16; the double rounding differs from one rounding only
on a float32 tie of a 2^-29 relative width.

Rounding points, read out of the code at this commit:

    ffn.hip:687-689     LN0 of rows read from memory -> Xn (pack_bf16x2)
    ffn.hip:630-632     LN0 of the CONV / SRC prologue's rows -> Xn
    ffn.hip:830-833     chain: LN0 of block B on block A's fp32 result -> Xn
    ffn.hip:782-783     act(phase 1 + b1) -> Hs
    ffn.hip:905-907     projection: u = next-LN(out) -> Xn
    ffn.hip:371-372     projection result -> yp (proj_pair, once)
    ffn.hip:1051-1052   the u output with u_bf16
    ffn.hip:808, 875    b2, alpha, residual: fp32;  row_ln (:296) fp32;
                        block A's result handed to block B (:822) fp32
    ffn.hip:542, 602-608  SRC: a, Ws bf16 operands, fp32 accumulators + sbias
    convstage.h:193, 277  o, wo bf16 operands; :311-312 xa fp32
    convstage.h:403-404 LN0 -> U
    convstage.h:503-504 GLU -> G
    ffn.hip:1213-1215   depthwise taps -> bf16 pairs (sbk_dw_image); convstage.h:569
                        v_dot2 of bf16 pairs, fp32 accumulation from the fp32 conv bias
    convstage.h:619-621 LN1, Swish -> V
    convstage.h:669-672 b2c, mask, residual fp32
    all GEMM weights    bf16 as given

Instantiations and the test ids of test_gpu_layer_terms.py that launch them
(act: none / swish / lrelu / gelu; `probe` ids take none and lrelu only):

    ffn_kernel<256, act, PROJ 0, CHAIN 0>   test_reference[ffn-<act>-...], test_exact_single[ffn-...]
    ffn_kernel<256, act, PROJ 1, CHAIN 0>   test_reference[ffn_proj-<act>-...], test_exact_single[ffn_proj-...]
    ffn_kernel<256, act, PROJ 1, CHAIN 1>   test_reference[ffn_chain-<act>-...-np256|np768-...], test_exact_chain[...-np256]
    ffn_kernel<256, act, PROJ 0, CHAIN 1>   test_reference[ffn_chain-<act>-...-np0-...], test_exact_chain[...-np0]
    conv_chain_kernel<act>                  test_reference[conv_ffn_chain-<act>-...], test_exact_conv[conv_ffn_chain-...]
    conv_tail_kernel<act>                   test_reference[conv_ffn_tail-<act>-...], test_exact_conv[conv_ffn_tail-...]
    src_ffn_kernel<act>                     test_reference[src_ffn_proj-<act>-...], test_exact_src[...]

Every reference id exercises every rounding point of its launch listed above
(a conv id those of convstage.h too); the exact probes are built so that no
rounding point rounds (every value at one is a bf16 number).

Bounds.  E32[family][output] is the deviation of reference(dtype=float32) from
reference() per tensor, max|err| / max(1, max|ref|); fp32 outputs are held to
max(1e-5, 8 E32), bf16 outputs (given here before their last rounding) to
|err| <= 2^-8 |ref| + that bound times max(1, max|ref|).  The float32
evaluation has exact products, float32 accumulation over K-steps of 32 and
correctly rounded LayerNorm sums, so that the table does not depend on a BLAS
or on the number of threads.  E32 is measured on each case and on further
draws of its rows (measure_e32), so it is at or above the figure of the case's
own inputs: whether one draw turns a rounding at all is chance, and where it
turns none the bound would be the 1e-5 floor, which one turned value breaks.
"""
import copy

import torch
import torch.nn.functional as F

D = 256
BM = 48  # rows (frames) per workgroup
ACTS = ("none", "swish", "lrelu", "gelu")
SLOPE = {"none": 0.0, "swish": 0.0, "lrelu": 0.01, "gelu": 0.0}
ACT_ABI = {"none": "none", "swish": "swish", "lrelu": "leaky_relu", "gelu": "gelu"}  # keys of _enc.ACT


# ------------------------------------------------------------------ primitives
def rbf(t, rounding=True):
    """Round to bf16, nearest even, keep the dtype."""
    return t.float().to(torch.bfloat16).to(t.dtype) if rounding else t


def ln(t, p, deff=D):
    """LayerNorm over the first deff columns in t's dtype, zeros in the rest.
    float32: the two reductions are correctly rounded (summed in float64), the
    rest is IEEE float32 arithmetic, so that the float32 evaluation does not
    depend on a library's summation order."""
    g, b, eps = p
    v = t[..., :deff]
    if t.dtype == torch.float64:
        y = F.layer_norm(v, (deff,), g[:deff].double(), b[:deff].double(), eps)
    else:
        d = v - v.double().mean(-1, keepdim=True).float()
        var = (d.double() ** 2).mean(-1, keepdim=True).float()
        y = d * (1.0 / torch.sqrt(var + eps)) * g[:deff] + b[:deff]
    return torch.cat([y, torch.zeros_like(t[..., deff:])], dim=-1)


def mm(a, w):
    """a . w^T in a's dtype.  float32: exact products, float32 accumulation
    over K-steps of 32 (the MFMA's), whatever the BLAS does."""
    if a.dtype == torch.float64:
        return a @ w.double().T
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    wd = w.double()
    for k0 in range(0, a.shape[1], 32):
        acc = acc + (a[:, k0:k0 + 32].double() @ wd[:, k0:k0 + 32].T).float()
    return acc


def _cr(fn, h):
    """fn(h) correctly rounded to h's dtype (evaluated in float64): the float32
    evaluation does not depend on a vector library's sigmoid or erf."""
    return fn(h.double()).to(h.dtype)


def act_fn(h, act, slope, scale=1.0):
    """The activation of scale * h (1: the kernel's)."""
    h = h * scale
    if act == "swish":
        return h * _cr(torch.sigmoid, h)
    if act == "gelu":
        return 0.5 * h * (1.0 + _cr(torch.erf, h * 0.70710678118654752))
    if act == "lrelu":
        return torch.where(h >= 0, h, h * slope)
    return h


def _block(x, p, act, slope, deff, rounding, scale):
    dt = x.dtype
    xn = rbf(ln(x, p["ln0"], deff), rounding)
    hs = rbf(act_fn(mm(xn, p["w1"]) + p["b1"].to(dt), act, slope, scale), rounding)
    z = x + p["alpha"] * (mm(hs, p["w2"]) + p["b2"].to(dt))
    return ln(z, p["post_ln"], deff) if p.get("post_ln") is not None else z


def dwconv(g3, taps, bias, padl, halo_tile=None):
    """g3 (B, T, D), taps (K, D): C[b, t] = bias + sum_k taps[k] g3[b, t + k - padl],
    zeros outside [0, T), summed tap by tap in g3's dtype.  halo_tile: frames
    of another halo_tile-frame tile read as zeros."""
    K, T = taps.shape[0], g3.shape[1]

    def run(g):
        gp = F.pad(g, (0, 0, padl, K - 1 - padl))
        acc = torch.zeros_like(g) if bias is None else bias.expand_as(g).clone()
        for k in range(K):
            acc = acc + taps[k] * gp[:, k:k + T]
        return acc

    if halo_tile is None:
        return run(g3)
    out = torch.zeros_like(g3)
    for t0 in range(0, T, halo_tile):
        own = torch.zeros_like(g3)
        own[:, t0:t0 + halo_tile] = g3[:, t0:t0 + halo_tile]
        out[:, t0:t0 + halo_tile] = run(own)[:, t0:t0 + halo_tile]
    return out


def conv_stage(x, cv, deff, rounding, halo_tile=None):
    """The convolution-module stage on (B*T, D) rows x: xc (B*T, D)."""
    dt = x.dtype
    B, T, K = cv["B"], cv["T"], cv["K"]
    xa = x + mm(cv["o"].to(dt), cv["wo"])
    if cv["bo"] is not None:
        xa = xa + cv["bo"].to(dt)
    u = rbf(ln(xa, cv["ln0"], deff), rounding)
    h = mm(u, cv["w1"]) + cv["b1"].to(dt)
    g = rbf(h[:, :D] * _cr(torch.sigmoid, h[:, D:]), rounding)
    padl = K - 1 if cv["causal"] else (K - 1) // 2
    bc = cv["bc"].to(dt) if cv["bc"] is not None else None
    c = dwconv(g.reshape(B, T, D), rbf(cv["taps"].to(dt), rounding), bc, padl, halo_tile).reshape(B * T, D)
    n = ln(c, cv["ln1"], deff)
    v = mm(rbf(n * _cr(torch.sigmoid, n), rounding), cv["w2"])
    if cv["b2"] is not None:
        v = v + cv["b2"].to(dt)
    if cv["kpm"] is not None:
        v = v.masked_fill(cv["kpm"].bool()[:, None], 0.0)
    return xa + v


def length_mask(rel_len, T):
    """(B*T,) uint8: t > floor(rel_len[b] * T) in float32, as sbk_length_mask."""
    lim = torch.floor(rel_len.float() * torch.tensor(float(T), dtype=torch.float32))
    return (torch.arange(T, dtype=torch.float32)[None] > lim[:, None]).to(torch.uint8).reshape(-1)


def reference(c, rounding=True, dtype=torch.float64, act_scale=(1.0, 1.0), halo_tile=None):
    """The outputs of launch c: a dict of `out`, `u`, `yp` (dtype) and `kpm_out`
    (uint8) as the launch has them.  bf16 outputs (the names in BF16_OUT(c)) are
    given before their last rounding, which the bf16 bound carries."""
    dt, deff = dtype, c["deff"]
    res = {}
    if "src" in c:
        s = c["src"]
        x = mm(s["a"].to(dt), s["ws"])
        if s["sbias"] is not None:
            x = x + s["sbias"].to(dt)
        if s["rel_len"] is not None:
            res["kpm_out"] = length_mask(s["rel_len"], s["T"])
    elif "conv" in c:
        x = conv_stage(c["x"].to(dt), c["conv"], deff, rounding, halo_tile)
    else:
        x = c["x"].to(dt)
    z = _block(x, c["A"], c["act"], c["slope"], deff, rounding, act_scale[0])
    if c.get("B") is not None:
        z = _block(z, c["B"], c["act"], c["slope"], deff, rounding, act_scale[1])
    if c["launch"] != "conv_ffn_tail":
        res["out"] = z
    if c.get("next_ln") is not None:
        u = ln(z, c["next_ln"], deff)
        if c.get("wp") is not None:
            res["yp"] = mm(rbf(u, rounding), c["wp"])
        else:
            res["u"] = u
    return res


def bf16_out(c):
    """The names of launch c's bf16 outputs."""
    if c.get("wp") is not None:
        return {"yp"}
    return {"u"} if c.get("u_bf16") and c.get("next_ln") is not None else set()


# ------------------------------------------------------------ reference inputs
# What the scales are for.  The bound is 8 E32, and E32 is the largest effect of
# one bf16 rounding turned by a float32-sized error: 2^-8 |operand| |weight| on
# an output that is a sum of 256 .. 2048 such products.  With Gaussian rows and
# weights N / 16 (test_gpu_proj_tail._block) that is 1e-3 .. 5e-3 of the output
# and a term such as alpha = 0.45 is not 4 bounds away from it.  So:
#   * no outliers: uniform rows and LayerNorm parameters, weights of random sign
#     and magnitude {0.75, 1, 1.25} * scale;
#   * rows 0.3 +- ROW_SD and a post-LN of that gain: eps = 1e-3 instead of 1e-5
#     changes 1 / sigma by tens of per cent, in block B too;
#   * b1 = 1 + 0.3 N and W2 row c = (FFN_MAG / H) (m_c + s), m_c = +-[0.5, 1.5]
#     (times 0.7, at the same size, for block A of the conv chain): the hidden units have a mean
#     and column c of the second GEMM is a coherent sum FFN_MAG m_c mean(h), large
#     against one turned value, while Xn still enters through an incoherent W1;
#   * the conv stage's contributions o . wo^T, bo, b2c of the rows' size, so that
#     LN0 of block A passes each of them on; a gate bias of N(0, 1); V . W2c^T a
#     quarter of that: a turned U or V value reaches the output through the
#     residual at 1e-3 of that product, a tap at a tenth of it, block A's LN0
#     terms through an incoherent sum, and the bound has to sit under all three.
# Changing any draw below changes the inputs and with them the E32 table.
W2_MEAN = 1.0      # |m_c| = W2_MEAN * [0.5, 1.5]
FFN_MAG = 0.07     # size of the second GEMM's coherent sum per unit m_c mean(h): of the rows' spread
CONV_W2 = 1 / 2048  # after_conv weight scale
CONV_A_MEAN = 0.7  # W2_MEAN of block A in the conv chain
CONV_ROW_SD = 0.02  # the conv launches' rows: the stage's own contributions add to the variance
ROW_SD = 0.035  # standard deviation of a row's values about their mean of 0.3


def _ch(deff):
    return (torch.arange(D) < deff).float()


def _uni(gen, shape, sd=1.0):
    """Uniform, zero mean, standard deviation sd: no outliers."""
    return (torch.rand(shape, generator=gen) - 0.5) * (sd * 12 ** 0.5)


def _w(gen, shape, scale):
    """A weight matrix of random signs and magnitudes scale * {0.75, 1, 1.25}."""
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    return sign * (0.75 + 0.25 * torch.randint(0, 3, shape, generator=gen).float()) * scale


def _lnp(gen, deff, gain=1.0, bsd=0.3, eps=1e-5, gsd=0.17):
    ch = _ch(deff)
    return (gain * (1.0 + _uni(gen, D, gsd)) * ch, _uni(gen, D, bsd) * ch, eps)


def _blk(gen, H, deff, post, w2_mean=None):
    ch = _ch(deff)
    # W2 row c = (FFN_MAG / H) (m_c + s), m_c = +-[0.5, 1.5]: with b1 of mean 1 the hidden units have a
    # mean, so column c of the second GEMM is a coherent sum of size FFN_MAG m_c; see the note above
    m = _uni(gen, D, 0.29)
    w2_mean = w2_mean or W2_MEAN
    m = w2_mean * torch.where(m >= 0, m + 1.0, m - 1.0)
    return dict(ln0=_lnp(gen, deff, bsd=0.5, gsd=0.4),
                w1=(_w(gen, (H, D), 1 / 16) * ch[None, :]).to(torch.bfloat16),
                b1=1.0 + 0.3 * torch.randn(H, generator=gen),
                w2=((m[:, None] + _w(gen, (D, H), 1.0)) * (FFN_MAG / w2_mean / H) * ch[:, None]).to(torch.bfloat16),
                b2=0.03 * torch.randn(D, generator=gen) * ch, alpha=0.5,
                post_ln=_lnp(gen, deff, gain=ROW_SD, bsd=0.01) if post else None)


def _rows(gen, M, deff, sd=ROW_SD):
    return ((_uni(gen, (M, D), sd) + 0.3) * _ch(deff)).contiguous()


def _conv(gen, B, T, K, causal, masked, deff):
    ch = _ch(deff)
    ch2 = torch.cat([ch, ch])
    kpm = None
    if masked:  # ragged: utterance b keeps floor(rel * T) + 1 frames
        kpm = length_mask(torch.tensor([1.0, 0.6] + [0.8] * (B - 2))[:B], T)
    return dict(B=B, T=T, K=K, causal=causal,
                o=(_uni(gen, (B * T, D)) * ch).to(torch.bfloat16),
                wo=(_w(gen, (D, D), 1 / 1024) * ch[:, None] * ch[None, :]).to(torch.bfloat16),
                bo=0.015 * torch.randn(D, generator=gen) * ch,
                ln0=_lnp(gen, deff),
                w1=(_w(gen, (2 * D, D), 1 / 16) * ch2[:, None] * ch[None, :]).to(torch.bfloat16),
                b1=torch.cat([0.3 * torch.ones(D), torch.ones(D)]) * torch.randn(2 * D, generator=gen) * ch2,
                taps=(_w(gen, (K, D), 1 / 4) * ch[None, :]).contiguous(),
                bc=0.3 * torch.randn(D, generator=gen) * ch,
                ln1=_lnp(gen, deff),
                w2=(_w(gen, (D, D), CONV_W2) * ch[:, None] * ch[None, :]).to(torch.bfloat16),
                b2=0.015 * torch.randn(D, generator=gen) * ch, kpm=kpm)


def make_case(launch, act, H, np_=0, deff=D, M=None, B=None, T=None, K=31, causal=False, masked=True, Kin=None,
              rel=False, u_bf16=False, post=True, seed=0):
    """The inputs of one reference case (CPU tensors in the kernels' formats:
    GEMM weights bf16, everything else fp32; w1 of the conv stage unpermuted,
    rows [:D] the GLU values and [D:] the gates)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    conv, src = launch.startswith("conv"), launch == "src_ffn_proj"
    chain = launch in ("ffn_chain", "conv_ffn_chain")
    if conv:
        M = B * T
    c = dict(launch=launch, act=act, slope=SLOPE[act], H=H, np=np_, deff=deff, M=M, u_bf16=u_bf16)
    if src:
        Tm = M // 2 if rel else 1
        c["src"] = dict(a=_uni(gen, (M, Kin)).to(torch.bfloat16),
                        ws=(_w(gen, (D, Kin), ROW_SD / Kin ** 0.5) * _ch(deff)[:, None]).to(torch.bfloat16),
                        sbias=(0.015 * torch.randn(D, generator=gen) + 0.3) * _ch(deff),
                        rel_len=torch.tensor([1.0, 0.55]) if rel else None, T=Tm)
        c["Kin"] = Kin
    else:
        c["x"] = _rows(gen, M, deff, CONV_ROW_SD if conv else ROW_SD)
    if conv:
        c["conv"] = _conv(gen, B, T, K, causal, masked, deff)
    c["A"] = _blk(gen, H, deff, post=post or chain or launch == "conv_ffn_tail",
                  w2_mean=CONV_A_MEAN if launch == "conv_ffn_chain" else None)
    c["B"] = _blk(gen, H, deff, post=False) if chain else None
    c["next_ln"] = _lnp(gen, deff)
    c["wp"] = (_w(gen, (np_, D), 1 / 16) * _ch(deff)[None, :]).to(torch.bfloat16) if np_ else None
    shape = f"B{B}T{T}K{K}{'c' if causal else ''}{'m' if masked else ''}" if conv else f"M{M}"
    if src:
        shape += f"Kin{Kin}{'r' if rel else ''}"
    c["id"] = f"{launch}-{act}-H{H}-np{np_}-d{deff}-{shape}{'-ubf' if u_bf16 else ''}"
    return c


def family(c):
    return (c["launch"], c["act"], c["H"])


def instantiation(c):
    """The kernel instantiation that launch c runs."""
    kern = {"conv_ffn_chain": "conv_chain_kernel", "conv_ffn_tail": "conv_tail_kernel", "src_ffn_proj": "src_ffn_kernel"}
    if c["launch"] in kern:
        return f"{kern[c['launch']]}<{c['act']}>"
    return f"ffn_kernel<256, {c['act']}, PROJ {int(c['np'] > 0)}, CHAIN {int(c.get('B') is not None)}>"


def _ref_cases():
    """Every launch with every activation; over them M in {48, 49, 97} (B 2,
    T in {49, 97}), H in {256, 1024} and 2048 for the single block, np in
    {256, 768}, d_eff in {256, 144}, K in {31, 15} and 31 causal."""
    cs = []
    Ms, Hs, NPs, Ds = (48, 49, 97), (256, 1024, 2048), (256, 768), (256, 144)
    for i, act in enumerate(ACTS):
        cs.append(make_case("ffn", act, Hs[i % 3], 0, Ds[i % 2], M=Ms[i % 3], u_bf16=bool(i % 2), seed=i))
        cs.append(make_case("ffn_proj", act, Hs[(i + 1) % 3], NPs[i % 2], Ds[(i + 1) % 2], M=Ms[(i + 1) % 3],
                            post=bool(i % 2), seed=10 + i))
        cs.append(make_case("ffn_chain", act, Hs[i % 2], NPs[(i + 1) % 2], Ds[i % 2], M=Ms[(i + 2) % 3], seed=20 + i))
        cs.append(make_case("ffn_chain", act, Hs[(i + 1) % 2], 0, Ds[(i + 1) % 2], M=Ms[i % 3], u_bf16=bool(i % 2),
                            seed=30 + i))
        cs.append(make_case("src_ffn_proj", act, Hs[(i + 2) % 3], NPs[i % 2], Ds[i % 2], M=(98, 48, 49, 98)[i],
                            Kin=(64, 256, 768, 256)[i], rel=i in (0, 3), seed=40 + i))
        K, causal = ((31, False), (15, False), (31, True), (31, False))[i]
        cs.append(make_case("conv_ffn_chain", act, Hs[(i + 1) % 2], NPs[(i + 1) % 2], Ds[i % 2], B=2, T=(97, 49)[i % 2],
                            K=K, causal=causal, masked=i != 1, seed=50 + i))
        K, causal = ((15, False), (31, True), (31, False), (31, False))[i]
        cs.append(make_case("conv_ffn_tail", act, Hs[i % 2], 0, Ds[(i + 1) % 2], B=2, T=(49, 97)[i % 2], K=K,
                            causal=causal, masked=i != 2, seed=60 + i))
    # Swish at the shapes of the default model
    cs.append(make_case("ffn_chain", "swish", 1024, 768, 144, M=97, seed=71))
    cs.append(make_case("conv_ffn_chain", "swish", 1024, 768, 256, B=2, T=97, K=31, seed=72))
    cs.append(make_case("conv_ffn_tail", "swish", 1024, 0, 256, B=2, T=97, K=31, seed=73))
    assert len({c["id"] for c in cs}) == len(cs)
    return cs


_CASES = None


def ref_cases():
    global _CASES
    if _CASES is None:
        _CASES = _ref_cases()
    return _CASES


_REF = {}


def cached_reference(c):
    """reference(c) in float64 with rounding, computed once per case and shared."""
    if c["id"] not in _REF:
        _REF[c["id"]] = reference(c)
    return _REF[c["id"]]


# --------------------------------------------------------------- E32 and bounds
# E32[family][output]: the largest deviation, over the family's cases in
# ref_cases() (measure_e32: the case and further draws of its rows), of
# reference(c, dtype=float32) from reference(c) (both with rounding), per tensor
# max|err| / max(1, max|ref|), rounded up to two digits.  It is dominated by the
# bf16 roundings (Xn, Hs, U, G, V, the projection's u) that the float32 error
# turns, which reach `out`, a LayerNorm'd `u` and `yp` at different sizes: hence
# one figure per output.  test_layer_ref_cpu.py::test_e32_table re-measures it.
E32 = {
    ("conv_ffn_chain", "gelu", 256): {"out": 4.3e-05, "yp": 0.00085},
    ("conv_ffn_chain", "lrelu", 1024): {"out": 2.5e-05, "yp": 0.00067},
    ("conv_ffn_chain", "none", 1024): {"out": 2.5e-05, "yp": 0.00076},
    ("conv_ffn_chain", "swish", 256): {"out": 3.1e-05, "yp": 0.00084},
    ("conv_ffn_chain", "swish", 1024): {"out": 2.8e-05, "yp": 0.00077},
    ("conv_ffn_tail", "gelu", 1024): {"u": 0.00014},
    ("conv_ffn_tail", "lrelu", 256): {"u": 0.00017},
    ("conv_ffn_tail", "none", 256): {"u": 0.00019},
    ("conv_ffn_tail", "swish", 1024): {"u": 0.00024},
    ("ffn", "gelu", 256): {"out": 4.7e-06, "u": 4.6e-05},
    ("ffn", "lrelu", 2048): {"out": 3.4e-06, "u": 3.3e-05},
    ("ffn", "none", 256): {"out": 1.3e-05, "u": 0.00011},
    ("ffn", "swish", 1024): {"out": 6.6e-06, "u": 5.1e-05},
    ("ffn_chain", "gelu", 256): {"out": 2.3e-05, "u": 0.00012},
    ("ffn_chain", "gelu", 1024): {"out": 6.5e-06, "yp": 0.00027},
    ("ffn_chain", "lrelu", 256): {"out": 2.3e-05, "yp": 0.00057},
    ("ffn_chain", "lrelu", 1024): {"out": 3.9e-06, "u": 1.9e-05},
    ("ffn_chain", "none", 256): {"out": 2.8e-05, "yp": 0.0008},
    ("ffn_chain", "none", 1024): {"out": 5.6e-06, "u": 4e-05},
    ("ffn_chain", "swish", 256): {"out": 1.9e-05, "u": 0.00012},
    ("ffn_chain", "swish", 1024): {"out": 7e-06, "yp": 0.00035},
    ("ffn_proj", "gelu", 1024): {"out": 6.3e-06, "yp": 0.00042},
    ("ffn_proj", "lrelu", 256): {"out": 1.2e-05, "yp": 0.00034},
    ("ffn_proj", "none", 1024): {"out": 4.3e-06, "yp": 0.00026},
    ("ffn_proj", "swish", 2048): {"out": 5.7e-06, "yp": 0.00029},
    ("src_ffn_proj", "gelu", 2048): {"out": 3.5e-06, "yp": 9.5e-05},
    ("src_ffn_proj", "lrelu", 1024): {"out": 5e-06, "yp": 0.00017},
    ("src_ffn_proj", "none", 2048): {"out": 2.6e-06, "yp": 0.00014},
    ("src_ffn_proj", "swish", 256): {"out": 8e-06, "yp": 0.00041},
}


def deviation(got, ref):
    """Per tensor: max|got - ref| / max(1, max|ref|)."""
    return float((got.double() - ref.double()).abs().max()) / max(1.0, float(ref.abs().max()))


def resampled(c, i):
    """Case c with its rows drawn again (draw i): the parameters stay, x, a and o change."""
    gen = torch.Generator().manual_seed(5000 + 17 * i + sum(map(ord, c["id"])))
    c = copy.copy(c)
    if "src" in c:
        c["src"] = dict(c["src"], a=_uni(gen, c["src"]["a"].shape).to(torch.bfloat16))
    else:
        c["x"] = _rows(gen, c["M"], c["deff"], CONV_ROW_SD if "conv" in c else ROW_SD)
    if "conv" in c:
        c["conv"] = dict(c["conv"], o=(_uni(gen, (c["M"], D)) * _ch(c["deff"])).to(torch.bfloat16))
    return c


E32_ROWS = 776  # rows per case over which E32 is measured (draws of M rows each, at least 4)


def measure_e32(c):
    """{output: deviation} of the float32 evaluation from the float64 one, on
    the case and on further draws of its rows, E32_ROWS rows in all: whether a
    bf16 rounding is turned at all in 10^4 .. 10^5 values is chance, and one
    draw alone would often record none."""
    worst = {}
    for i in range(max(4, -(-E32_ROWS // c["M"]))):
        ci = resampled(c, i) if i else c
        r64 = cached_reference(c) if i == 0 else reference(ci)
        r32 = reference(ci, dtype=torch.float32)
        for k in r64:
            if k != "kpm_out":
                worst[k] = max(worst.get(k, 0.0), deviation(r32[k], r64[k]))
    return worst


def bound(c, name):
    """The bound of output `name` of a case: max(1e-5, 8 * E32).  The 8 covers another
    summation order in the MFMA K-steps and the LayerNorm reductions and the
    1-ulp v_exp / v_rcp / v_rsq, each of which turns bf16 roundings as the
    float32 evaluation does (the margin of test_gpu_selfattn_paths.py)."""
    return max(1e-5, 8 * E32[family(c)][name])


def excess(got, ref, bnd, bf16):
    """How far got is from ref in units of the bound (<= 1 passes), and the
    plain deviation.  fp32 outputs: per tensor, deviation / bnd.  bf16 outputs:
    elementwise |err| <= 2^-8 |ref| + bnd max(1, max|ref|)."""
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    big = max(1.0, float(ref.abs().max()))
    if bf16:
        return float((err / (2.0 ** -8 * ref.abs() + bnd * big)).max()), float(err.max()) / big
    return float(err.max()) / big / bnd, float(err.max()) / big


# ------------------------------------------------------------------- the terms
def terms(c):
    """The names of the terms of launch c that test_every_term_is_visible drops
    or alters in the reference alone."""
    t = []
    for blk in ("A", "B") if c.get("B") is not None else ("A",):
        t += [f"{blk}.{n}" for n in ("ln0_gain", "ln0_bias", "ln0_eps", "b1", "b2", "alpha", "act", "h64")]
    if c["A"].get("post_ln") is not None:
        t += ["post.gain", "post.bias"]
    if c.get("next_ln") is not None:
        t += ["next.gain", "next.bias"]
    if "conv" in c:
        t += ["conv.bo", "conv.bc", "conv.b1_value", "conv.b1_gate", "conv.tap0", "conv.tapK", "conv.ln1_bias", "conv.b2"]
        if c["conv"]["kpm"] is not None:
            t.append("conv.kpm")
        if c["conv"]["T"] > BM:
            t.append("conv.halo")
    if "src" in c:
        t.append("src.sbias")
    return t


def altered(c, term):
    """(case, reference keywords) with one term dropped or altered: a bias
    zeroed, a gain set to one, eps 1e-3, alpha 0.45, the activation's argument
    times 1.2, the last 64 hidden units zeroed, a tap zeroed, the mask dropped,
    the halo across a 48-frame tile edge zeroed."""
    c = copy.copy(c)
    kw = {}
    where, name = term.split(".")
    live = _ch(c["deff"])
    if where in ("A", "B"):
        p = c[where] = dict(c[where])
        g, b, eps = p["ln0"]
        if name == "ln0_gain":
            p["ln0"] = (live.clone(), b, eps)
        elif name == "ln0_bias":
            p["ln0"] = (g, torch.zeros_like(b), eps)
        elif name == "ln0_eps":
            p["ln0"] = (g, b, 1e-3)
        elif name in ("b1", "b2"):
            p[name] = torch.zeros_like(p[name])
        elif name == "alpha":
            p["alpha"] = 0.45
        elif name == "act":
            kw["act_scale"] = (1.2, 1.0) if where == "A" else (1.0, 1.2)
        elif name == "h64":
            w2 = p["w2"].clone()
            w2[:, -64:] = 0
            p["w2"] = w2
    elif where in ("post", "next"):
        if where == "post":
            c["A"] = dict(c["A"])
        g, b, eps = c["A"]["post_ln"] if where == "post" else c["next_ln"]
        new = (live.clone(), b, eps) if name == "gain" else (g, torch.zeros_like(b), eps)
        if where == "post":
            c["A"]["post_ln"] = new
        else:
            c["next_ln"] = new
    elif where == "conv":
        cv = c["conv"] = dict(c["conv"])
        if name in ("bo", "bc", "b2"):
            cv[name] = None
        elif name in ("b1_value", "b1_gate"):
            b1 = cv["b1"].clone()
            (b1[:D] if name == "b1_value" else b1[D:]).zero_()
            cv["b1"] = b1
        elif name in ("tap0", "tapK"):
            taps = cv["taps"].clone()
            taps[0 if name == "tap0" else -1] = 0
            cv["taps"] = taps
        elif name == "ln1_bias":
            g, b, eps = cv["ln1"]
            cv["ln1"] = (g, torch.zeros_like(b), eps)
        elif name == "kpm":
            cv["kpm"] = None
        elif name == "halo":
            kw["halo_tile"] = BM
    elif where == "src":
        c["src"] = dict(c["src"], sbias=None)
    return c, kw


def reached_rows(c, term):
    """The rows a term can reach at all.  Every row, except: the mask reaches the
    masked rows; every term inside the conv module (conv bias, GLU bias, taps,
    LN1 bias, after_conv b2, halo) reaches the unmasked rows only, since a masked
    row's module output is zeroed; tap k reaches the rows whose frame t + k -
    padL lies inside the utterance; the halo reaches the rows whose window
    crosses a 48-frame tile edge."""
    M = c["M"]
    rows = torch.ones(M, dtype=torch.bool)
    if not term.startswith("conv.") or term == "conv.bo":
        return rows
    cv = c["conv"]
    T, K = cv["T"], cv["K"]
    masked = cv["kpm"].bool() if cv["kpm"] is not None else torch.zeros(M, dtype=torch.bool)
    if term == "conv.kpm":
        return masked
    rows = ~masked
    padl = K - 1 if cv["causal"] else (K - 1) // 2
    t = torch.arange(T)
    if term in ("conv.tap0", "conv.tapK"):
        f = t + (0 if term == "conv.tap0" else K - 1) - padl
        rows = rows & ((f >= 0) & (f < T)).repeat(cv["B"])
    if term == "conv.halo":
        lo, hi = (t - padl).clamp(0, T - 1), (t + K - 1 - padl).clamp(0, T - 1)
        rows = rows & ((lo // BM != t // BM) | (hi // BM != t // BM)).repeat(cv["B"])
    return rows


# --------------------------------------------------------------- exact probes
def walsh(M, bits=8):
    """(M, 256) of +-1: row r is the Walsh function of a distinct non-zero
    `bits`-bit mask, the `bits` single-bit masks first (so that from M >= bits
    rows on no two columns below 2^bits agree in every row)."""
    masks = [1 << i for i in range(bits)]
    n = (1 << bits) - 1
    step = 37 if bits == 8 else 11  # coprime to n
    i = 0
    while len(masks) < M:
        m = (i * step) % n + 1
        i += 1
        if m not in masks:
            masks.append(m)
    assert M <= n and len(set(masks[:M])) == M
    m = torch.tensor(masks[:M])[:, None] & torch.arange(D)[None, :]
    par = torch.zeros_like(m)
    for i in range(8):
        par ^= (m >> i) & 1
    return (1 - 2 * par).float()


def _probe_blk(H, k, seed, neutral=False):
    """A block whose result is exact: gain 1, b0 in [2, 4), one-hot W1 (a
    permutation per chunk), W2 one-hot on chunk k, every bias a multiple of
    2^-4.  neutral: W2 = 0 and b2 = 0 (the block returns its rows)."""
    j = torch.arange(H)
    q, i = j // 256, j % 256
    sig = ((2 * q + 3 + 2 * seed) * i + 11 * q + 5 + seed) % 256
    w1 = torch.zeros(H, D)
    w1[j, sig] = 1.0
    cc = torch.arange(D)
    pi = (13 * cc + 7 + 3 * seed) % 256
    w2 = torch.zeros(D, H)
    b2 = torch.zeros(D)
    if not neutral:
        w2[cc, 256 * k + pi] = 1.0
        b2 = ((3 * cc + 5 * (cc // 64) + seed) % 64).float() / 16 - 2  # no period of 64 (the Kin = 64 rows have one)
    b0 = 2 + ((7 * cc + 3 + 5 * seed) % 32).float() / 16
    b1 = ((5 * j + 1 + seed) % 64).float() / 16 - 2
    return dict(ln0=(torch.ones(D), b0, 1e-5), w1=w1.to(torch.bfloat16), b1=b1, w2=w2.to(torch.bfloat16), b2=b2,
                alpha=0.5, post_ln=None, sig=sig, pi=pi, k=k)


def probe_term(w, p, act, slope):
    """alpha (act(Xn W1^T + b1) W2^T + b2) of a probe block on rows 4 w or w
    (w: +-1 Walsh rows), in closed form, float64: column c takes hidden unit
    j = 256 k + pi(c), whose value is b0[sig(j)] + w[:, sig(j)] + b1[j]."""
    b0 = p["ln0"][1].double()
    if not bool(p["w2"].any()):
        return torch.zeros(w.shape[0], D, dtype=torch.float64)
    j = 256 * p["k"] + p["pi"]
    h = b0[p["sig"][j]][None, :] + w.double()[:, p["sig"][j]] + p["b1"].double()[j][None, :]
    return p["alpha"] * (act_fn(h, act, slope) + p["b2"].double()[None, :])


PROBE_SLOPE = {"none": 0.0, "lrelu": 0.5}


def probe_case(launch, act, H, k, M=None, np_=0, which="A", B=None, T=None, Kin=None, rel=False, u_bf16=False):
    """An exact probe of hidden chunk k of block `which`.  Rows 4 w_r (for
    block B of a chain: block A neutral and a post-LN of gain 1, bias 0, so
    that B's rows are LN(4 w_r) = w_r (1 - 3e-7)).  The projection is a
    selection: yp[:, n] = bf16(u[:, rho(n)])."""
    conv, src = launch.startswith("conv"), launch == "src_ffn_proj"
    chain = launch in ("ffn_chain", "conv_ffn_chain")
    if conv:
        M = B * T
    bits = 6 if Kin == 64 else 8
    w = walsh(M, bits)
    c = dict(launch=launch, act=act, slope=PROBE_SLOPE[act], H=H, np=np_, deff=D, M=M, u_bf16=u_bf16, w=w, which=which)
    gen = torch.Generator().manual_seed(77)
    if src:
        # a holds Kin / 256 scaled copies of the Walsh rows (Kin 64: their first 64 columns,
        # which a 6-bit mask repeats), Ws picks copy c % ncopy of column c back at 4 / scale
        ncopy = max(1, Kin // 256)
        sc = (1.0, 2.0, 0.5)[:ncopy]
        kw = min(Kin, 256)
        a = torch.cat([w[:, :kw] * s for s in sc], dim=1)
        ws = torch.zeros(D, Kin)
        cc = torch.arange(D)
        ws[cc, kw * (cc % ncopy) + cc % kw] = 4.0 / torch.tensor(sc)[cc % ncopy]
        c["src"] = dict(a=a.to(torch.bfloat16), ws=ws.to(torch.bfloat16), sbias=None,
                        rel_len=torch.tensor([1.0, 0.4]) if rel else None, T=M // 2 if rel else 1)
        c["Kin"] = Kin
    else:
        c["x"] = (4 * w).contiguous()
    if conv:  # a neutral conv stage: o = 0, bo = 0, after_conv weight and bias 0; the rest as a reference case
        cv = _conv(gen, B, T, 31, False, True, D)
        cv["o"] = torch.zeros_like(cv["o"])
        cv["bo"] = torch.zeros(D)
        cv["w2"] = torch.zeros_like(cv["w2"])
        cv["b2"] = torch.zeros(D)
        c["conv"] = cv
    unit = (torch.ones(D), torch.zeros(D), 1e-5)
    if which == "A":
        c["A"] = _probe_blk(H, k, 0)
        c["B"] = _probe_blk(H, 0, 1, neutral=True) if chain else None
        if chain or launch == "conv_ffn_tail":
            c["A"]["post_ln"] = _lnp(gen, D)
    else:
        c["A"] = _probe_blk(H, 0, 0, neutral=True)
        c["A"]["post_ln"] = unit
        c["B"] = _probe_blk(H, k, 1)
    c["next_ln"] = _lnp(gen, D)
    if np_:
        n = torch.arange(np_)
        wp = torch.zeros(np_, D)
        wp[n, (7 * n + 3 * (n // 256)) % 256] = 1.0
        c["wp"] = wp.to(torch.bfloat16)
        c["rho"] = (7 * n + 3 * (n // 256)) % 256
    else:
        c["wp"] = None
    c["id"] = f"probe-{launch}-{act}-H{H}-k{k}-{which}-M{M}-np{np_}"
    return c


def probe_expected(c):
    """The probe's outputs from the closed form: the stage before the first
    further LayerNorm exactly (float64 holds every value), the LayerNorms
    after it in float64.  `exact`: the names that are exact as they stand."""
    w, act, slope = c["w"], c["act"], c["slope"]
    if c["which"] == "A":
        z = 4 * w.double() + probe_term(w, c["A"], act, slope)
        exact = c["A"]["post_ln"] is None
        if not exact:
            z = ln(z, c["A"]["post_ln"])
    else:
        zp = ln(4 * w.double(), c["A"]["post_ln"])
        z = zp + probe_term(w, c["B"], act, slope)
        exact = False
    res = {}
    if c["launch"] != "conv_ffn_tail":
        res["out"] = z
    if c.get("next_ln") is not None:
        u = ln(z, c["next_ln"])
        if c["wp"] is not None:
            res["yp"] = u[:, c["rho"]]
        else:
            res["u"] = u
    if "src" in c and c["src"]["rel_len"] is not None:
        res["kpm_out"] = length_mask(c["src"]["rel_len"], c["src"]["T"])
    return res, ({"out"} if exact else set())
