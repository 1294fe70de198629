"""csrc/attention.hip kernel by kernel: the two LDS-DMA instantiations and the
eight instantiations of the general flash kernel, driven directly through
_enc.relpos_attention / _enc.mha_attention and compared key by key with a
float64 restatement of the same algebra on the kernels' operand layout
(core_ref_self below, anchored to oracle.conformer.rel_pos_mha by a CPU test).

Which kernel an id runs.  The first id component names it; test_dispatch_table
restates the host dispatch of sbk_relpos_attention_ld / sbk_relpos_attention_mask
/ sbk_mha_attention and checks every id against it:

    id                   kernel                                   reached by
    dma_band             relpos_flash_dma_kernel<true>            bf16, dh 64, no probs, no additive mask, qkv / pk
                                                                  16-B aligned, pk row stride % 8 == 0, T <= 4096
                                                                  (layout "aligned", and "pkcol": the encoder's
                                                                  column slice of a (2T-1, 3d) buffer)
    dma_plain            relpos_flash_dma_kernel<false>           _enc.mha_attention; reference without band / biases
    gen_bf16_64          relpos_flash_kernel<bf16_t, 64, false>   dh 32; dh 64 with an additive mask
                                                                  (sbk_relpos_attention_mask); dh 64 with qkv one
                                                                  element off alignment ("misq": scalar staging);
                                                                  dh 64 with a pk row stride of d + 4 ("pkld4":
                                                                  ldp % 8 == 4, scalar staging); T = 4097
    gen_bf16_64_probs    relpos_flash_kernel<bf16_t, 64, true>    need_probs, dh 64
    gen_bf16_128[_probs] relpos_flash_kernel<bf16_t, 128, *>      dh 96 and 128
    gen_f32_64[_probs]   relpos_flash_kernel<float, 64, *>        dh 64 and 32; 36 (vector path, dh % 8 == 4: the Q /
                                                                  bias fragment runs 4 dims past the head); 30
                                                                  (dh % 4 != 0: scalar staging)
    gen_f32_128[_probs]  relpos_flash_kernel<float, 128, *>       dh 128 and 72; 100 (dh % 8 == 4)

Shapes.  Every reach above runs T = 1, 63, 64, 65, 129 and 200 (one chunk with
every DMA row clamped, one past it, three chunks, and at 200 clamped first /
last blocks around the unclamped DMA fast path), with (B, H), the key-padding
mask and the input family rotated over them so that the grids
B * H * ceil(T / 64) include 1, 3, 8 and 9; T = 257 (B = 3) and T = 1037 add
the grids 15 and 17 for the XCD remap's remainders.  The DMA ids also run
T = 577 (nine chunks: every residue of the bitmap scan c0 = w + 8k,
c1 = c0 + 4), 2113 (chunks 31 / 32 / 33 across the mlo / mhi words) and 4096
(64 chunks, bit 63); gen_bf16_64 runs T = 4097, where the dispatch hands over.
Every id has its own seed (crc32 of the id).

Key-padding masks: "none" (a null pointer), "suffix" (ragged, ending in a
1-key utterance where B > 1), "lead" (leading padding, up to all keys but the
last), "hole<c>" (utterance b has exactly one padded key in chunk c + b: the
chunk's first key for even chunks, its last for odd ones).  Additive masks
(T = 129, every general id, with a suffix key-padding mask): "f2d" a (T, T)
float mask, "causal" a bool mask passed as 0 / -inf, "bh" a per-(B*H) float
mask with its batch / head strides.  test_every_row_keeps_a_key: no row is
fully masked (the reference is NaN there; out of scope).

Guard bands.  qkv, pk, pbu, pbv and the additive mask are views into larger
device buffers whose every other element is NaN (the columns beside a
strided pk included); around the key-padding mask the bytes are 1 (padded).
The views start a multiple of 16 B into their buffers (qkv of "misq": 130 B).
All of it is the test's own memory, so nothing can fault; a read outside an
operand that reaches arithmetic comes out as NaN, and is reported as such
before any numeric comparison.

Probe.  The kernels that return no probabilities are read out key by key:
with V = 0 but V[w0 + c, c] = 1 (c < dh), out[i, c] is P[i, w0 + c].  The
windows w0 cover every key for T <= 200 (plus one at 32 that straddles the
first chunk boundary and the tail window T - dh); for longer T they are 0, 32,
the tail and a window centred on each hole.  The rel_shift clamp slots, the
tail mask and the padded-chunk bitmap are each a single key's probability
there.

Inputs and bounds.  The error convention per tensor is max |err| / max(1,
max |ref|) unless stated elementwise; no bound was taken from a kernel run.

  fp32 ids: families "flat" (N(0,1) operands, biases 0.3 N(0,1), scale
    1/sqrt(d)) and "peaked" (K x 4; mean max-probability 0.33 .. 0.66 on the
    shapes used, asserted in 0.3 .. 0.9 by test_peaked_family_is_peaked; the
    score spread goes with 4 / sqrt(H), so peaked cases at T >= 129 take
    H <= 2).  out, probs and probe: max(1e-5, 8 * E32).  1e-5 is what the
    cross-attention kernels hold; E32 is the deviation of a float32 CPU
    evaluation of core_ref_self from the float64 one, the largest over the
    cases of a family and T (table E32 below; flat <= 1.1e-6, peaked 1.2e-6 ..
    1.9e-6, so the bounds are 1e-5 for flat and 1.0e-5 .. 1.52e-5 for peaked);
    8 x allows for another summation order and the 1-ulp hardware exp2.
  bf16 ids, family "grid": operands are rounded to bf16 first and the
    reference gets the rounded values.  q, pbu and pbv are multiples of 1/8 in
    [-2, 2] and scale = fl32(0.125 / log2(e)), for which fl32(scale * log2(e))
    is exactly 0.125 (test_grid_family_scale_is_exact), so the kernels' bf16
    Qu / Qv fragments are exact and the rounding of (q + u) * scale * log2(e)
    to bf16 (6.6e-3 absolute on probabilities with ordinary inputs, which
    would swamp a single key) does not occur.  K is 4 N(0,1), pk and V N(0,1),
    as bf16.  Two roundings remain, P to bf16 for the P.V MFMA and out to
    bf16, each <= 2^-8 relative, hence elementwise
        |out - ref| <= 2^-8 sum_j P_ij |v_jd| + 2^-8 |ref| + 1e-5,
    which for the probe's one-hot V is |out - P| <= 2^-7 P + 1e-5 (half a bf16
    ulp is at most 2^-8 of the value, so two round-to-nearest steps cannot
    exceed it; a CPU emulation that rounds the normalised P and out to bf16
    reaches 0.49 of it at T = 65, 200 and 577).  The fp32 probs of the _probs ids: max(1e-5, 8 * E32), E32 <= 5.2e-7.
  bf16 ids, family "ord": one case per bf16 kernel with N(0,1) operands and
    the model's scale 1/sqrt(d), at the 2e-2 elementwise (of max(1, |ref|))
    that test_relpos_attention_bf16_vs_torch holds, out and probs: the
    operand-rounding path stays exercised.

The references of T >= 2048 are evaluated in float64 with the same torch ops
on the device."""
import math
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import oracle.conformer as OC

gpu = pytest.mark.gpu

LOG2E32 = np.float32(1.4426950408889634)        # the kernels' log2(e) constant
GRID_SCALE = np.float32(0.125 / math.log2(math.e))  # fl32(GRID_SCALE * LOG2E32) == 0.125 exactly
# E32[family][T]: deviation of a float32 CPU evaluation of core_ref_self from the float64 one (out and
# probs, max |err| / max(1, max |ref|)), the largest over the fp32 cases of that family and T, measured
# on the CPU and rounded up to two digits (test_float32_reference_deviation_is_recorded re-measures it)
E32 = {"flat": {1: 0.0, 63: 4.4e-7, 64: 3.8e-7, 65: 4.0e-7, 129: 9.8e-7, 200: 1.1e-6},
       "peaked": {1: 0.0, 63: 1.2e-6, 64: 1.5e-6, 65: 1.7e-6, 129: 1.6e-6, 200: 1.9e-6, 257: 1.3e-6, 1037: 1.4e-6},
       "grid": {1: 0.0, 63: 2.8e-7, 64: 3.3e-7, 65: 2.8e-7, 129: 5.2e-7, 200: 3.8e-7}}  # probs of the _probs ids


def bound32(c):
    """The fp32 bound of a case: max(1e-5, 8 * E32)."""
    return max(1e-5, 8 * E32[c.fam][c.T])


DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16}
KERNELS = {
    "dma_band": "relpos_flash_dma_kernel<true>", "dma_plain": "relpos_flash_dma_kernel<false>",
    "gen_bf16_64": "relpos_flash_kernel<bf16_t, 64, false>",
    "gen_bf16_64_probs": "relpos_flash_kernel<bf16_t, 64, true>",
    "gen_bf16_128": "relpos_flash_kernel<bf16_t, 128, false>",
    "gen_bf16_128_probs": "relpos_flash_kernel<bf16_t, 128, true>",
    "gen_f32_64": "relpos_flash_kernel<float, 64, false>", "gen_f32_64_probs": "relpos_flash_kernel<float, 64, true>",
    "gen_f32_128": "relpos_flash_kernel<float, 128, false>",
    "gen_f32_128_probs": "relpos_flash_kernel<float, 128, true>",
}


def core_ref_self(qkv, pk, pbu, pbv, kpm, am, B, T, H, dh, scale):
    """The attention core of RelPosMHAXL for query = key = value from plain
    torch ops, in the dtype and on the device of qkv: qkv (B*T, 3d)
    head-interleaved [h][q|k|v][dh], pk (2T-1, d), pbu / pbv (H*dh) read as
    (H, dh), kpm (B, T) bool or None (True = padded, applied as -inf), am
    additive and broadcastable to (B, H, T, T) or None (added after the
    scale).  rel_shift in closed form: bd[i, T-1-i+j].  pk None: plain scaled
    dot-product attention, no biases.  Returns (out (B*T, d), probs
    (B, H, T, T))."""
    x = qkv.view(B, T, H, 3, dh)
    q, k, v = x[:, :, :, 0], x[:, :, :, 1], x[:, :, :, 2]
    if pk is None:
        score = torch.einsum("bihd,bjhd->bhij", q, k)
    else:
        ac = torch.einsum("bihd,bjhd->bhij", q + pbu.view(H, dh), k)
        bdf = torch.einsum("bihd,rhd->bhir", q + pbv.view(H, dh), pk.reshape(2 * T - 1, H, dh))
        i = torch.arange(T, device=qkv.device).view(T, 1)
        j = torch.arange(T, device=qkv.device).view(1, T)
        score = ac + torch.gather(bdf, -1, (T - 1 - i + j).expand(B, H, T, T))
        del bdf
    score = score * scale
    if am is not None:
        score = score + am
    if kpm is not None:
        score = score.masked_fill(kpm.view(B, 1, 1, T), -float("inf"))
    probs = torch.softmax(score, -1)
    return torch.einsum("bhij,bjhd->bihd", probs, v).reshape(B * T, H * dh), probs


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
TS = (1, 63, 64, 65, 129, 200)
# (B, H) per T, rotated over the reaches: the grids B * H * ceil(T / 64) of both kernel families
# include 1, 3, 8, 9 here, 15 at T = 257 and 17 at T = 1037 (test_grid_sizes_cover_remap_remainders)
BH = {1: ((1, 1), (3, 1), (2, 4), (3, 3)), 63: ((3, 1), (2, 4), (3, 3), (1, 2)), 64: ((2, 4), (1, 1), (3, 3), (3, 1)),
      65: ((2, 2), (3, 1), (1, 4), (2, 1)), 129: ((3, 1), (1, 1), (2, 2), (2, 4)), 200: ((2, 1), (3, 2), (1, 1), (2, 3))}
KPMS = ("none", "suffix", "lead")
# (kernel, dtype, dh, need_probs, layout); layouts: "aligned"; "misq" qkv one element off a 16-B boundary;
# "pkld4" pk row stride d + 4; "pkcol" pk a column slice of a (2T-1, 3d) buffer (stride 3d, the encoder's)
REACHES = [("dma_band", "bf16", 64, False, "aligned"), ("dma_band", "bf16", 64, False, "pkcol"),
           ("dma_plain", "bf16", 64, False, "aligned"),
           ("gen_bf16_64", "bf16", 32, False, "aligned"), ("gen_bf16_64", "bf16", 64, False, "misq"),
           ("gen_bf16_64", "bf16", 64, False, "pkld4"), ("gen_bf16_64_probs", "bf16", 64, True, "aligned")]
REACHES += [(f"gen_bf16_128{'_probs' if p else ''}", "bf16", dh, p, "aligned") for dh in (96, 128) for p in (False, True)]
REACHES += [(f"gen_f32_64{'_probs' if p else ''}", "f32", dh, p, "aligned") for dh in (64, 32, 36, 30)
            for p in (False, True)]
REACHES += [(f"gen_f32_128{'_probs' if p else ''}", "f32", dh, p, "aligned") for dh in (128, 72, 100)
            for p in (False, True)]

CASES = {}


def _add(kern, dt, dh, probs, lay, B, H, T, fam, kpm="none", am=None):
    cid = f"{kern}-d{dh}-{lay}-T{T}-B{B}H{H}-{fam}-{kpm}" + (f"-{am}" if am else "")
    assert cid not in CASES, cid
    CASES[cid] = SimpleNamespace(id=cid, kern=kern, dt=dt, dh=dh, probs=probs, lay=lay, B=B, H=H, T=T, fam=fam,
                                 kpm=kpm, am=am, d=H * dh, api="mha" if kern == "dma_plain" else "relpos")


def _build_cases():
    for r, (kern, dt, dh, probs, lay) in enumerate(REACHES):
        for t, T in enumerate(TS):
            B, H = BH[T][(r + t) % 4]
            fam = "grid" if dt == "bf16" else ("flat", "peaked")[(r + t) % 2]
            if fam == "peaked" and T >= 129:  # the score spread goes with 4 / sqrt(H): see
                H = min(H, 2)                 # test_peaked_family_is_peaked
            _add(kern, dt, dh, probs, lay, B, H, T, fam, KPMS[(r + t) % 3])
    # grids 15 and 17
    for kern, dt, dh, fam in (("dma_band", "bf16", 64, "grid"), ("dma_plain", "bf16", 64, "grid"),
                              ("gen_bf16_64", "bf16", 32, "grid"), ("gen_f32_64", "f32", 64, "peaked")):
        _add(kern, dt, dh, False, "aligned", 3, 1, 257, fam, "suffix")
        _add(kern, dt, dh, False, "aligned", 1, 1, 1037, fam, "lead")
    for kern in ("dma_band", "dma_plain"):
        # nine chunks: every residue of the bitmap scan (c0 = w + 8k, c1 = c0 + 4); one hole per utterance
        for c0 in (0, 3, 6):
            _add(kern, "bf16", 64, False, "aligned", 3, 1, 577, "grid", f"hole{c0}")
        _add(kern, "bf16", 64, False, "aligned", 2, 2, 577, "grid", "suffix")
        # chunks 31 / 32 / 33 across the mlo / mhi split; 64 chunks, bit 63
        for c0 in (31, 32, 33):
            _add(kern, "bf16", 64, False, "aligned", 1, 1, 2113, "grid", f"hole{c0}")
        _add(kern, "bf16", 64, False, "aligned", 1, 1, 4096, "grid", "hole63")
    _add("gen_bf16_64", "bf16", 64, False, "aligned", 1, 1, 4097, "grid", "hole63")  # the hand-over
    # additive masks, T = 129, with a suffix key-padding mask
    for am in ("f2d", "causal", "bh"):
        for kern, dt, dh in (("gen_bf16_64", "bf16", 64), ("gen_bf16_64_probs", "bf16", 64),
                             ("gen_bf16_128", "bf16", 96), ("gen_bf16_128_probs", "bf16", 128),
                             ("gen_f32_64", "f32", 36), ("gen_f32_64_probs", "f32", 64),
                             ("gen_f32_128", "f32", 100), ("gen_f32_128_probs", "f32", 72)):
            fam = "grid" if dt == "bf16" else ("peaked" if am == "f2d" else "flat")
            _add(kern, dt, dh, kern.endswith("_probs"), "aligned", 2, 2, 129, fam, "suffix70", am)
    # one ordinary case per bf16 kernel: N(0,1) operands and the model's scale (operand rounding in play)
    for kern, dh, lay in (("dma_band", 64, "pkcol"), ("dma_plain", 64, "aligned"), ("gen_bf16_64", 32, "aligned"),
                          ("gen_bf16_64_probs", 64, "aligned"), ("gen_bf16_128", 96, "aligned"),
                          ("gen_bf16_128_probs", 128, "aligned")):
        _add(kern, "bf16", dh, kern.endswith("_probs"), lay, 3, 2, 200, "ord", "suffix")


_build_cases()


def _dispatch(c):
    """The host dispatch of sbk_relpos_attention_ld / _mask / sbk_mha_attention
    restated: (kernel id, staging path) of a case."""
    bf, d = c.dt == "bf16", c.d
    ldp = {"pkld4": d + 4, "pkcol": 3 * d}.get(c.lay, d)
    aligned = c.lay != "misq"
    if c.api == "mha":
        assert bf and c.dh == 64 and c.T <= 4096 and aligned
        return "dma_plain", "dma"
    if c.am is None and bf and c.dh == 64 and not c.probs and ldp % 8 == 0 and c.T <= 4096 and aligned:
        return "dma_band", "dma"
    vec = 8 if bf else 4
    vec_ok = c.dh % vec == 0 and d % vec == 0 and ldp % vec == 0 and aligned
    return f"gen_{c.dt}_{64 if c.dh <= 64 else 128}" + ("_probs" if c.probs else ""), "vec" if vec_ok else "scalar"


def _hole_key(c, T):
    """The one padded key of chunk c: its first key (c even) or its last."""
    return 64 * c if c % 2 == 0 else min(64 * c + 63, T - 1)


def _kpm(c):
    """(B, T) bool key-padding mask of a case (True = padded), or None."""
    B, T = c.B, c.T
    if c.kpm == "none":
        return None
    m = torch.zeros(B, T, dtype=torch.bool)
    if c.kpm == "suffix":  # ragged, ending in a 1-key utterance where B > 1
        lens = {1: [max(1, 2 * T // 3)], 2: [max(1, 2 * T // 3), 1], 3: [T, max(1, 2 * T // 3), 1]}[B]
        m = torch.arange(T)[None] >= torch.tensor(lens)[:, None]
    elif c.kpm == "suffix70":
        m = torch.arange(T)[None] >= torch.tensor([T, 70])[:, None]
    elif c.kpm == "lead":  # leading padding, up to all keys but the last
        n = [min(x, T - 1) for x in (3, T // 2, T - 1)][:B]
        m = torch.arange(T)[None] < torch.tensor(n)[:, None]
    else:
        c0 = int(c.kpm[4:])
        for b in range(B):
            m[b, _hole_key(c0 + b, T)] = True
    return m


def _am(c, g):
    """Additive mask of a case as float32 (shape (T, T) or (B, H, T, T)), or None."""
    T = c.T
    if c.am is None:
        return None
    if c.am == "f2d":
        return 0.5 * torch.randn(T, T, generator=g)
    if c.am == "causal":  # the bool mask, passed as 0 / -inf
        return torch.zeros(T, T).masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), -float("inf"))
    return 0.5 * torch.randn(c.B, c.H, T, T, generator=g)


def _inputs(c):
    """Seeded CPU inputs of a case as float32 values (bf16 cases: rounded to
    bf16).  q / k / v are (B*T, H, dh); scale is the float32 the kernel gets."""
    g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
    B, T, H, dh, d = c.B, c.T, c.H, c.dh, c.d
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    grid = lambda t: (8 * t).round().clamp(-16, 16) / 8  # noqa: E731
    n = SimpleNamespace(q=rnd(B * T, H, dh), k=rnd(B * T, H, dh), v=rnd(B * T, H, dh), pk=rnd(2 * T - 1, d),
                        pbu=0.3 * rnd(d), pbv=0.3 * rnd(d), scale=np.float32(1.0 / math.sqrt(d)))
    if c.fam in ("peaked", "grid"):
        n.k = 4 * n.k
    if c.fam == "grid":
        n.q, n.pbu, n.pbv, n.scale = grid(n.q), grid(n.pbu), grid(n.pbv), GRID_SCALE
    if c.dt == "bf16":
        for a in ("q", "k", "v", "pk"):
            setattr(n, a, getattr(n, a).to(torch.bfloat16).float())
    n.kpm, n.am = _kpm(c), _am(c, g)
    return n


def _qkv(n, v=None):
    return torch.stack((n.q, n.k, n.v if v is None else v), 2).reshape(n.q.shape[0], -1)


def _ref_probs(c, n, dev=None, dtype=torch.float64):
    """core_ref_self's probabilities for a case (on dev when given)."""
    dev = dev or torch.device("cpu")
    to = lambda t: None if t is None else t.to(device=dev, dtype=dtype)  # noqa: E731
    am = None if n.am is None else to(n.am).view((1, 1, c.T, c.T) if n.am.dim() == 2 else n.am.shape)
    band = c.api != "mha"
    out, probs = core_ref_self(to(_qkv(n)), to(n.pk) if band else None, to(n.pbu) if band else None,
                               to(n.pbv) if band else None, None if n.kpm is None else n.kpm.to(dev), am, c.B, c.T,
                               c.H, c.dh, float(n.scale))
    return out, probs


def _pv(probs, v, B, T, H, dh):
    """(P · V, P · |V|) as (B*T, d) for v (B*T, H, dh) in probs' dtype."""
    v4 = v.to(device=probs.device, dtype=probs.dtype).view(B, T, H, dh)
    f = lambda x: torch.einsum("bhij,bjhd->bihd", probs, x).reshape(B * T, H * dh)  # noqa: E731
    return f(v4), f(v4.abs())


def _windows(c):
    """Probe windows (first key of each): every key once for T <= 200, and for
    longer T the head, a chunk-straddling window, the tail and the holes."""
    T, dh = c.T, c.dh
    last = max(T - dh, 0)
    if T <= 200:
        w = set(range(0, last + 1, dh)) | {last, min(32, last)}
    else:
        w = {0, 32, last}
        if c.kpm.startswith("hole"):
            w |= {min(max(_hole_key(int(c.kpm[4:]) + b, T) - dh // 2, 0), last) for b in range(c.B)}
    return sorted(w)


def _probe_v(c, w0):
    """V = 0 but V[j, col] = 1 for j = w0 + col: out[i, col] = P[i, w0 + col]."""
    v = torch.zeros(c.B, c.T, c.H, c.dh)
    for col in range(min(c.dh, c.T - w0)):
        v[:, w0 + col, :, col] = 1.0
    return v.view(c.B * c.T, c.H, c.dh)


# ---------------------------------------------------------------------------
# CPU checks of the reference and of the input conditions
# ---------------------------------------------------------------------------
def test_core_ref_matches_oracle():
    """core_ref_self on the oracle's own in_proj / linear_pos projections,
    through out_proj, is oracle.conformer.rel_pos_mha in float64 to 1e-12:
    no mask, a ragged key-padding mask, a 2-D bool attn_mask, a 2-D float one
    and a per-(B*H) float one, at dh = 16, 36 and 32."""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    for B, T, H, dh, lens, amk in ((2, 37, 4, 16, None, None), (3, 70, 2, 36, (70, 41, 1), None),
                                   (2, 20, 2, 36, (20, 13), "bool"), (2, 65, 1, 32, (65, 50), "f2d"),
                                   (2, 33, 3, 16, None, "bh")):
        d = H * dh
        sd = {"in_proj_weight": rnd(3 * d, d) / math.sqrt(d), "linear_pos.weight": rnd(d, d) / math.sqrt(d),
              "pos_bias_u": 0.3 * rnd(dh, H), "pos_bias_v": 0.3 * rnd(dh, H),
              "out_proj.weight": rnd(d, d) / math.sqrt(d), "out_proj.bias": rnd(d)}
        x, pe = rnd(B, T, d), rnd(1, 2 * T - 1, d)
        kpm = None if lens is None else torch.arange(T)[None] >= torch.tensor(lens)[:, None]
        am = {None: None, "bool": torch.ones(T, T, dtype=torch.bool).triu(1), "f2d": rnd(T, T),
              "bh": rnd(B * H, T, T)}[amk]
        ro, ra = OC.rel_pos_mha(x, pe, sd, "", H, kpm, am)
        add = None
        if am is not None:
            add = am.view(1, 1, T, T) if am.dim() == 2 else am.view(B, H, T, T)
            if add.dtype == torch.bool:
                add = torch.zeros(add.shape, dtype=torch.float64).masked_fill(add, -float("inf"))
        qkv = F.linear(x, sd["in_proj_weight"]).reshape(B * T, 3 * d)
        pk = F.linear(pe, sd["linear_pos.weight"]).reshape(2 * T - 1, d)
        o, a = core_ref_self(qkv, pk, sd["pos_bias_u"].reshape(-1), sd["pos_bias_v"].reshape(-1), kpm, add, B, T, H,
                             dh, 1.0 / math.sqrt(d))
        out = F.linear(o, sd["out_proj.weight"], sd["out_proj.bias"]).view(B, T, d)
        tag = (B, T, H, dh, amk)
        assert torch.isfinite(ro).all() and torch.isfinite(ra).all(), tag
        assert float((out - ro).abs().max()) <= 1e-12, tag
        assert float((a - ra).abs().max()) <= 1e-12, tag


def test_dispatch_table():
    """Every case names the kernel the host dispatch sends it to, every
    instantiation of both kernels is reached, and the general kernel runs
    its vector and its scalar staging in both dtypes."""
    seen = set()
    for c in CASES.values():
        kern, path = _dispatch(c)
        assert kern == c.kern, (c.id, kern)
        seen.add((kern, path))
        if c.lay in ("misq", "pkld4") or c.dh == 30:
            assert path == "scalar", c.id
    assert {k for k, _ in seen} == set(KERNELS)
    for dt in ("bf16", "f32"):
        assert {p for k, p in seen if k.startswith(f"gen_{dt}")} == {"vec", "scalar"}


def test_grid_sizes_cover_remap_remainders():
    """The XCD remap (nwg >> 3 tiles per XCD, nwg & 7 XCDs with one more) runs
    at grids 1, 3, 8, 9, 15 and 17 in the DMA kernels and in the general one."""
    for fam in ("dma", "gen"):
        grids = {c.B * c.H * ((c.T + 63) // 64) for c in CASES.values() if c.kern.startswith(fam)}
        assert {1, 3, 8, 9, 15, 17} <= grids, (fam, sorted(grids))


def test_every_row_keeps_a_key():
    for c in CASES.values():
        g = torch.Generator().manual_seed(zlib.crc32(c.id.encode()))
        kpm = _kpm(c)
        live = torch.ones(c.B, 1, 1, c.T, dtype=torch.bool) if kpm is None else ~kpm.view(c.B, 1, 1, c.T)
        if c.am is not None:
            am = _am(c, g)
            live = live & (am.view((1, 1, c.T, c.T) if am.dim() == 2 else am.shape) > -float("inf"))
        assert bool(live.any(-1).all()), c.id
        if c.kpm.startswith("hole"):
            assert kpm.sum(-1).tolist() == [1] * c.B, c.id


def test_grid_family_scale_is_exact():
    """fl32(scale * log2(e)) is exactly 0.125 for the bf16 grid family, whose
    q, pbu and pbv are multiples of 1/8 in [-2, 2]: (q + u) * 0.125 has at most
    6 significant bits, so the kernels' bf16 Qu / Qv fragments are exact."""
    assert np.float32(GRID_SCALE) * LOG2E32 == np.float32(0.125)
    c = next(c for c in CASES.values() if c.fam == "grid" and c.T == 200)
    n = _inputs(c)
    for t in (n.q, n.pbu, n.pbv):
        assert torch.equal(t * 8, (t * 8).round()) and float(t.abs().max()) <= 2.0
    qu = (n.q + n.pbu.view(c.H, c.dh)) * 0.125
    assert torch.equal(qu.to(torch.bfloat16).float(), qu)


def test_peaked_family_is_peaked():
    """The fp32 peaked family (K x 4) has a mean max-probability between 0.3
    and 0.9 under the reference (no masks), at every shape with T >= 63 it
    runs (the flat family is printed beside it)."""
    for c in CASES.values():
        if c.dt != "f32" or c.T < 63:
            continue
        n = _inputs(c)
        n.kpm = n.am = None
        mp = float(_ref_probs(c, n)[1].amax(-1).mean())
        print(f"selfattn_paths {c.id}: mean max-probability {mp:.3f}")
        assert c.fam == "flat" or 0.3 <= mp <= 0.9, (c.id, mp)


def test_float32_reference_deviation_is_recorded():
    """The E32 table: every fp32 case's float32 CPU evaluation of
    core_ref_self (and the probabilities of the bf16 _probs grid cases)
    deviates from float64 by no more than twice the recorded figure of its
    family and T (the margin is for another BLAS build's summation order; on
    the machine it was measured on it is within 1x)."""
    for c in CASES.values():
        if c.dt != "f32" and not (c.probs and c.fam == "grid"):
            continue
        n = _inputs(c)
        o64, p64 = _ref_probs(c, n)
        o32, p32 = _ref_probs(c, n, dtype=torch.float32)
        e = float((p32 - p64).abs().max())
        if c.dt == "f32":
            e = max(e, float((o32 - o64).abs().max()) / max(1.0, float(o64.abs().max())))
        assert e <= 2 * E32[c.fam][c.T], (c.id, e)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _guard(t, dev, dtype, front=64, ld=None, col0=0, fill=float("nan"), back=64):
    """t as a view into a larger device buffer whose every other element is
    `fill`: `front` elements before it, `back` after; ld / col0: t's rows are a
    column slice [col0, col0 + cols) of rows of ld elements."""
    if ld is None:
        buf = torch.full((front + t.numel() + back,), fill, device=dev, dtype=dtype)
        x = buf[front:front + t.numel()].view(t.shape)
    else:
        rows, cols = t.shape
        buf = torch.full((front + rows * ld + back,), fill, device=dev, dtype=dtype)
        x = buf[front:front + rows * ld].view(rows, ld)[:, col0:col0 + cols]
    x.copy_(t)
    assert buf.data_ptr() % 64 == 0
    return x


def _operands(c, n, dev):
    dtype, d = DTYPE[c.dt], c.d
    a = SimpleNamespace()
    a.qkv = _guard(_qkv(n), dev, dtype, front=65 if c.lay == "misq" else 64)
    assert a.qkv.is_contiguous() and (a.qkv.data_ptr() % 16 != 0) == (c.lay == "misq")
    ld, col0 = {"pkld4": (d + 4, 0), "pkcol": (3 * d, d)}.get(c.lay, (None, 0))
    a.pk = _guard(n.pk, dev, dtype, ld=ld, col0=col0)
    assert a.pk.data_ptr() % 16 == 0 and a.pk.stride(0) == (ld or d)
    a.pbu, a.pbv = _guard(n.pbu, dev, torch.float32, front=4), _guard(n.pbv, dev, torch.float32, front=12)
    a.kpm = None if n.kpm is None else _guard(n.kpm.to(torch.uint8), dev, torch.uint8, front=16, fill=1)
    a.am = None
    if n.am is not None:
        m = _guard(n.am, dev, torch.float32)
        a.am = (m, 0, 0) if m.dim() == 2 else (m, c.H * c.T * c.T, c.T * c.T)
    return a


def _launch(c, n, a):
    from speechbrain_amd import _enc
    if c.api == "mha":
        return _enc.mha_attention(a.qkv, a.kpm, c.B, c.T, c.H, c.dh, float(n.scale)), None
    return _enc.relpos_attention(a.qkv, a.pk, a.pbu, a.pbv, a.kpm, c.B, c.T, c.H, c.dh, float(n.scale),
                                 need_probs=c.probs, am=a.am)


def _where(c, idx, w0=None):
    row, col = int(idx) // c.d, int(idx) % c.d
    s = f"b {row // c.T} query {row % c.T} head {col // c.dh} dim {col % c.dh}"
    return s + (f" = key {w0 + col % c.dh}" if w0 is not None else "")


def _check_out(c, tag, got, ref, mag, w0=None):
    """got (B*T, d) from the kernel against ref = P · V (mag = P · |V|)."""
    assert got.dtype == DTYPE[c.dt] and got.shape == ref.shape, (tag, got.dtype, got.shape)
    got, ref, mag = got.double().cpu(), ref.cpu(), mag.cpu()
    bad = ~torch.isfinite(got)
    assert not bad.any(), (f"{tag}: {int(bad.sum())} non-finite outputs (a read outside an operand reached "
                           f"arithmetic), first at {_where(c, bad.flatten().nonzero()[0], w0)}")
    err = (got - ref).abs()
    if c.dt == "f32":
        tol = torch.full_like(err, bound32(c) * max(1.0, float(ref.abs().max())))
    elif c.fam == "ord":
        tol = 2e-2 * ref.abs().clamp(min=1.0)
    else:
        tol = 2.0 ** -8 * mag + 2.0 ** -8 * ref.abs() + 1e-5
    ratio = err / tol
    worst = int(ratio.argmax())
    print(f"selfattn_paths {tag}: max err {float(err.max()):.3e}, worst err / bound {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0, (f"{tag}: err {float(err.flatten()[worst]):.3e} > bound "
                                       f"{float(tol.flatten()[worst]):.3e} at {_where(c, worst, w0)} "
                                       f"(ref {float(ref.flatten()[worst]):.4e}); "
                                       f"{int((ratio > 1).sum())} / {ratio.numel()} out of bound")


def _run_case(c, dev):
    n = _inputs(c)
    rdev = dev if c.T >= 2048 else None  # the long references in float64 on the device
    ref_out, P = _ref_probs(c, n, rdev)
    assert torch.isfinite(P).all()
    a = _operands(c, n, dev)
    out, probs = _launch(c, n, a)
    _check_out(c, f"{c.id} out", out, ref_out, _pv(P, n.v, c.B, c.T, c.H, c.dh)[1])
    if c.probs:
        assert probs.shape == P.shape and probs.dtype == torch.float32
        pg = probs.double().cpu()
        assert torch.isfinite(pg).all(), f"{c.id}: non-finite probabilities"
        err = float((pg - P.cpu()).abs().max())
        bound = 2e-2 if c.fam == "ord" else bound32(c)
        print(f"selfattn_paths {c.id} probs: max err {err:.3e} bound {bound:.0e}")
        assert err <= bound, (c.id, err)
        return
    assert probs is None
    if c.fam == "ord":
        return
    v3 = a.qkv.view(c.B * c.T, c.H, 3, c.dh)[:, :, 2]
    for w0 in _windows(c):
        v = _probe_v(c, w0)
        v3.copy_(v)
        out, _ = _launch(c, n, a)
        _check_out(c, f"{c.id} probe w0={w0}", out, *_pv(P, v, c.B, c.T, c.H, c.dh), w0=w0)


@gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_selfattn_kernel(dev, cid):
    """One case of the table in the module docstring: out for random V, the
    returned probabilities of the _probs kernels, and for the kernels that
    return none the probabilities read out key by key through one-hot V
    windows; all operands inside NaN guard bands."""
    _run_case(CASES[cid], dev)
