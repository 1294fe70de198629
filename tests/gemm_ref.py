"""Exact integer probes for the GEMM family (csrc/gemm.hip, gemm_tn.hip and
the bf16 half of gemm256.hip): the case lists, the operands, the references
and the checker shared by test_gemm_ref_cpu.py and test_gpu_gemm_tiles.py.

Operands are integers in [-4, 4] (exact in bf16 and fp32).  With K <= 1288
every partial sum of a product is bounded by 16 K < 2^15, far below 2^24, so
ANY fp32 accumulation order — every MFMA shape, every split across
workgroups, the fp32 atomics of gemm_tn — gives the same bits, and the
reference is an int64 matmul on the CPU.  Bias, alpha = 0.5, the row mask,
the residual and LeakyReLU(0.25) keep the result exact (multiples of 1/8
below 2^15), so the fp32 output is compared bit for bit and the bf16 output
against ref.to(bfloat16) bit for bit.

Swish, GELU, GLU and the row LayerNorm are inexact: there W is scaled by
1/64 and bias by 1/4 (still exact operands; K <= 256 keeps the
pre-activations O(1)), the reference is the epilogue in float64 on the exact
pre-activation, and the bound is the project's fp32 one (test_gpu_layer_terms,
test_gpu_lstm): |err| / max(1, |ref|_inf) <= max(1e-5, 8 E32), E32 the same
epilogue evaluated by torch in fp32 on the CPU; a bf16 output adds
2^-8 |ref| per element (half a bf16 ulp).

No GPU is needed to import this module."""
import dataclasses
import functools

import torch

SBK_ERR_ARG = 1001
PAD = 64               # guard band (elements) either side of every device buffer
SENTINEL = -12288.0    # exact in bf16 and fp32, finite, never a plausible result of a stray store
ALPHA = 0.5
SLOPE = 0.25
LN_EPS = 1e-5
ACT_ID = {"none": 0, "affine": 0, "lrelu": 3, "swish": 1, "gelu": 4, "glu": 2}
EXACT = ("none", "affine", "lrelu")
INEXACT = ("swish", "gelu", "glu")
LAYOUTS = ("dense", "strided", "out+1", "ldr+1", "bias+1")

# tile id -> (BM, BN, BK), from the switch in sbk_gemm
TILES_BF16 = {1: (128, 128, 64), 2: (64, 64, 64), 3: (128, 64, 64), 4: (64, 64, 256), 5: (64, 128, 256),
              6: (128, 64, 256), 7: (128, 128, 128), 8: (64, 64, 128), 9: (64, 64, 32), 10: (128, 64, 32),
              11: (128, 128, 64), 12: (128, 64, 64), 13: (64, 64, 64), 17: (64, 128, 32), 18: (64, 64, 64),
              19: (128, 64, 64), 20: (64, 128, 64), 21: (128, 128, 64), 22: (64, 64, 32), 30: (256, 256, 64)}
TILES_F32 = {1: (128, 128, 32), 2: (64, 64, 32), 3: (128, 64, 32)}
RING = (11, 12, 13)
PREFETCH = (18, 19, 20, 21, 22)
# sbk_gemm_ln instantiations: name -> (operands bf16, tile argument, BM, BK)
LN_INST = {"bf16-0": (True, 0, 32, 32), "bf16-1": (True, 1, 32, 64), "bf16-2": (True, 2, 64, 32),
           "fp32": (False, 0, 32, 32)}


@dataclasses.dataclass(frozen=True)
class Case:
    entry: str                 # C-ABI entry point
    bf16: bool                 # operand dtype (else fp32)
    tile: int
    M: int
    N: int
    K: int
    epi: str = "none"
    out_bf16: bool = False     # sbk_gemm_ln: dtype of u
    layout: str = "dense"
    batch: int = 1
    zdiv: int = 0              # sbk_gemm_batched: heads H of the head-interleaved layout
    nsplit: int = 0            # sbk_gemm_tn*
    seed: int = 0

    @property
    def scaled(self):
        return self.epi in INEXACT

    @property
    def vec(self):
        return 8 if self.bf16 else 4

    @property
    def bm(self):
        if self.entry == "sbk_gemm":
            return (TILES_BF16 if self.bf16 else TILES_F32)[self.tile or 2][0]
        return 64

    @property
    def nout(self):
        return self.N // 2 if self.epi == "glu" else self.N

    @property
    def expect_err(self):
        """The entry point must refuse this case with SBK_ERR_ARG (and write nothing)."""
        if self.entry != "sbk_gemm":
            return False
        if self.tile in RING:
            return bool(self.K % 64 or self.K < 192)
        if self.tile == 30:  # gemm256: N % 256, K % 64, aligned epilogue operands, no GLU
            return bool(self.N % 256 or self.K % 64 or self.epi == "glu"
                        or self.layout in ("out+1", "ldr+1", "bias+1"))
        return False

    def mask_rows(self):
        if self.epi == "none" or self.entry not in ("sbk_gemm", "sbk_gemm_ln"):
            return ()
        if self.entry == "sbk_gemm_ln":
            return tuple(sorted({self.M // 2, self.M - 1}))
        return tuple(sorted({0, self.M - 1, min(self.bm, self.M) - 1}))

    def __str__(self):
        s = (f"{self.entry} {'bf16' if self.bf16 else 'fp32'} tile {self.tile} M={self.M} N={self.N} K={self.K} "
             f"epilogue={self.epi} out={'bf16' if self.out_bf16 else 'fp32'} layout={self.layout}")
        if self.batch > 1 or self.entry == "sbk_gemm_batched":
            s += f" batch={self.batch} zdiv={self.zdiv}"
        if self.entry.startswith("sbk_gemm_tn"):
            s += f" nsplit={self.nsplit}"
        return s


# ---------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------
def table_shapes(tile, BM, BN, BK, vec):
    """The (M, N, K) table of the issue for one tile.  The LDS-DMA ring takes
    only K % 64 == 0, K >= 192, so its K column is replaced by the ring's own
    3 steps (the prologue's minimum), a full ring, the first wrap and two wraps."""
    t = [(1, 8, vec), (BM, BN, BK), (BM + 1, BN + 4, BK + vec), (BM - 1, BN - 2, 2 * BK), (3 * BM, 3 * BN, 3 * BK),
         (17 * BM, BN, BK), (8 * BM, BN, BK), (2 * BM + 3, 72, 5 * BK + vec)]
    if tile in RING:
        ring_k = (192, 192, 256, 320, 576, 192, 256, 320)
        t = [(m, n, k) for (m, n, _), k in zip(t, ring_k)]
    return t


def _with_epilogues(mk, shapes, glu_ok=True, rotate_inexact=False):
    """Both output dtypes on every shape: the exact epilogues rotated over the
    shapes, every inexact one on each shape with K <= 256 (GLU: N % 32 == 0;
    rotate_inexact: one of Swish / GELU per shape, for the long gemm256 list)."""
    out = []
    for i, (M, N, K) in enumerate(shapes):
        for ob in (False, True):
            out.append(mk(M, N, K, EXACT[(i + ob) % 3], ob))
        if K <= 256:
            for epi in ((INEXACT[(i + i // 2) % 2],) if rotate_inexact else INEXACT):
                if epi == "glu" and (N % 32 or not glu_ok):
                    continue
                for ob in (False, True):
                    out.append(mk(M, N, K, epi, ob))
    return out


def gemm_cases(bf16, tile):
    """Every sbk_gemm launch of one (dtype, tile id)."""
    BM, BN, BK = (TILES_BF16 if bf16 else TILES_F32)[tile]
    vec = 8 if bf16 else 4

    def mk(M, N, K, epi, ob, layout="dense"):
        return Case("sbk_gemm", bf16, tile, M, N, K, epi, ob, layout, seed=tile)

    if tile == 30:
        shapes = [(M, N, K) for K in (64, 128, 192, 320) for M in (1, 255, 256, 257, 513) for N in (256, 768)]
        cases = _with_epilogues(mk, shapes, glu_ok=False, rotate_inexact=True)
        cases += [mk(256, 264, 64, "none", False), mk(256, 256, 64, "glu", False), mk(256, 256, 64, "glu", True)]
        full, ragged = (256, 256, 64), (257, 256, 128)
    else:
        cases = _with_epilogues(mk, table_shapes(tile, BM, BN, BK, vec))
        kg = 192 if tile in RING else BK
        for (M, N) in ((BM, 32), (BM + 1, BN + 32)):   # GLU: one group, and a ragged second tile column
            cases += [mk(M, N, kg, "glu", ob) for ob in (False, True)]
        if tile in RING:
            cases += [mk(BM, BN, 128, "none", False), mk(BM, BN, 200, "none", True)]
            full, ragged = (BM, BN, 192), (BM + 1, BN + 4, 256)
        else:
            full, ragged = (BM, BN, BK), (BM + 1, BN + 4, BK + vec)
        if tile in PREFETCH:  # 1, 2, 3, 4, 5, 9 steps of the 4-deep register pipeline, whole and with a K tail
            i = 0
            for n in (1, 2, 3, 4, 5, 9):
                for K in (n * BK, n * BK - 8):
                    for (M, N) in ((BM, BN), (BM + 1, BN + 4)):
                        cases.append(mk(M, N, K, EXACT[i % 3], bool((i // 3) & 1)))
                        i += 1
    for layout in LAYOUTS:
        for shp in (full, ragged):
            epis = ("affine", "glu") if shp is full else ("affine",)
            cases += [mk(*shp, epi, ob, layout) for epi in epis for ob in (False, True)]
    return cases


def gemm_ln_cases(inst):
    bf16, tile, _, BK = LN_INST[inst]
    vec = 8 if bf16 else 4
    cases = []
    for M in (1, 31, 32, 33, 65, 9 * 32 + 5):
        for K in (vec, BK, BK + vec, 3 * BK, 640):
            for ub in (False, True):
                cases.append(Case("sbk_gemm_ln", bf16, tile, M, 256, K, "affine", ub, "dense", seed=40 + tile))
            if M in (33, 9 * 32 + 5):
                cases.append(Case("sbk_gemm_ln", bf16, tile, M, 256, K, "affine", K == BK, "strided", seed=40 + tile))
    return cases


def batched_cases(bf16):
    vec = 8 if bf16 else 4
    cases, i = [], 0
    for M in (1, 63, 64, 65):
        for N in (8, 16, 72):
            for K in (vec, 48, 64 + vec):
                ob, heads, big = bool(i & 1), bool(i & 2), bool(i & 4)
                batch = 12 if big else 1
                cases.append(Case("sbk_gemm_batched", bf16, 0, M, N, K, "none", ob, "strided", batch=batch,
                                  zdiv=(4 if big else 1) if heads else 0, seed=50))
                i += 1
    return cases


TN_MN = (8, 56, 64, 72, 128, 136, 264)


def tn_cases(tile):
    cases, i = [], 0
    for K in (1, 63, 64, 65, 129, 1000):
        for nsplit in (1, 2, 3, 8, 0):
            M, N = TN_MN[i % 7], TN_MN[(3 * i + 2) % 7]
            cases.append(Case("sbk_gemm_tn_cfg", True, tile, M, N, K, nsplit=nsplit, layout="strided", seed=60 + tile))
            if i % 5 == 0:  # the per-head block layout of gemm_tn_into: padded batch strides, ldc = N + 8
                cases.append(Case("sbk_gemm_tn_cfg", True, tile, N, M, K, nsplit=nsplit, layout="strided", batch=3,
                                  seed=61 + tile))
            i += 1
    return cases


def tn_auto_cases():
    """sbk_gemm_tn (tile and split count chosen by the entry point)."""
    return [Case("sbk_gemm_tn", True, 0, M, N, K, layout="strided", batch=b, seed=70)
            for (M, N, K, b) in ((72, 136, 129, 1), (264, 128, 1000, 1), (64, 56, 65, 3))]


def tn_f32_cases():
    cases = []
    for (M, N, layout) in ((40, 36, "dense"), (37, 70, "dense"), (3, 3, "dense"), (40, 36, "lda+1")):
        for K in (1, 31, 32, 33, 257):
            for nsplit in (0, 1, 3):
                cases.append(Case("sbk_gemm_tn_f32", False, 0, M, N, K, nsplit=nsplit, layout=layout, seed=80))
    for (M, N) in ((40, 36), (37, 70)):
        for K, nsplit in ((33, 0), (257, 3)):
            cases.append(Case("sbk_gemm_tn_f32", False, 0, M, N, K, nsplit=nsplit, layout="strided", batch=4, seed=81))
    return cases


def dispatch_cases(bf16):
    """tile = 0 against tile = 2 (test_gemm_auto_tile_equals_tile_2)."""
    return [Case("sbk_gemm", bf16, 2, M, N, K, epi, ob, seed=9) for (M, N, K) in ((65, 68, 72), (192, 192, 192), (1, 8, 8))
            for epi in ("affine", "swish") for ob in (False, True)]


def control_cases():
    """The GPU negative controls: launched without the bias / the mask / with alpha = 1."""
    return [Case("sbk_gemm", True, 2, 65, 68, 72, "affine", ob, seed=9) for ob in (False, True)]


def ln_error_case(inst):
    bf16, tile, _, BK = LN_INST[inst]
    return Case("sbk_gemm_ln", bf16, tile, 33, 256, BK, "affine", False, seed=40 + tile)


def tn_error_case(tile):
    return Case("sbk_gemm_tn_cfg", True, tile, 72, 56, 65, nsplit=2, layout="strided", seed=60 + tile)


def wrapper_cases():
    """_enc.gemm on unaligned views and at K = 10; _enc.gemm_tn_into with 4 head blocks."""
    return {"views": Case("sbk_gemm", True, 0, 65, 72, 8, "none", seed=11),
            "k10-bf16": Case("sbk_gemm", True, 0, 33, 40, 10, "none", seed=12),
            "k10-fp32": Case("sbk_gemm", False, 0, 33, 40, 10, "none", seed=12),
            "tn_into-bf16": Case("sbk_gemm_tn", True, 0, 72, 16, 129, batch=4, seed=13),
            "tn_into-fp32": Case("sbk_gemm_tn", False, 0, 72, 16, 129, batch=4, seed=13)}


def all_cases():
    """Every case test_gpu_gemm_tiles.py launches, keyed by its parametrised test id."""
    groups = {}
    for t in TILES_BF16:
        groups[f"gemm-bf16-{t}"] = gemm_cases(True, t)
    for t in TILES_F32:
        groups[f"gemm-fp32-{t}"] = gemm_cases(False, t)
    for inst in LN_INST:
        groups[f"gemm_ln-{inst}"] = gemm_ln_cases(inst)
    for bf in (True, False):
        groups[f"batched-{'bf16' if bf else 'fp32'}"] = batched_cases(bf)
    for t in (64, 128):
        groups[f"tn-{t}"] = tn_cases(t)
    groups["tn-auto"] = tn_auto_cases()
    groups["tn-fp32"] = tn_f32_cases()
    groups["misc"] = (dispatch_cases(True) + dispatch_cases(False) + control_cases() + [ln_error_case(i) for i in LN_INST]
                      + [tn_error_case(t) for t in (64, 128)] + list(wrapper_cases().values()))
    return groups


# ---------------------------------------------------------------------------
# operands and references
# ---------------------------------------------------------------------------
def _ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g, dtype=torch.int64)


@functools.lru_cache(maxsize=32)
def _int_operands(kind, batch, M, N, K, seed):
    g = torch.Generator().manual_seed(((seed * 1009 + M) * 1013 + N) * 1019 + K + 7 * batch)
    if kind == "nt":     # A (batch, M, K) · W (batch, N, K)^T
        return {"A": _ints(g, batch, M, K), "W": _ints(g, batch, N, K), "bias": _ints(g, N), "res": _ints(g, M, N),
                "ln_g": _ints(g, N), "ln_b": _ints(g, N)}
    return {"A": _ints(g, batch, K, M), "B": _ints(g, batch, K, N), "C0": _ints(g, batch, M, N)}


@dataclasses.dataclass
class Operands:
    """fp32 CPU tensors holding the exact operand values, and the int64 product."""
    A: torch.Tensor
    W: torch.Tensor
    S: torch.Tensor                      # int64 A·W^T (or A^T·B), unscaled
    sum_abs: int                         # max over elements of sum |a||w|: bounds every partial sum
    bias: torch.Tensor = None
    res: torch.Tensor = None
    mask: torch.Tensor = None            # uint8 [M]
    alpha: float = 1.0
    wscale: float = 1.0
    C0: torch.Tensor = None
    ln_g: torch.Tensor = None
    ln_b: torch.Tensor = None


@functools.lru_cache(maxsize=32)
def _product(kind, batch, M, N, K, seed):
    """int64 product of the integer operands, and max sum |a||w| (exact in float64, and quick)."""
    io = _int_operands(kind, batch, M, N, K, seed)
    if kind == "tn":
        A, B = io["A"], io["B"]
        return A.transpose(1, 2) @ B, int((A.abs().double().transpose(1, 2) @ B.abs().double()).max())
    A, W = io["A"], io["W"]
    return A @ W.transpose(1, 2), int((A.abs().double() @ W.abs().double().transpose(1, 2)).max())


def operands(case):
    tn = case.entry.startswith("sbk_gemm_tn")
    key = ("tn" if tn else "nt", case.batch, case.M, case.N, case.K, case.seed)
    io = _int_operands(*key)
    S, sa = _product(*key)
    if tn:
        return Operands(io["A"].float(), io["B"].float(), S, sa, C0=io["C0"].float())
    A, W = io["A"], io["W"]
    ws = 1.0 / 64 if case.scaled else 1.0
    o = Operands(A.float(), W.float() * ws, S, sa, wscale=ws)
    if case.entry == "sbk_gemm_batched":
        return o
    o.A, o.W, o.S = o.A[0], o.W[0], S[0]
    if case.epi != "none":
        o.bias = io["bias"].float() * (0.25 if case.scaled else 1.0)
        o.res = io["res"][:, :case.nout].float().contiguous()
        o.mask = torch.zeros(case.M, dtype=torch.uint8)
        o.mask[list(case.mask_rows())] = 1
        o.alpha = ALPHA
    if case.entry == "sbk_gemm_ln":
        o.res[case.M // 2] = 3.0          # masked row, constant residual: variance exactly zero
        o.ln_g = io["ln_g"].float() * 0.25
        o.ln_b = io["ln_b"].float() * 0.25
    return o


def probe_conditions(case, o=None):
    """The three conditions the exactness argument rests on."""
    o = o or operands(case)
    rt = all(torch.equal(t.to(torch.bfloat16).float(), t) for t in (o.A, o.W))
    Af, Wf = o.A, o.W / o.wscale
    if case.entry.startswith("sbk_gemm_tn"):
        f32 = Af.transpose(-1, -2) @ Wf
    else:
        f32 = Af @ Wf.transpose(-1, -2)
    return {"bf16_round_trip": rt, "sum_abs": o.sum_abs, "fp32_equals_int64": torch.equal(f32.double(), o.S.double())}


def glu_split(x):
    """[value16 | gate16] column groups of the pre-activation -> (value, gate), each (M, N / 2)."""
    M, N = x.shape
    v = x.view(M, N // 32, 2, 16)
    return v[:, :, 0].reshape(M, N // 2), v[:, :, 1].reshape(M, N // 2)


def epilogue(pre, epi, bias, res, mask, alpha, dtype=torch.float64, alpha_after_res=False):
    """The fused epilogue of sbk_gemm in `dtype` on the pre-activation `pre`:
    bias, activation, row mask, alpha, residual."""
    x = pre.to(dtype)
    if bias is not None:
        x = x + bias.to(dtype)
    if epi == "lrelu":
        x = torch.where(x >= 0, x, x * SLOPE)
    elif epi == "swish":
        x = x * torch.sigmoid(x)
    elif epi == "gelu":
        x = 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    elif epi == "glu":
        a, g = glu_split(x)
        x = a * torch.sigmoid(g)
    if mask is not None:
        x = torch.where(mask.bool()[:, None], torch.zeros((), dtype=dtype), x)
    if alpha_after_res:
        return (x + (res.to(dtype) if res is not None else 0)) * alpha
    x = x * alpha
    if res is not None:
        x = x + res.to(dtype)
    return x


def layernorm(x, g, b, dtype=torch.float64):
    if dtype == torch.float32:
        return torch.nn.functional.layer_norm(x.float(), x.shape[-1:], g.float(), b.float(), LN_EPS)
    x = x.to(dtype)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + LN_EPS) * g.to(dtype) + b.to(dtype)


def rel_bound(ref64, ref32):
    """max(1e-5, 8 E32), E32 = the error of the same epilogue in fp32 torch on
    the CPU, both relative to max(1, |ref|_inf)."""
    scale = max(1.0, float(ref64.abs().max()))
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    return max(1e-5, 8 * e32), e32


def reference(case, o=None):
    """-> (ref, rel): exact cases rel is None and ref is the fp32 tensor every
    bit of which the kernel must reproduce (cast to bf16 for a bf16 output);
    inexact cases ref is float64 and rel the relative bound."""
    o = o or operands(case)
    if case.entry.startswith("sbk_gemm_tn"):
        return (o.C0.double() + o.S.double()).float(), None
    pre = o.S.double() * o.wscale
    if case.entry == "sbk_gemm_batched":
        return pre.float(), None
    r64 = epilogue(pre, case.epi, o.bias, o.res, o.mask, o.alpha)
    if case.epi in INEXACT:
        r32 = epilogue(pre, case.epi, o.bias, o.res, o.mask, o.alpha, torch.float32)
        return r64, rel_bound(r64, r32)[0]
    assert torch.equal(r64.float().double(), r64)
    return r64.float(), None


def reference_ln(case, o=None):
    """sbk_gemm_ln: (out exact fp32, u float64, relative bound of u)."""
    o = o or operands(case)
    out, _ = reference(case, o)
    u64 = layernorm(out, o.ln_g, o.ln_b)
    return out, u64, rel_bound(u64, layernorm(out, o.ln_g, o.ln_b, torch.float32))[0]


# ---------------------------------------------------------------------------
# checker
# ---------------------------------------------------------------------------
def mismatch(got, want):
    """Bitwise comparison of two 2-D tensors of one dtype: (number of
    mismatching elements, first mismatching (row, column) or None)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    iv = {4: torch.int32, 2: torch.int16, 8: torch.int64}[got.element_size()]
    bad = got.contiguous().view(iv) != want.contiguous().view(iv)
    n = int(bad.sum())
    return n, (tuple(bad.nonzero()[0].tolist()) if n else None)


def excess(got, ref64, rel, bf16_out):
    """Inexact comparison: (count over the bound, first (row, column), worst
    |err| / max(1, |ref|_inf) after the bf16 half-ulp allowance)."""
    scale = max(1.0, float(ref64.abs().max()))
    err = (got.double() - ref64).abs()
    slack = ref64.abs() * 2.0 ** -8 if bf16_out else torch.zeros_like(ref64)
    bad = ~(err <= rel * scale + slack)     # a NaN counts as bad
    n = int(bad.sum())
    worst = float(torch.nan_to_num((err - slack).clamp_min(0), nan=float("inf")).max()) / scale
    return n, (tuple(bad.nonzero()[0].tolist()) if n else None), worst


def check(case, got, ref, rel=None):
    """-> (count, first, worst): the exact or the bounded comparison of one case's output."""
    if rel is None:
        want = ref.to(got.dtype)
        n, first = mismatch(got, want)
        return n, first, 0.0
    return excess(got, ref, rel, got.dtype == torch.bfloat16)


def describe(case, what, n, first, got, ref):
    r, c = first
    return (f"{case}: {what}: {n} of {got.numel()} elements wrong, first at (row {r}, column {c}): "
            f"got {float(got[r, c])!r}, want {float(ref[r, c])!r}")


# ---------------------------------------------------------------------------
# guard-banded buffers (any device)
# ---------------------------------------------------------------------------
def place(t, strides, dev, fill, off=0, shape=None, dtype=None):
    """A fresh 1-D buffer on `dev` filled with `fill`, and the strided view of
    it that starts PAD + off elements in; `t` (or nothing, for an output) is
    copied into the view.  The buffer reaches PAD elements before the view and
    one leading dimension plus PAD past its last element, so the columns
    [N, ld) of every row are inside it.  -> (buffer, view)"""
    shape = tuple(t.shape) if t is not None else tuple(shape)
    dtype = dtype or t.dtype
    span = sum((s - 1) * st for s, st in zip(shape, strides)) + 1
    size = PAD + off + span + max(strides) + PAD
    buf = torch.full((size,), fill, dtype=dtype, device=dev)
    view = buf.as_strided(shape, tuple(strides), PAD + off)
    if t is not None:
        view.copy_(t.to(dtype))
    return buf, view


def outside_untouched(buf, view, fill):
    """Every element of `buf` that is not an element of `view` still holds `fill`."""
    b = buf.cpu()
    inside = torch.zeros(b.numel(), dtype=torch.bool)
    inside.as_strided(tuple(view.shape), tuple(view.stride()), view.storage_offset()).fill_(True)
    return bool((b[~inside] == fill).all())
