"""Exact block-scaled probes for the MXFP8 GEMM kernels (mx_gemm_kernel and
mx_gemm256_kernel of csrc/mxgemm.hip, gemm256_kernel<true, ...> and
splitk_epi_kernel of csrc/gemm256.hip): the case lists, the raw byte
operands, the references, the independent MXFP8 quantiser and the checker
shared by test_mx_ref_cpu.py and test_gpu_mx_tiles.py.

Operands are built on the CPU as bytes, never through mx_quant: e4m3 codes of
the integers in [-4, 4] (all exact in e4m3fn) and E8M0 scale bytes chosen per
(row, 32-block).  Three families:

  F  flat: one scale byte for all of A and one for all of W, dense integers,
     K <= 2048, so |sum| <= 16 K <= 2^15 units of one power of two;
  B  one block: row m of A is non-zero in the single 32-block m % (K / 32)
     (the rest +-0 codes), W dense, and every scale byte differs from its
     neighbours (SA = 127 + (3m + 5b) % 7 - 3, SW = 120 + (2n + 3b) % 7 - 3:
     adjacent blocks, rows 32 / 64 / 128 apart and SA against SW all differ).
     An output is one 32-term integer sum times one power of two, exact
     whatever the MFMA's internal alignment does, and any wrong scale pick is
     off by a factor >= 2.  BT is the same with the roles of A and W swapped;
  X  mixed: dense operands under the B scale pattern.  The sum is exact in
     fp32 arithmetic (probe_conditions: < 2^24 units); the MFMA's own
     accumulation measured exact there too (test_gpu_mx_tiles.py), so it is
     compared bit for bit as well.
  E  quantiser edges: A is all +-0 codes, so the value is the fp32 residual,
     crafted block by block (edge_blocks).

The reference of every family is one float64 matmul of the dequantised
operands: every product is a multiple of the smallest unit and the sums stay
below 2^53 units, so it is exact.  The exact epilogue (integer bias in
[-8, 8], ReLU, alpha = 0.5, integer residual) keeps it representable in fp32
(asserted), so fp32 outputs are compared bit for bit, bf16 outputs with
ref.to(bfloat16) bit for bit and MXFP8 outputs byte for byte and scale byte
for scale byte with mx_quantise(ref).  GELU lowers the W scale bytes by 6
(pre-activations O(1)) and is compared with float64 GELU on the exact
pre-activation under gemm_ref's rule max(1e-5, 8 E32).

No GPU is needed to import this module."""
import dataclasses
import functools
import math

import torch
import torch.nn.functional as F

from gemm_ref import PAD, SBK_ERR_ARG, SENTINEL, excess, mismatch, outside_untouched, place, rel_bound  # noqa: F401

NAN8 = 0x7F            # e4m3fn NaN code: operand guard bands, byte-output sentinel
NANS = 0xFF            # E8M0 NaN code: scale guard bands, scale-output sentinel
ALPHA = 0.5
ACT_NONE, ACT_RELU, ACT_GELU = 0, 3, 4
ACTS = (ACT_NONE, ACT_RELU, ACT_GELU)
OUT_F32, OUT_BF16, OUT_MX = 0, 1, 2
OUTS = (OUT_F32, OUT_BF16, OUT_MX)
KERNELS = ("k128", "k256x128", "k256")   # mx_gemm_kernel, mx_gemm256_kernel, gemm256_kernel<true>
FLAT = ((127, 124), (130, 121))
SW_BASE = 120
GELU_SHIFT = 6
ROWS_PAST_M = 4        # sentinel rows below every output

_INT_CODE = torch.tensor([0x00, 0x38, 0x40, 0x44, 0x48], dtype=torch.uint8)


def expected_kernel(M, N):
    """The dispatch rule of sbk_mx_gemm (mxgemm.hip)."""
    if N % 256 == 0 and ((M + 255) // 256) * (N // 256) >= 180:
        return "k256"
    return "k256x128" if M >= 4096 else "k128"


@dataclasses.dataclass(frozen=True)
class Case:
    kernel: str                # which kernel must run it ("k256": sbk_mx_gemm256 called directly)
    fam: str                   # F, B, BT, X, E
    M: int
    N: int
    K: int
    act: int = ACT_NONE
    out: int = OUT_F32
    epi: bool = False          # bias, alpha = 0.5 and (res) the residual
    res: bool = True
    flat: int = 0              # F / E: index into FLAT
    conv: tuple = None         # (B, T_in, C, k, stride): A rows are overlapping windows of (B * T_in, C)
    seed: int = 0
    entry: str = None          # override the entry point (the dispatch-boundary and split-K tests)

    @property
    def entry_point(self):
        return self.entry or ("sbk_mx_gemm256" if self.kernel == "k256" else "sbk_mx_gemm")

    @property
    def gelu(self):
        return self.act == ACT_GELU

    @property
    def has_bias(self):
        return self.epi and self.fam != "E"

    @property
    def has_res(self):
        return self.fam == "E" or (self.epi and self.res)

    @property
    def alpha(self):
        return ALPHA if (self.epi or self.fam == "E") else 1.0

    def __str__(self):
        s = (f"{self.entry_point} [{self.kernel}] family {self.fam} M={self.M} N={self.N} K={self.K} act={self.act} "
             f"out_mode={self.out} epilogue={'yes' if self.epi else 'no'}{'' if self.res else ' (no res)'}")
        if self.fam in ("F", "E"):
            s += f" scales={FLAT[self.flat]}"
        if self.conv:
            s += f" conv(B, T_in, C, k, stride)={self.conv}"
        return s


def conv_case(kernel, fam, B, T_in, C, k, stride, N, **kw):
    T_out = (T_in - k) // stride + 1
    return Case(kernel, fam, B * T_out, N, k * C, conv=(B, T_in, C, k, stride), **kw)


# ---------------------------------------------------------------------------
# case lists
# ---------------------------------------------------------------------------
INST_SHAPE = {"k128": (129, 128, 256), "k256x128": (4097, 128, 256), "k256": (257, 256, 256)}
SHAPES = {
    "k128": [(M, N, K) for K in (128, 256, 384, 512) for M in (1, 127, 128, 129, 257) for N in (128, 384)]
            + [(512, 256, 256), (384, 256, 256)],                       # nt % 8 == 0 (XCD remap) and nt = 6
    "k256x128": [(M, N, K) for K in (128, 256, 384, 512, 896) for M in (4096, 4097, 4351) for N in (128, 1024)],
    "k256": [(M, N, K) for K in (128, 256, 384) for M in (1, 255, 256, 257, 513, 2305) for N in (256, 512)],
}
MIXED_SHAPES = {"k128": [(129, 128, 128), (257, 384, 512), (128, 128, 384)],
                "k256x128": [(4097, 128, 384), (4096, 128, 896)],
                "k256": [(257, 256, 128), (513, 512, 384)]}
CONV = {"k128": (3, 201, 128, 3, 2, 128), "k256x128": (3, 2801, 128, 3, 2, 128), "k256": (3, 201, 128, 3, 2, 256)}
SPLIT_SHAPE = (17820, 1024, 2048)


def instantiation_cases(kernel, act, out):
    """The cases of one (kernel, ACT, OUT) instantiation: every family with the
    full epilogue at a shape of two row tiles, the second of one row; with an
    exact activation and MXFP8 out also the quantiser edges."""
    M, N, K = INST_SHAPE[kernel]
    s = 100 + 10 * act + out
    fams = ("F", "X") if act == ACT_GELU else ("F", "B", "BT")
    cases = [Case(kernel, f, M, N, K, act, out, epi=True, flat=i & 1, seed=s) for i, f in enumerate(fams)]
    if act == ACT_RELU:  # ReLU alone, no residual: the zeros of the negative half keep their sign bit clear
        cases.append(Case(kernel, "F", M, N, K, act, out, epi=True, res=False, flat=1, seed=s + 1))
    if act != ACT_GELU and out == OUT_MX:
        Me = len(edge_blocks()) * 2 + 1
        cases.append(Case(kernel, "E", Me if kernel != "k256x128" else 4096 + Me, N, 128, act, out, seed=s))
    return cases


def shape_cases(kernel, K):
    """The shape table of one kernel at one K: F on every shape (both flat
    scale pairs in turn), B or BT in turn, the output modes in turn."""
    cases = []
    for i, (M, N, k) in enumerate(s for s in SHAPES[kernel] if s[2] == K):
        cases.append(Case(kernel, "F", M, N, k, out=OUTS[i % 3], flat=i & 1, seed=K + i))
        cases.append(Case(kernel, ("B", "BT")[i & 1], M, N, k, out=OUTS[(i + 1) % 3], seed=K + i))
    return cases


def shape_ks(kernel):
    return sorted({s[2] for s in SHAPES[kernel]})


def mixed_cases(kernel):
    return [Case(kernel, "X", M, N, K, seed=7 + i) for i, (M, N, K) in enumerate(MIXED_SHAPES[kernel])]


def conv_cases(kernel):
    B, T_in, C, k, stride, N = CONV[kernel]
    return [conv_case(kernel, fam, B, T_in, C, k, stride, N, out=OUTS[i % 3], seed=30 + i)
            for i, fam in enumerate(("F", "B", "BT"))]


def dispatch_cases():
    """180 tiles of 256 x 256: sbk_mx_gemm runs the multi-phase kernel; 176: the 256 x 128 one."""
    return {"at": Case("k256", "F", 11520, 1024, 128, flat=1, seed=41, entry="sbk_mx_gemm"),
            "at-direct": Case("k256", "F", 11520, 1024, 128, flat=1, seed=41),
            "below": Case("k256x128", "F", 11264, 1024, 128, flat=1, seed=42)}


def split_cases():
    M, N, K = SPLIT_SHAPE
    return [Case("k256", "F", M, N, K, ACT_RELU, OUT_F32, epi=True, res=r, seed=50 + r, entry="sbk_mx_gemm_ws")
            for r in (True, False)]


def error_case(entry):
    k = "k256" if entry == "sbk_mx_gemm256" else "k128"
    return Case(k, "F", 129, 256, 128, ACT_NONE, OUT_MX, epi=True, seed=60, entry=entry)


def all_cases():
    """Every case test_gpu_mx_tiles.py launches, keyed by its test id."""
    g = {}
    for kern in KERNELS:
        for act in ACTS:
            for out in OUTS:
                g[f"inst-{kern}-{act}-{out}"] = instantiation_cases(kern, act, out)
        for K in shape_ks(kern):
            g[f"shapes-{kern}-{K}"] = shape_cases(kern, K)
        g[f"mixed-{kern}"] = mixed_cases(kern)
        g[f"conv-{kern}"] = conv_cases(kern)
    g["dispatch"] = list(dispatch_cases().values())
    g["split"] = split_cases()
    g["errors"] = [error_case(e) for e in ("sbk_mx_gemm", "sbk_mx_gemm256", "sbk_mx_gemm_ws")]
    return g


# ---------------------------------------------------------------------------
# e4m3 / E8M0 codes
# ---------------------------------------------------------------------------
def encode_ints(t, neg_zero=None):
    """int64 in [-4, 4] -> e4m3fn bytes; zeros take the sign bit where neg_zero is set."""
    b = _INT_CODE[t.abs()]
    sign = t < 0
    if neg_zero is not None:
        sign = sign | ((t == 0) & neg_zero)
    return b | (sign.to(torch.uint8) << 7)


@functools.lru_cache(maxsize=1)
def e4m3_table():
    """float64 value of every e4m3fn code (0x7F and 0xFF: NaN), from the format's definition."""
    v = []
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        x = m * 2.0 ** -9 if e == 0 else (float("nan") if (e == 15 and m == 7) else (1 + m / 8) * 2.0 ** (e - 7))
        v.append(-x if c & 0x80 else x)
    return torch.tensor(v, dtype=torch.float64)


def decode(q, s):
    """e4m3 bytes (R, K) and E8M0 bytes (R, K / 32) -> float64 values."""
    return e4m3_table()[q.long()] * torch.exp2(s.double() - 127).repeat_interleave(32, dim=1)


def scale_bytes(am):
    """E8M0 byte of the smallest power of two 2^E with amax / 2^E <= 448, by
    integer arithmetic on frexp(amax): amax = m 2^e, 448 = 0.875 2^9, so
    E = e - 9, plus 1 when m > 0.875 (8 m > 7); an all-zero block takes byte 0."""
    m, e = torch.frexp(am.double())
    E = (e.long() - 9 + (m * 8 > 7).long()).clamp(-127, 127)
    return torch.where(am > 0, E + 127, torch.zeros_like(E)).to(torch.uint8)


def scale_byte_scalar(am):
    """scale_bytes for one Python float, through math.frexp (pins the tensor version)."""
    if not am > 0:
        return 0
    m, e = math.frexp(am)
    return max(-127, min(127, e - 9 + (1 if m * 8 > 7 else 0))) + 127


def e4m3_bytes(q, truncate=False):
    """float64 values already scaled into [-448, 448] -> e4m3fn bytes, RNE
    (torch.float8_e4m3fn; the float32 step is exact for the probes' values).
    truncate: round towards zero instead — a modelled wrong kernel."""
    q = q.clamp(-448, 448)
    if not truncate:
        assert torch.equal(q.float().double(), q)
        return q.float().to(torch.float8_e4m3fn).view(torch.uint8)
    tab = e4m3_table()[:0x7F]                      # the non-negative codes, ascending
    idx = torch.searchsorted(tab, q.abs().contiguous(), right=True) - 1
    return idx.to(torch.uint8) | ((torch.signbit(q)).to(torch.uint8) << 7)


def mx_quantise(v, scale_off=None, truncate=False):
    """The MXFP8 quantisation of an (M, N) matrix along its rows, blocks of 32:
    -> (e4m3 bytes (M, N), E8M0 bytes (M, N / 32)).  Independent of the
    kernels and of oracle.wav2vec.mx_round (test_mx_ref_cpu.py pins the two
    to each other).  scale_off(sb, am) -> sb models a wrong scale byte."""
    M, N = v.shape
    x = v.double().reshape(M, N // 32, 32)
    am = x.abs().amax(-1)
    sb = scale_bytes(am)
    if scale_off is not None:
        sb = scale_off(sb, am)
    q = torch.ldexp(x, (127 - sb.long())[..., None].expand_as(x))
    return e4m3_bytes(q, truncate).reshape(M, N), sb


def dequantise(q, sb):
    return decode(q, sb)


# ---------------------------------------------------------------------------
# quantiser edge blocks (family E)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def edge_blocks():
    """-> list of (name, 32 fp32 values): one 32-column output block each."""
    f32 = torch.float32
    up = lambda x: float(torch.nextafter(torch.tensor(x, dtype=f32), torch.tensor(float("inf"), dtype=f32)))
    dn = lambda x: float(torch.nextafter(torch.tensor(x, dtype=f32), torch.tensor(0.0, dtype=f32)))
    small = [((i * 7) % 13 - 6) * 0.25 for i in range(32)]
    blocks = [("zero", [0.0] * 32), ("zero-signed", [-0.0 if i & 1 else 0.0 for i in range(32)])]
    for k in (-3, 0, 5):
        a = 448.0 * 2.0 ** k
        for name, top in (("at", a), ("above", up(a)), ("below", dn(a)), ("neg-at", -a), ("neg-above", -up(a))):
            for lane in (0, 31):
                v = [s * 2.0 ** k for s in small]
                v[lane] = top
                blocks.append((f"448*2^{k} {name} lane {lane}", v))
    # RNE ties: amax 256 * 2^k (mantissa 0.5: E = k), q = v / 2^k half way between two codes
    ties = [17.0, 19.0, -21.0, 2.125, 2.375, -2.625, 216.0, -200.0, 2.0 ** -10, 3 * 2.0 ** -10, -5 * 2.0 ** -10,
            2.0 ** -11, 0.0068359375, 1.0625, 1.1875, 208.0, 0.2578125, -0.2734375]
    for k in (-7, 0, 4):
        for lane in (0, 31):
            v = [0.0] * 32
            free = [i for i in range(32) if i != lane]
            for i, t in zip(free, ties):
                v[i] = t * 2.0 ** k
            v[lane] = -256.0 * 2.0 ** k if lane else 256.0 * 2.0 ** k
            blocks.append((f"ties 2^{k} amax lane {lane}", v))
    return [(n, torch.tensor(v, dtype=f32)) for n, v in blocks]


def edge_residual(M, N):
    """The E family's residual: block j of row r holds edge block
    (r + 5 j) % len, so with M >= len rows every edge block sits in every
    column-block position."""
    eb = torch.stack([v for _, v in edge_blocks()])
    r, j = torch.arange(M)[:, None], torch.arange(N // 32)[None, :]
    return eb[(r + 5 * j) % len(eb)].reshape(M, N)


# ---------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class Operands:
    X: torch.Tensor            # A's bytes as stored: (M, K), or the conv input (B * T_in, C)
    SX: torch.Tensor           # its scale bytes
    W: torch.Tensor            # (N, K) bytes
    SW: torch.Tensor           # (N, K / 32)
    bias: torch.Tensor = None  # fp32 [N]
    res: torch.Tensor = None   # fp32 [M, N]


def pattern_sa(rows, nb):
    m, b = torch.arange(rows)[:, None], torch.arange(nb)[None, :]
    return (127 + (3 * m + 5 * b) % 7 - 3).to(torch.uint8)


def pattern_sw(rows, nb, base=SW_BASE):
    n, b = torch.arange(rows)[:, None], torch.arange(nb)[None, :]
    return (base + (2 * n + 3 * b) % 7 - 3).to(torch.uint8)


def _dense(g, rows, K):
    return torch.randint(-4, 5, (rows, K), generator=g, dtype=torch.int64)


def _one_block(g, rows, K, active=None):
    """Row r non-zero (no zero element) in block r % (K / 32) only; +-0 codes elsewhere."""
    nb = K // 32
    t = torch.zeros(rows, nb, 32, dtype=torch.int64)
    mag = torch.randint(1, 5, (rows, 32), generator=g) * (torch.randint(0, 2, (rows, 32), generator=g) * 2 - 1)
    r = torch.arange(rows)
    blk = r % nb if active is None else active
    t[r, blk] = mag
    return t.reshape(rows, K)


def a_rows(case):
    """Conv addressing: (M, k) indices of the input rows each A row concatenates."""
    B, T_in, C, k, stride = case.conv
    T_out = (T_in - k) // stride + 1
    m = torch.arange(case.M)
    start = (m // T_out) * T_in + (m % T_out) * stride
    return start[:, None] + torch.arange(k)[None, :]


@functools.lru_cache(maxsize=6)
def _operands(fam, M, N, K, flat, gelu, conv, seed, has_bias, has_res):
    g = torch.Generator().manual_seed((((seed * 1009 + M) * 1013 + N) * 1019 + K) * 7 + len(fam))
    shift = GELU_SHIFT if gelu else 0
    if conv:
        B, T_in, C, k, stride = conv
        xr, xk = B * T_in, C
    else:
        xr, xk = M, K
    nz = torch.randint(0, 2, (xr, xk), generator=g).bool()
    if fam in ("F", "BT", "X"):
        xi = _dense(g, xr, xk)
    elif fam == "E":
        xi = torch.zeros(xr, xk, dtype=torch.int64)
    elif conv:  # B under overlapping windows: only the input rows a single window owns (tap 1 of k 3, stride 2)
        assert (k, stride) == (3, 2)
        j = torch.arange(xr) % T_in
        own = (j % 2 == 1) & (j < 2 * ((T_in - k) // stride + 1))
        xi = _one_block(g, xr, xk, active=(torch.arange(xr) // 2) % (xk // 32)) * own[:, None]
    else:
        xi = _one_block(g, xr, xk)
    wi = _one_block(g, N, K) if fam == "BT" else _dense(g, N, K)
    X = encode_ints(xi, nz)
    W = encode_ints(wi, torch.randint(0, 2, (N, K), generator=g).bool())
    if fam in ("F", "E"):
        sa, sw = FLAT[flat]
        SX = torch.full((xr, xk // 32), sa, dtype=torch.uint8)
        SWt = torch.full((N, K // 32), sw - shift, dtype=torch.uint8)
    else:
        SX, SWt = pattern_sa(xr, xk // 32), pattern_sw(N, K // 32, SW_BASE - shift)
    o = Operands(X, SX, W, SWt)
    if has_bias:
        o.bias = torch.randint(-8, 9, (N,), generator=g).float() * (0.25 if gelu else 1.0)
    if fam == "E":
        o.res = edge_residual(M, N)
    elif has_res:
        o.res = torch.randint(-8, 9, (M, N), generator=g).float()
    return o


def operands(case):
    return _operands(case.fam, case.M, case.N, case.K, case.flat, case.gelu, case.conv, case.seed, case.has_bias,
                     case.has_res)


def gemm_a(case, o):
    """A as the GEMM sees it: (bytes (M, K), scale bytes (M, K / 32))."""
    if not case.conv:
        return o.X, o.SX
    idx = a_rows(case)
    return o.X[idx].reshape(case.M, case.K), o.SX[idx].reshape(case.M, case.K // 32)


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
def product(case, o, rows=None, cols=None, wrong=None):
    """float64 A · W^T of the dequantised operands, exact (module docstring);
    rows / cols restrict it.  wrong: a modelled wrong kernel (see wrong_product)."""
    Aq, SA = gemm_a(case, o)
    Wq, SW = o.W, o.SW
    if rows is not None:
        Aq, SA = Aq[rows], SA[rows]
    if cols is not None:
        Wq, SW = Wq[cols], SW[cols]
    if wrong is not None:
        Aq, SA, Wq, SW = wrong_operands(wrong, Aq, SA, Wq, SW)
    return decode(Aq, SA) @ decode(Wq, SW).t()


def conv_product(case, o):
    """The same product by an integer-valued conv1d over the stored input
    (float64, exact): the reference of the conv-addressing cases."""
    B, T_in, C, k, stride = case.conv
    x = decode(o.X, o.SX).view(B, T_in, C).transpose(1, 2)
    w = decode(o.W, o.SW).view(case.N, k, C).transpose(1, 2)
    return F.conv1d(x, w, stride=stride).transpose(1, 2).reshape(case.M, case.N)


def sum_abs(case, o):
    """sum |a| |w| of every output (float64, exact): bounds every partial sum."""
    Aq, SA = gemm_a(case, o)
    return decode(Aq, SA).abs() @ decode(o.W, o.SW).abs().t()


def unit(case, o):
    """The power of two every product of the case is a multiple of."""
    return 2.0 ** (int(o.SX.min()) + int(o.SW.min()) - 254)


def epilogue(pre, case, o, dtype=torch.float64, rows=None, cols=None, alpha_first=False, res_scaled=False):
    """res + alpha * act(pre + bias) in `dtype`; the two flags model wrong kernels."""
    x = pre.to(dtype)
    if o.bias is not None:
        x = x + (o.bias if cols is None else o.bias[cols]).to(dtype)
    if alpha_first:
        x = x * case.alpha
    if case.act == ACT_RELU:
        x = torch.relu(x)
    elif case.act == ACT_GELU:
        x = 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    if not alpha_first:
        x = x * case.alpha
    if o.res is not None:
        r = o.res if rows is None else o.res[rows]
        r = (r if cols is None else r[:, cols]).to(dtype)
        x = x + (r * case.alpha if res_scaled else r)
    return x


@functools.lru_cache(maxsize=4)
def _reference(case):
    o = operands(case)
    pre = conv_product(case, o) if case.conv else product(case, o)
    r64 = epilogue(pre, case, o)
    if case.gelu:
        return r64, rel_bound(r64, epilogue(pre, case, o, torch.float32))[0]
    assert torch.equal(r64.float().double(), r64), f"{case}: the exact epilogue is not representable in fp32"
    return r64.float(), None


def reference(case):
    """-> (ref, rel): exact cases ref is the fp32 tensor the kernel must
    reproduce bit for bit (cast to bf16, or quantised by mx_quantise, for the
    other output modes) and rel is None; GELU: ref float64 and the bound."""
    return _reference(case)


def probe_conditions(case, o=None, full=True):
    """The conditions the exactness argument rests on.  The sum bound is 16 K
    (F) and 512 (B, BT) units by construction; for X it is computed."""
    o = o or operands(case)
    codes_ok = bool(((o.X & 0x7F) <= 0x48).all() and ((o.W & 0x7F) <= 0x48).all())
    if case.fam in ("F", "E"):
        units = 16 * case.K
    elif case.fam in ("B", "BT"):
        units = 16 * 32          # one block: 32 products of at most 16 units of that block's power of two
    else:
        units = float(sum_abs(case, o).max()) / unit(case, o)
    return {"codes": codes_ok, "sum_units": units}


# ---------------------------------------------------------------------------
# modelled wrong kernels (applied to the reference on the CPU)
# ---------------------------------------------------------------------------
WRONG_PRODUCT = ("block^1", "row^32", "sw_from_sa", "halves_swapped", "ktile_skipped", "ktile_twice")


def wrong_operands(kind, Aq, SA, Wq, SW):
    M, K = Aq.shape
    nb = K // 32
    if kind == "block^1":           # the scale of block b taken from b ^ 1
        return Aq, SA[:, torch.arange(nb) ^ 1], Wq, SW
    if kind == "row^32":            # the A scale of row r taken from r ^ 32
        r = (torch.arange(M) ^ 32).clamp(max=M - 1)
        return Aq, SA[r], Wq, SW
    if kind == "sw_from_sa":        # W scales read from SA
        r = torch.arange(Wq.shape[0]).clamp(max=M - 1)
        return Aq, SA, Wq, SA[r]
    if kind == "halves_swapped":    # A's two 16-B halves of a block swapped between the lane halves
        return Aq.view(M, nb, 2, 16).flip(2).reshape(M, K), SA, Wq, SW
    if kind == "ktile_skipped":     # the last K-tile never accumulated
        Aq = Aq.clone()
        Aq[:, K - 128:] = 0
        return Aq, SA, Wq, SW
    if kind == "ktile_twice":       # a stale ring stage: K-tile 0 in place of the last one
        Aq, SA = Aq.clone(), SA.clone()
        Aq[:, K - 128:] = Aq[:, :128]
        SA[:, nb - 4:] = SA[:, :4]
        return Aq, SA, Wq, SW
    raise ValueError(kind)


def rows_stored_past_m(ref, tile_rows):
    """The last row tile's rows shifted down by one (the first of them left
    unwritten, the last stored past M): -> the (M + 1, N) buffer such a
    kernel leaves in a sentinel-filled output."""
    M = ref.shape[0]
    m0 = (M - 1) // tile_rows * tile_rows
    buf = torch.full((M + 1, ref.shape[1]), SENTINEL, dtype=ref.dtype)
    buf[:m0] = ref[:m0]
    buf[m0 + 1:] = ref[m0:]
    return buf


# ---------------------------------------------------------------------------
# checker
# ---------------------------------------------------------------------------
def ratio_to_sum_abs(got, ref64, sabs):
    """max |got - ref| / sum |a b| (the X family's figure)."""
    return float(((got.double() - ref64).abs() / sabs.clamp_min(1e-300)).max())


def check(case, got, got_scales, ref, rel=None):
    """One launch's output against the reference -> list of failure strings.
    got: fp32 / bf16 values or e4m3 bytes (M, N); got_scales: E8M0 bytes
    (M, N / 32) for MXFP8 out.  A GELU case with MXFP8 out is checked by
    check_mx_of_fp32 instead."""
    fails = []

    def add(what, n, first, g, w):
        if n:
            r, c = first
            fails.append(f"{case}: {what}: {n} of {g.numel()} wrong, first at (row {r}, column {c}): "
                         f"got {g[r, c].item()!r}, want {w[r, c].item()!r}")

    if case.out == OUT_MX:
        assert rel is None
        wq, ws = mx_quantise(ref)
        add("e4m3 bytes", *mismatch_u8(got, wq), got, wq)
        add("scale bytes", *mismatch_u8(got_scales, ws), got_scales, ws)
        return fails
    if rel is None:
        want = ref.to(got.dtype)
        n, first = mismatch(got, want)
        add("out", n, first, got, want)
        return fails
    n, first, _ = excess(got, ref, rel, got.dtype == torch.bfloat16)
    add(f"out (bound {rel:.2e})", n, first, got, ref)
    return fails


def mismatch_u8(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.uint8, (got.shape, want.shape)
    bad = got != want
    n = int(bad.sum())
    return n, (tuple(bad.nonzero()[0].tolist()) if n else None)


def valid_codes(q, s=None):
    """No e4m3 NaN code among the bytes, no E8M0 NaN code among the scales."""
    ok = not bool(((q & 0x7F) == 0x7F).any())
    return ok and (s is None or not bool((s == NANS).any()))


# ---------------------------------------------------------------------------
# the 256 x 256 kernel's tile order (gemm256.hip tile_of, sbk_common.h xcd_tile)
# ---------------------------------------------------------------------------
def xcd_tile(nwg, orig):
    xcd, q8, r8 = orig & 7, nwg >> 3, nwg & 7
    return (xcd * (q8 + 1) if xcd < r8 else r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3)


def tile_of(orig, ntn, ntm):
    wg = xcd_tile(ntn * ntm, orig)
    gsz = 8 * ntn
    grp = wg // gsz
    first = grp * 8
    gm = min(8, ntm - first)
    i = wg - grp * gsz
    return first + i % gm, i // gm


def split_tail_tiles(M, N, K, cus):
    """The (row tile, column tile) list the split-K tail rule (gemm256.hip
    split_tail) runs as two K halves on a device of `cus` compute units."""
    ntn, ntm = N // 256, (M + 255) // 256
    nt = ntn * ntm
    tail = nt % cus
    if not (nt > cus and 0 < tail and 2 * tail <= cus and K // 128 >= 16):
        return []
    return [tile_of(i, ntn, ntm) for i in range(nt - tail, nt)]
