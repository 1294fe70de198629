"""The GEMM family (csrc/gemm.hip, csrc/gemm_tn.hip, the bf16 half of
csrc/gemm256.hip) tile by tile on exact integer probes (tests/gemm_ref.py).

Operands are integers in [-4, 4], so any correct fp32 accumulation order
gives the same bits and the int64 CPU matmul is the answer bit for bit, with
bias, alpha = 0.5, row mask, residual and LeakyReLU(0.25) on top (bf16
outputs: ref.to(bfloat16), bit for bit).  Swish, GELU, GLU and the row
LayerNorm are compared with their float64 evaluation on the exact
pre-activation under |err| / max(1, |ref|_inf) <= max(1e-5, 8 E32), plus
2^-8 |ref| per element for a bf16 output.  Every operand is a view into a
NaN-filled buffer (the row mask: 0xFF), every output a view into a buffer of
sentinels that reaches 64 elements either side and covers the columns
[N, ldc): the output must be finite and no sentinel may move.  The C ABI is
called directly so that ldc > N, misaligned pointers and leading dimensions
and the argument errors are reachable.

Instantiation -> test (tile ids and template arguments as in the switches):

  sbk_gemm bf16   1 launch<128,128,64>      2 launch<64,64,64>      3 launch<128,64,64>
                  4 launch<64,64,256,1>     5 launch<64,128,256,1>  6 launch<128,64,256,1>
                  7 launch<128,128,128,1>   8 launch<64,64,128>     9 launch<64,64,32>
                 10 launch<128,64,32>      17 launch<64,128,32>
                 11 launch_ring<128,128>   12 launch_ring<128,64>  13 launch_ring<64,64>
                 18 launch_pf<64,64,64>    19 launch_pf<128,64,64> 20 launch_pf<64,128,64>
                 21 launch_pf<128,128,64>  22 launch_pf<64,64,32>
                 30 gemm256_kernel<false, none / Swish / LeakyReLU / GELU, fp32 / bf16>
                                                          -> test_gemm_tile_bf16[<id>]
  sbk_gemm fp32   1 launch<float,128,128,32>  2 launch<float,64,64,32>  3 launch<float,128,64,32>
                                                          -> test_gemm_tile_fp32[<id>]
  sbk_gemm_ln     bf16 tile 0 launch<32,256,32>, 1 launch<32,256,64>, 2 launch<64,256,32>,
                  fp32 launch<float,32,256,32>            -> test_gemm_ln[<inst>]
  sbk_gemm_batched  launch<bf16,64,64,64> / launch<float,64,64,32> over grid.z
                                                          -> test_gemm_batched[bf16 / fp32]
  sbk_gemm_tn_cfg   gemm_tn_kernel<64,64> / <128,128>     -> test_gemm_tn_cfg[64 / 128]
  sbk_gemm_tn       (tile and split chosen)               -> test_gemm_tn_auto
  sbk_gemm_tn_f32   gemm_tn_f32_kernel, vector and element-wise loads -> test_gemm_tn_f32

Deviations from the shape table that the kernels' own argument rules force:
the LDS-DMA ring (tiles 11-13) takes only K % 64 == 0, K >= 192, so its K
column is 192 / 256 / 320 / 576; tile 30 takes only N % 256 == 0, K % 64 == 0
and aligned epilogue operands and has no GLU, so it runs its own M x N x K
grid and the GLU / misaligned-layout cases assert SBK_ERR_ARG there.  The
table's last row reaches K = 5 * 256 + 8 = 1288 on the BK = 256 tiles: sums
stay below 16 * 1288 < 2^15.  With exact probes every tile gives the same
bits, so these tests cannot tell which tile tile = 0 picked; the dispatch
thresholds are host arithmetic and out of scope.

Each test prints the worst error of its inexact epilogues against the bound."""
import ctypes
import dataclasses

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
_BF16, _F32 = torch.bfloat16, torch.float32


def _abi():
    from speechbrain_amd._lib import lib, ptr, stream_of
    return lib(), ptr, stream_of


def _vp(t, byte_off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + byte_off)


class Worst:
    """Worst error of the inexact epilogues of one test, printed against the bound."""

    def __init__(self, name):
        self.name, self.fig = name, {}

    def add(self, key, worst, rel):
        w, r = self.fig.get(key, (0.0, rel))
        self.fig[key] = (max(w, worst), min(r, rel))

    def report(self):
        for k, (w, r) in sorted(self.fig.items()):
            print(f"{self.name}: {k}: worst |err| / max(1, |ref|_inf) = {w:.2e}, bound {r:.2e}")


# ---------------------------------------------------------------------------
# sbk_gemm
# ---------------------------------------------------------------------------
def launch_gemm(case, dev, drop=(), tile=None):
    """One sbk_gemm launch on guard-banded operands -> (rc, out buffer, out view)."""
    L, ptr, stream_of = _abi()
    o = R.operands(case)
    tdt, odt = (_BF16 if case.bf16 else _F32), (_BF16 if case.out_bf16 else _F32)
    add = 8 if case.layout == "strided" else 0
    M, N, K, No = case.M, case.N, case.K, case.nout
    _, A = R.place(o.A, (K + add, 1), dev, NAN, dtype=tdt)
    _, W = R.place(o.W, (K + add, 1), dev, NAN, dtype=tdt)
    bias = res = mask = None
    ldr = 0
    if o.bias is not None and "bias" not in drop:
        _, bias = R.place(o.bias, (1,), dev, NAN, off=int(case.layout == "bias+1"))
    if o.res is not None:
        ldr = No + add + int(case.layout == "ldr+1")
        _, res = R.place(o.res, (ldr, 1), dev, NAN)
    if o.mask is not None and "mask" not in drop:
        _, mask = R.place(o.mask, (1,), dev, 0xFF)
    obuf, out = R.place(None, (No + add, 1), dev, R.SENTINEL, off=int(case.layout == "out+1"), shape=(M, No), dtype=odt)
    rc = L.sbk_gemm(int(case.bf16), ptr(A), K + add, ptr(W), K + add, M, N, K, ptr(bias), R.ACT_ID[case.epi], R.SLOPE,
                    ptr(res), ldr, 1.0 if "alpha" in drop else o.alpha, ptr(mask), ptr(out), No + add,
                    int(case.out_bf16), case.tile if tile is None else tile, stream_of(out))
    return rc, obuf, out


def verify(case, rc, obuf, out, worst=None, ref=None, rel=None):
    """Return code, finiteness, the guard band and the comparison of one launch."""
    if case.expect_err:
        assert rc == R.SBK_ERR_ARG, f"{case}: returned {rc}, expected SBK_ERR_ARG"
        assert bool((obuf == R.SENTINEL).all()), f"{case}: refused, but wrote to the output buffer"
        return None
    assert rc == 0, f"{case}: returned {rc}"
    got = out.cpu()
    g2 = got.reshape(-1, got.shape[-1])
    assert bool(torch.isfinite(g2.float()).all()), f"{case}: non-finite output (a guard-band NaN was read)"
    assert R.outside_untouched(obuf, out, R.SENTINEL), f"{case}: a sentinel outside the output moved"
    if ref is None:
        ref, rel = R.reference(case)
    r2 = ref.reshape(-1, ref.shape[-1])
    n, first, w = R.check(case, g2, r2, rel)
    assert n == 0, R.describe(case, "out", n, first, g2, r2)
    if rel is not None and worst is not None:
        worst.add(f"{case.epi} -> {'bf16' if case.out_bf16 else 'fp32'}", w, rel)
    return got


def _run_gemm_cases(cases, dev, name):
    worst = Worst(name)
    for case in cases:
        verify(case, *launch_gemm(case, dev), worst)
    worst.report()


@pytest.mark.parametrize("tile", list(R.TILES_BF16))
def test_gemm_tile_bf16(dev, tile):
    """Every shape, K edge, epilogue, output dtype and operand layout of one
    bf16 tile id (the list: gemm_ref.gemm_cases)."""
    _run_gemm_cases(R.gemm_cases(True, tile), dev, f"sbk_gemm bf16 tile {tile}")


@pytest.mark.parametrize("tile", list(R.TILES_F32))
def test_gemm_tile_fp32(dev, tile):
    _run_gemm_cases(R.gemm_cases(False, tile), dev, f"sbk_gemm fp32 tile {tile}")


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_gemm_auto_tile_equals_tile_2(dev, bf16):
    """tile = 0 gives tile = 2's bits in both output dtypes (exact and inexact epilogues)."""
    for case in R.dispatch_cases(bf16):
        a = verify(case, *launch_gemm(case, dev))
        rc, obuf, out = launch_gemm(case, dev, tile=0)
        b = verify(case, rc, obuf, out)
        n, first = R.mismatch(a, b)
        assert n == 0, R.describe(case, "tile 0 against tile 2", n, first, b, a)


@pytest.mark.parametrize("drop", ["bias", "mask", "alpha"])
def test_checker_has_teeth_on_real_launches(dev, drop):
    """Negative control: a launch without the bias, without the mask or with
    alpha = 1 is reported against the full reference, in both output dtypes."""
    for case in R.control_cases():
        rc, obuf, out = launch_gemm(case, dev, drop=(drop,))
        assert rc == 0
        ref, _ = R.reference(case)
        n, first, _ = R.check(case, out.cpu(), ref)
        assert n > 0 and first is not None, (drop, str(case))
        if drop == "mask":   # only the masked rows differ
            assert first[0] == 0


# ---------------------------------------------------------------------------
# sbk_gemm_ln
# ---------------------------------------------------------------------------
def launch_ln(case, dev, mutate=None):
    L, ptr, stream_of = _abi()
    o = R.operands(case)
    tdt, udt = (_BF16 if case.bf16 else _F32), (_BF16 if case.out_bf16 else _F32)
    add = 8 if case.layout == "strided" else 0
    M, N, K = case.M, case.N, case.K
    t = {}
    _, t["A"] = R.place(o.A, (K + add, 1), dev, NAN, dtype=tdt)
    _, t["W"] = R.place(o.W, (K + add, 1), dev, NAN, dtype=tdt)
    _, t["bias"] = R.place(o.bias, (1,), dev, NAN)
    _, t["res"] = R.place(o.res, (N + add, 1), dev, NAN)
    _, t["mask"] = R.place(o.mask, (1,), dev, 0xFF)
    _, t["g"] = R.place(o.ln_g, (1,), dev, NAN)
    _, t["b"] = R.place(o.ln_b, (1,), dev, NAN)
    obuf, t["out"] = R.place(None, (N + add, 1), dev, R.SENTINEL, shape=(M, N), dtype=_F32)
    ubuf, t["u"] = R.place(None, (N + add, 1), dev, R.SENTINEL, shape=(M, N), dtype=udt)
    a = {k: _vp(v) for k, v in t.items()}
    a.update(lda=K + add, ldw=K + add, ldr=N + add, ldc=N + add, ldu=N + add, N=N)
    if mutate:
        mutate(a, t)
    rc = L.sbk_gemm_ln(int(case.bf16), a["A"], a["lda"], a["W"], a["ldw"], M, a["N"], K, a["bias"], a["res"], a["ldr"],
                       o.alpha, a["mask"], a["out"], a["ldc"], a["g"], a["b"], R.LN_EPS, a["u"], a["ldu"],
                       int(case.out_bf16), case.tile, stream_of(t["out"]))
    return rc, obuf, t["out"], ubuf, t["u"]


@pytest.mark.parametrize("inst", list(R.LN_INST))
def test_gemm_ln(dev, inst):
    """out bit-exact; u against a float64 LayerNorm of the exact out; the
    masked zero-variance row gives ln_b exactly; strided ldr / ldc / ldu give
    the same; argument errors write nothing."""
    worst = Worst(f"sbk_gemm_ln {inst}")
    for case in R.gemm_ln_cases(inst):
        o = R.operands(case)
        ref, u64, rel = R.reference_ln(case, o)
        rc, obuf, out, ubuf, u = launch_ln(case, dev)
        verify(dataclasses.replace(case, out_bf16=False), rc, obuf, out, ref=ref)
        gu = u.cpu()
        assert bool(torch.isfinite(gu.float()).all()), f"{case}: non-finite u"
        assert R.outside_untouched(ubuf, u, R.SENTINEL), f"{case}: a sentinel outside u moved"
        n, first, w = R.excess(gu, u64, rel, case.out_bf16)
        assert n == 0, R.describe(case, "u", n, first, gu, u64)
        worst.add(f"LayerNorm -> {'bf16' if case.out_bf16 else 'fp32'}", w, rel)
        r = case.M // 2
        assert torch.equal(gu[r].float(), o.ln_b.to(gu.dtype).float()), f"{case}: zero-variance row {r} is not ln_b"
    worst.report()

    case = R.ln_error_case(inst)
    es = 2 if case.bf16 else 4

    def shift(name, nbytes):
        return lambda a, t: a.__setitem__(name, _vp(t[name], nbytes))

    bad = {"N = 264": lambda a, t: a.__setitem__("N", 264), "null ln_g": lambda a, t: a.__setitem__("g", None),
           "A + 1": shift("A", es), "W + 1": shift("W", es), "bias + 1": shift("bias", 4), "res + 1": shift("res", 4),
           "out + 1": shift("out", 4), "ln_g + 1": shift("g", 4), "ln_b + 1": shift("b", 4), "u + 1": shift("u", 4)}
    for ld in ("lda", "ldw", "ldr", "ldc", "ldu"):
        bad[f"{ld} + 1"] = (lambda ld: lambda a, t: a.__setitem__(ld, a[ld] + 1))(ld)
    for what, mutate in bad.items():
        rc, obuf, out, ubuf, u = launch_ln(case, dev, mutate)
        assert rc == R.SBK_ERR_ARG, f"{case}: {what}: returned {rc}, expected SBK_ERR_ARG"
        assert bool((obuf == R.SENTINEL).all()) and bool((ubuf == R.SENTINEL).all()), f"{case}: {what}: wrote"


# ---------------------------------------------------------------------------
# sbk_gemm_batched
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_gemm_batched(dev, bf16):
    """Plain (zdiv = 0) and head-interleaved (zdiv = H) outputs, batch 1 (the
    gridDim.z == 1 branch) and 3 * 4, M < Ma, padded batch strides with NaN
    between the matrices; the final matrix as a whole, bit for bit."""
    L, ptr, stream_of = _abi()
    tdt = _BF16 if bf16 else _F32
    for case in R.batched_cases(bf16):
        o = R.operands(case)
        Bt, M, N, K = case.batch, case.M, case.N, case.K
        lda = ldw = K + 8
        sA, sW = (M + 3) * lda + 8, N * ldw + 16     # Ma = M + 3: the rows past M stay NaN
        _, A = R.place(o.A, (sA, lda, 1), dev, NAN, dtype=tdt)
        _, W = R.place(o.W, (sW, ldw, 1), dev, NAN, dtype=tdt)
        odt = _BF16 if case.out_bf16 else _F32
        if case.zdiv:
            H = case.zdiv
            ldc = H * N + 8
            sC, sCo = N, M * ldc
            obuf, out = R.place(None, (sCo, sC, ldc, 1), dev, R.SENTINEL, shape=(Bt // H, H, M, N), dtype=odt)
        else:
            ldc = N + 8
            sC, sCo = M * ldc + 24, 0
            obuf, out = R.place(None, (sC, ldc, 1), dev, R.SENTINEL, shape=(Bt, M, N), dtype=odt)
        rc = L.sbk_gemm_batched(int(bf16), ptr(A), lda, sA, ptr(W), ldw, sW, M, N, K, Bt, ptr(out), ldc, sC, case.zdiv,
                                sCo, int(case.out_bf16), stream_of(out))
        verify(case, rc, obuf, out)


# ---------------------------------------------------------------------------
# sbk_gemm_tn, sbk_gemm_tn_cfg, sbk_gemm_tn_f32
# ---------------------------------------------------------------------------
def launch_tn(case, dev, K=None, mutate=None):
    L, ptr, stream_of = _abi()
    o = R.operands(case)
    tdt = _BF16 if case.bf16 else _F32
    M, N, batch = case.M, case.N, case.batch
    Kc = case.K
    add = {"dense": 0, "strided": 8, "lda+1": 1}[case.layout]
    lda, ldb = M + add, N + add
    ldc = N + (8 if case.layout == "strided" else 0)
    sA, sB, sC = Kc * lda + 8, Kc * ldb + 8, M * ldc + 16
    _, A = R.place(o.A, (sA, lda, 1), dev, NAN, dtype=tdt)
    _, B = R.place(o.W, (sB, ldb, 1), dev, NAN, dtype=tdt)
    cbuf, C = R.place(o.C0, (sC, ldc, 1), dev, R.SENTINEL)
    a = dict(A=_vp(A), B=_vp(B), lda=lda, ldb=ldb, M=M, K=Kc if K is None else K)
    if mutate:
        mutate(a, A)
    head = (a["A"], a["lda"], sA, a["B"], a["ldb"], sB, a["M"], N, a["K"], batch, ptr(C), ldc, sC)
    if case.entry == "sbk_gemm_tn_cfg":
        rc = L.sbk_gemm_tn_cfg(*head, case.tile, case.nsplit, stream_of(C))
    elif case.entry == "sbk_gemm_tn":
        rc = L.sbk_gemm_tn(*head, stream_of(C))
    else:
        rc = L.sbk_gemm_tn_f32(*head, case.nsplit, stream_of(C))
    return rc, cbuf, C


def _run_tn_cases(cases, dev):
    for case in cases:
        verify(case, *launch_tn(case, dev))


@pytest.mark.parametrize("tile", [64, 128])
def test_gemm_tn_cfg(dev, tile):
    """C0 + A^T B bit for bit at every split count (plain stores at one split,
    fp32 atomics otherwise, a recomputed split count at nsplit = 8, K = 65),
    K of one row / a chunk boundary / 1000, rotated M and N, a batch of 3 in
    the per-head block layout; K = 0 and the argument errors leave C alone."""
    _run_tn_cases(R.tn_cases(tile), dev)
    case = R.tn_error_case(tile)
    o = R.operands(case)
    rc, cbuf, C = launch_tn(case, dev, K=0)
    assert rc == 0
    verify(case, rc, cbuf, C, ref=o.C0)
    bad = {"M = 12": lambda a, A: a.__setitem__("M", 12), "lda < M": lambda a, A: a.__setitem__("lda", 64),
           "A + 1": lambda a, A: a.__setitem__("A", _vp(A, 2))}
    for what, mutate in bad.items():
        rc, cbuf, C = launch_tn(case, dev, mutate=mutate)
        assert rc == R.SBK_ERR_ARG, f"{case}: {what}: returned {rc}, expected SBK_ERR_ARG"
        verify(case, 0, cbuf, C, ref=o.C0)


def test_gemm_tn_auto(dev):
    _run_tn_cases(R.tn_auto_cases(), dev)


def test_gemm_tn_f32(dev):
    """The vector loads (M = 40, N = 36), the element-wise ones ((37, 70),
    (3, 3), lda = M + 1), K around the 32-row step, split counts 0 / 1 / 3, a
    batch of 4 with padded strides."""
    _run_tn_cases(R.tn_f32_cases(), dev)


# ---------------------------------------------------------------------------
# the Python wrappers
# ---------------------------------------------------------------------------
def test_wrapper_gemm_unaligned_views(dev):
    """_enc.gemm with a K-contiguous view whose row stride (24 B) or base
    pointer (2 B) is not 16-B aligned: the zero-width pad has to hand the
    kernel an aligned copy; and K = 10, the real padding case."""
    from speechbrain_amd import _enc
    case = R.wrapper_cases()["views"]
    o = R.operands(case)
    ref, _ = R.reference(case)
    A, W = o.A.to(_BF16).to(dev), o.W.to(_BF16).to(dev)
    dense = _enc.gemm(A, W).cpu()
    n, first = R.mismatch(dense, ref)
    assert n == 0, R.describe(case, "dense wrapper call", n, first, dense, ref)
    wide = torch.full((65, 12), NAN, dtype=_BF16, device=dev)
    wide[:, :8] = A
    flat = torch.full((1 + 65 * 8,), NAN, dtype=_BF16, device=dev)
    flat[1:] = A.reshape(-1)
    wflat = torch.full((1 + 72 * 8,), NAN, dtype=_BF16, device=dev)
    wflat[1:] = W.reshape(-1)
    for what, a, w in (("row stride 12", wide[:, :8], W), ("A from element 1", flat[1:].view(65, 8), W),
                       ("W from element 1", A, wflat[1:].view(72, 8))):
        assert a.data_ptr() % 16 or a.stride(0) % 8 or w.data_ptr() % 16
        got = _enc.gemm(a, w).cpu()
        n, first = R.mismatch(got, dense)
        assert n == 0, R.describe(case, what, n, first, got, dense)
    for dt in (_BF16, _F32):
        case = R.wrapper_cases()["k10-bf16" if dt == _BF16 else "k10-fp32"]
        o = R.operands(case)
        ref, _ = R.reference(case)
        got = _enc.gemm(o.A.to(dt).to(dev), o.W.to(dt).to(dev)).cpu()
        n, first = R.mismatch(got, ref)
        assert n == 0, R.describe(case, "K = 10", n, first, got, ref)


@pytest.mark.parametrize("dt", [_BF16, _F32], ids=["bf16", "fp32"])
def test_wrapper_gemm_tn_into_head_blocks(dev, dt):
    """_enc.gemm_tn_into: head h's product lands in columns h N .. h N + N - 1
    of one (M, H N) matrix, added to what was there."""
    from speechbrain_amd import _enc
    case = R.wrapper_cases()["tn_into-bf16" if dt == _BF16 else "tn_into-fp32"]
    H = case.batch
    o = R.operands(case)
    M, N = case.M, case.N
    c0 = o.C0.permute(1, 0, 2).reshape(M, H * N).contiguous()
    out = c0.to(dev)
    _enc.gemm_tn_into(o.A.to(dt).to(dev), o.W.to(dt).to(dev), out, H * N, N)
    ref = (o.C0.double() + o.S.double()).float().permute(1, 0, 2).reshape(M, H * N)
    got = out.cpu()
    n, first = R.mismatch(got, ref)
    assert n == 0, R.describe(case, "gemm_tn_into", n, first, got, ref)
