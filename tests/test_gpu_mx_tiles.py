"""The MXFP8 GEMM kernels tile by tile on exact block-scaled probes
(tests/mx_ref.py): mx_gemm_kernel (128 x 128) and mx_gemm256_kernel
(256 x 128, three LDS stages) of csrc/mxgemm.hip, gemm256_kernel<true, ...>
(256 x 256, multi-phase) with its split-K tail and splitk_epi_kernel of
csrc/gemm256.hip.

Operands are raw bytes built on the CPU — e4m3 codes of the integers in
[-4, 4] and chosen E8M0 scale bytes — so the float64 product of the
dequantised operands is exact and the kernels must reproduce it bit for bit:
the flat family (one scale per operand) for tiles, rings, K order, tails,
dispatch and split-K; the one-block family (a single non-zero 32-block per
row, every scale byte different from its neighbours) for the scale picks, in
both roles; the mixed family (dense operands under the same scale pattern),
whose error against the exact reference measured 0 and is asserted to be 0.
With integer bias, ReLU, alpha = 0.5 and an integer residual the fp32 output
is compared bit for bit,
the bf16 output with ref.to(bfloat16) bit for bit, and the MXFP8 output byte
for byte and scale byte for scale byte with mx_ref.mx_quantise, an
independent CPU quantiser, including crafted blocks (all zero, amax at, just
above and just below 448 * 2^k, negative amax, amax in lane 0 and lane 31,
RNE ties down to the subnormals).  GELU is compared with float64 GELU on the
exact pre-activation under max(1e-5, 8 E32) (+ 2^-8 |ref| for bf16); its
MXFP8 output equals the CPU quantisation of the same launch's fp32 output.

Every operand and scale array is a padded view (lda > K, ldsa > K / 32) into
a buffer of NaN codes (0x7F / 0xFF), every output and output-scale array a
view between 64 sentinels that also fill the columns [N, ldc), [N / 32, ldso)
and four rows below M: outputs are finite or valid codes and no sentinel
moves.  The C ABI is called directly.

Instantiation -> test id:
  mx_gemm_kernel<ACT, OUT>         -> test_mx_instantiation[k128-<act>-<out>]
  mx_gemm256_kernel<ACT, OUT>      -> test_mx_instantiation[k256x128-<act>-<out>]
  gemm256_kernel<true, ACT, OUT>   -> test_mx_instantiation[k256-<act>-<out>]
  splitk_epi_kernel<ReLU>          -> test_mx_split_k_tail_exact

Mixed family, largest |err| / sum |a b| measured on an MI355X: 0 (see
test_mx_mixed_scales)."""
import ctypes
import dataclasses

import pytest
import torch

import mx_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
_DT = {R.OUT_F32: torch.float32, R.OUT_BF16: torch.bfloat16, R.OUT_MX: torch.uint8}
_PTRS = ("A", "SA", "W", "SW", "bias", "res", "out", "out_scales", "ws", "stream")
_ORDER = ("A", "SA", "lda", "ldsa", "rpb", "a_bs", "s_bs", "W", "SW", "ldw", "ldsw", "M", "N", "K", "bias", "act",
          "alpha", "res", "ldr", "out", "ldc", "out_mode", "out_scales", "ldso")


def _lib():
    from speechbrain_amd._lib import lib
    return lib()


@dataclasses.dataclass
class Launch:
    rc: int
    obuf: torch.Tensor
    out: torch.Tensor          # (M, N) view
    sbuf: torch.Tensor = None
    sc: torch.Tensor = None    # (M, N / 32) view
    keep: tuple = ()


def launch(case, dev, over=None, entry=None, ws=None):
    """One launch of the case's entry point on guard-banded buffers.  over:
    argument name -> value, or a function of the valid value (pointers as
    integers) — the argument-error tests."""
    L = _lib()
    o = R.operands(case)
    M, N, K = case.M, case.N, case.K
    if case.conv:
        B, T_in, C, k, stride = case.conv
        a_bs, s_bs = T_in * C + 64, T_in * C // 32 + 4
        _, X = R.place(o.X.view(B, T_in * C), (a_bs, 1), dev, R.NAN8)
        _, SX = R.place(o.SX.view(B, T_in * C // 32), (s_bs, 1), dev, R.NANS)
        lda, ldsa, rpb = stride * C, stride * C // 32, (T_in - k) // stride + 1
    else:
        lda, ldsa, rpb, a_bs, s_bs = K + 16, K // 32 + 4, M, 0, 0
        _, X = R.place(o.X, (lda, 1), dev, R.NAN8)
        _, SX = R.place(o.SX, (ldsa, 1), dev, R.NANS)
    ldw, ldsw = K + 16, K // 32 + 4
    _, W = R.place(o.W, (ldw, 1), dev, R.NAN8)
    _, SW = R.place(o.SW, (ldsw, 1), dev, R.NANS)
    bias = res = None
    ldr = 0
    if o.bias is not None:
        _, bias = R.place(o.bias, (1,), dev, NAN)
    if o.res is not None:
        ldr = N + 4
        _, res = R.place(o.res, (ldr, 1), dev, NAN)
    mx = case.out == R.OUT_MX
    ldc = N + (16 if mx else 8)
    obuf, out = R.place(None, (ldc, 1), dev, R.NAN8 if mx else R.SENTINEL, shape=(M + R.ROWS_PAST_M, N),
                        dtype=_DT[case.out])
    out = out[:M]
    sbuf = sc = None
    ldso = 0
    if mx:
        ldso = N // 32 + 4
        sbuf, sc = R.place(None, (ldso, 1), dev, R.NANS, shape=(M + R.ROWS_PAST_M, N // 32), dtype=torch.uint8)
        sc = sc[:M]
    adr = lambda t: 0 if t is None else t.data_ptr()
    a = dict(A=adr(X), SA=adr(SX), lda=lda, ldsa=ldsa, rpb=rpb, a_bs=a_bs, s_bs=s_bs, W=adr(W), SW=adr(SW), ldw=ldw,
             ldsw=ldsw, M=M, N=N, K=K, bias=adr(bias), act=case.act, alpha=case.alpha, res=adr(res), ldr=ldr,
             out=adr(out), ldc=ldc, out_mode=case.out, out_scales=adr(sc), ldso=ldso, ws=adr(ws),
             ws_floats=0 if ws is None else ws.numel(), stream=torch.cuda.current_stream(dev).cuda_stream)
    for k_, v in (over or {}).items():
        a[k_] = v(a[k_]) if callable(v) else v
    entry = entry or case.entry_point
    names = _ORDER + (("ws", "ws_floats") if entry == "sbk_mx_gemm_ws" else ()) + ("stream",)
    args = [(ctypes.c_void_p(a[n]) if a[n] else None) if n in _PTRS else a[n] for n in names]
    rc = getattr(L, entry)(*args)
    return Launch(rc, obuf, out, sbuf, sc, keep=(X, SX, W, SW, bias, res))


def guards(case, r):
    """Return code, valid values and the sentinels of one launch -> the output(s) on the CPU."""
    assert r.rc == 0, f"{case}: returned {r.rc}"
    torch.cuda.synchronize()
    got = r.out.cpu()
    fill = R.NAN8 if case.out == R.OUT_MX else R.SENTINEL
    assert R.outside_untouched(r.obuf, r.out, fill), f"{case}: a sentinel outside the output moved"
    if case.out != R.OUT_MX:
        assert bool(torch.isfinite(got.float()).all()), f"{case}: non-finite output (a guard-band code was read)"
        return got, None
    gs = r.sc.cpu()
    assert R.outside_untouched(r.sbuf, r.sc, R.NANS), f"{case}: a sentinel outside the output scales moved"
    assert R.valid_codes(got, gs), f"{case}: NaN code in the MXFP8 output (unwritten, or a guard-band code was read)"
    return got, gs


def run(case, dev):
    """Launch, guard checks, comparison -> the fp32 / bf16 / byte output."""
    assert case.entry or R.expected_kernel(case.M, case.N) == case.kernel or case.kernel == "k256", str(case)
    ref, rel = R.reference(case)
    if case.gelu and case.out == R.OUT_MX:
        # the existing relation: bytes and scales are the CPU quantisation of the same launch's fp32 output
        c0 = dataclasses.replace(case, out=R.OUT_F32)
        f32, _ = guards(c0, launch(c0, dev))
        fails = R.check(c0, f32, None, ref, rel)
        got, gs = guards(case, launch(case, dev))
        wq, ws = R.mx_quantise(f32)
        for what, g, w in (("e4m3 bytes", got, wq), ("scale bytes", gs, ws)):
            n, first = R.mismatch_u8(g, w)
            if n:
                fails.append(f"{case}: {what} differ from the quantised fp32 output at {n} places, first {first}")
    else:
        got, gs = guards(case, launch(case, dev))
        fails = R.check(case, got, gs, ref, rel)
    assert not fails, "\n".join(fails)
    return got


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("out", R.OUTS)
@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("kernel", R.KERNELS)
def test_mx_instantiation(dev, kernel, act, out):
    """Every ACT x OUT instantiation of the three kernels with the full
    epilogue: F, B and BT (GELU: F and X), ReLU also without a residual, and
    for an exact activation with MXFP8 out the quantiser's edge blocks."""
    for case in R.instantiation_cases(kernel, act, out):
        run(case, dev)


@pytest.mark.parametrize("kernel,K", [(k, K) for k in R.KERNELS for K in R.shape_ks(k)])
def test_mx_shapes(dev, kernel, K):
    """The shape table: row tails of 1 / BM - 1 / BM + 1 rows, one to seven
    K-tiles (both buffers and their reuse; the three-stage ring's wrap and
    both of its vmcnt branches), grids with and without the XCD remap, the
    256 x 128 kernel's cpx tile map at N = 1024 (a tile produced twice leaves
    another unwritten: its sentinels fail the comparison), more than 8 row
    panels x 2 columns of the multi-phase kernel's panel groups."""
    for case in R.shape_cases(kernel, K):
        run(case, dev)


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_mx_mixed_scales(dev, kernel, capsys):
    """Dense operands under the varying scale pattern (family X): products
    span 2^16 and the exact sum fits fp32.  The first run on an MI355X
    measured max |err| / sum |a b| = 0 on every case of the three kernels
    (all 1 508 736 outputs bit-exact; the project's bound for random operands
    is 2e-5, test_gpu_wav2vec.py measures ~4e-6 there), so the assertion is
    bit equality with the exact reference; the ratio is still printed."""
    for case in R.mixed_cases(kernel):
        got, _ = guards(case, launch(case, dev))
        ref, _ = R.reference(case)
        ratio = R.ratio_to_sum_abs(got, ref.double(), R.sum_abs(case, R.operands(case)))
        with capsys.disabled():
            print(f"\n{case}: max |err| / sum|a b| = {ratio:.3e}")
        fails = R.check(case, got, None, ref)
        assert not fails, "\n".join(fails)


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_mx_conv_addressing(dev, kernel):
    """lda = stride * C < K (overlapping rows), rpb = T_out, padded batch
    strides; a batch boundary inside a tile and the last batch ending inside
    one.  The reference is an integer-valued conv1d over the stored input."""
    for case in R.conv_cases(kernel):
        run(case, dev)


def test_mx_dispatch_boundary(dev):
    """At 180 tiles of 256 x 256 sbk_mx_gemm equals sbk_mx_gemm256 bit for
    bit (and the exact reference); at 176 it runs the 256 x 128 kernel and
    equals the exact reference."""
    d = R.dispatch_cases()
    a = launch(d["at"], dev)
    b = launch(d["at-direct"], dev)
    assert a.rc == 0 and b.rc == 0, (a.rc, b.rc)
    assert torch.equal(a.out, b.out)
    ref, _ = R.reference(d["at-direct"])
    got, _ = guards(d["at"], a)
    fails = R.check(d["at"], got, None, ref)
    assert not fails, "\n".join(fails)
    run(d["below"], dev)


@pytest.mark.parametrize("with_res", [True, False])
def test_mx_split_k_tail_exact(dev, with_res):
    """sbk_mx_gemm_ws at test_gpu_gemm256.py's split-K shape on the flat
    family, bias + ReLU + alpha (+ residual): exact sums do not depend on the
    split, so the result equals sbk_mx_gemm's bit for bit, and the tail
    tiles equal the CPU reference bit for bit."""
    case = [c for c in R.split_cases() if c.res == with_res][0]
    M, N, K = case.M, case.N, case.K
    L = _lib()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    tiles = R.split_tail_tiles(M, N, K, cus)
    if not tiles:
        pytest.skip(f"{cus} CUs: no split tail at this shape")
    nws = int(L.sbk_mx_gemm_ws_floats(M, N, K, 0))
    assert nws == 2 * len(tiles) * 65536, (nws, len(tiles))
    plain = launch(case, dev, entry="sbk_mx_gemm")
    ws = torch.full((nws + 8,), NAN, device=dev)[:nws]
    split = launch(case, dev, entry="sbk_mx_gemm_ws", ws=ws)
    assert plain.rc == 0 and split.rc == 0, (plain.rc, split.rc)
    torch.cuda.synchronize()
    assert torch.equal(split.out, plain.out)
    got, _ = guards(case, split)
    o = R.operands(case)
    for tm, tn in tiles:
        rows, cols = slice(256 * tm, min(256 * tm + 256, M)), slice(256 * tn, 256 * tn + 256)
        ref = R.epilogue(R.product(case, o, rows, cols), case, o, rows=rows, cols=cols)
        assert torch.equal(ref.float().double(), ref)
        n, first = R.mismatch(got[rows, cols].contiguous(), ref.float())
        assert n == 0, f"{case}: tail tile ({tm}, {tn}): {n} wrong, first at {first}"


def _errors(entry):
    plus = lambda d: (lambda v: v + d)
    e = [("K % 128", dict(K=64)), ("N % 128", dict(N=64)), ("rpb 0", dict(rpb=0)),
         ("A misaligned", dict(A=plus(8))), ("W misaligned", dict(W=plus(8))), ("lda % 16", dict(lda=plus(8))),
         ("ldw % 16", dict(ldw=plus(8))), ("a_bs % 16", dict(a_bs=8)), ("SA misaligned", dict(SA=plus(2))),
         ("SW misaligned", dict(SW=plus(2))), ("ldsa % 4", dict(ldsa=plus(2))), ("ldsw % 4", dict(ldsw=plus(2))),
         ("s_bs % 4", dict(s_bs=2)), ("Swish", dict(act=1)), ("unknown act", dict(act=7)),
         ("out_mode 2, null scales", dict(out_scales=0)), ("out_mode 2, ldc % 16", dict(ldc=plus(8))),
         ("out_mode 3", dict(out_mode=3))]
    if entry == "sbk_mx_gemm256":
        e.append(("N % 256", dict(N=128)))
    else:
        e.append(("ldso % 4", dict(ldso=plus(2))))
    if entry == "sbk_mx_gemm_ws":
        e += [("negative workspace", dict(ws_floats=-1)), ("null workspace", dict(ws=0, ws_floats=1024)),
              ("misaligned workspace", dict(ws=plus(4)))]
    return e


@pytest.mark.parametrize("entry", ["sbk_mx_gemm", "sbk_mx_gemm256", "sbk_mx_gemm_ws"])
def test_mx_argument_errors(dev, entry):
    """Each is refused with SBK_ERR_ARG before anything is written; the same
    arguments without the error run and give the exact result."""
    case = R.error_case(entry)
    ws = torch.zeros(1024 + 8, device=dev)[:1024] if entry == "sbk_mx_gemm_ws" else None
    for name, over in _errors(entry):
        r = launch(case, dev, over=over, ws=ws)
        assert r.rc == R.SBK_ERR_ARG, f"{entry}: {name}: returned {r.rc}"
        torch.cuda.synchronize()
        assert bool((r.obuf == R.NAN8).all()) and bool((r.sbuf == R.NANS).all()), f"{entry}: {name}: refused, but wrote"
    got, gs = guards(case, launch(case, dev, ws=ws))
    fails = R.check(case, got, gs, R.reference(case)[0])
    assert not fails, "\n".join(fails)
