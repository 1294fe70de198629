"""CPU test of the GEMM probes (tests/gemm_ref.py): the conditions the
bit-exactness argument rests on hold for every case test_gpu_gemm_tiles.py
launches, the case lists cover what they claim, and the checker rejects a
set of wrong "kernels" modelled in torch — so a pass on the GPU means
something."""
import pytest
import torch

import gemm_ref as R

GROUPS = R.all_cases()


@pytest.mark.parametrize("group", list(GROUPS))
def test_probe_conditions(group):
    """Operands survive bf16, every partial sum is below 2^20 (sum |a||w|
    bounds them all), and the fp32 CPU matmul equals the int64 one."""
    seen = set()
    for case in GROUPS[group]:
        key = (case.batch, case.M, case.N, case.K, case.seed, case.scaled)
        if key in seen:
            continue
        seen.add(key)
        o = R.operands(case)
        c = R.probe_conditions(case, o)
        assert c["bf16_round_trip"], str(case)
        assert c["sum_abs"] < 2 ** 20, (str(case), c["sum_abs"])
        assert c["fp32_equals_int64"], str(case)
        for t in (o.bias, o.res, o.C0, o.ln_g, o.ln_b):
            if t is not None:   # multiples of 1/4 in [-4, 4]
                assert torch.equal((t * 4).round(), t * 4) and float(t.abs().max()) <= 4.0, str(case)
        if case.scaled:
            assert case.K <= 256, str(case)


@pytest.mark.parametrize("bf16,tile", [(True, t) for t in R.TILES_BF16] + [(False, t) for t in R.TILES_F32])
def test_gemm_case_list_covers_the_issue(bf16, tile):
    """Per tile id: every epilogue with both output dtypes, every layout at a
    full and a ragged shape, the mask on row 0, row M - 1 and the last row of
    the first tile, and the pipeline's K edges."""
    cases = R.gemm_cases(bf16, tile)
    BM, BN, BK = (R.TILES_BF16 if bf16 else R.TILES_F32)[tile]
    run = [c for c in cases if not c.expect_err]
    for epi in R.EXACT + R.INEXACT:
        for ob in (False, True):
            hit = [c for c in run if c.epi == epi and c.out_bf16 == ob]
            assert bool(hit) == (not (tile == 30 and epi == "glu")), (tile, epi, ob)
    for layout in R.LAYOUTS:
        shapes = {(c.M, c.N) for c in cases if c.layout == layout}
        assert (BM, BN) in shapes and (BM + 1, BN + (0 if tile == 30 else 4)) in shapes, (tile, layout)
        assert layout == "dense" or len(shapes) == 2, (tile, layout)
    ks = {c.K for c in run}
    if tile in R.RING:
        assert {192, 256, 320, 576} <= ks and {c.K for c in cases if c.expect_err} == {128, 200}
    elif tile in R.PREFETCH:
        assert {n * BK - d for n in (1, 2, 3, 4, 5, 9) for d in (0, 8)} <= ks
    elif tile == 30:
        assert ks == {64, 128, 192, 320} and {c.M for c in run} == {1, 255, 256, 257, 513}
        assert any(c.N == 264 for c in cases if c.expect_err)
    big = R.Case("sbk_gemm", bf16, tile, 3 * BM, BN, BK, "affine")
    assert big.mask_rows() == (0, BM - 1, 3 * BM - 1)
    assert max(c.M for c in cases) <= 17 * 128 and max(c.N for c in cases) <= 3 * 256
    assert max(c.K for c in cases) <= 5 * 256 + 8


# ---------------------------------------------------------------------------
# the checker accepts the right answer and rejects wrong kernels
# ---------------------------------------------------------------------------
def _case(epi, ob=False, M=65, N=96, K=144):
    return R.Case("sbk_gemm", True, 2, M, N, K, epi, ob, seed=3)


def _run(case, pre=None, **changes):
    """The modelled kernel: the epilogue in float64 (exact epilogues: exact) on `pre`."""
    o = R.operands(case)
    kw = dict(bias=o.bias, res=o.res, mask=o.mask, alpha=o.alpha)
    kw.update(changes)
    pre = o.S.double() * o.wscale if pre is None else pre
    x = R.epilogue(pre, case.epi, kw["bias"], kw["res"], kw["mask"], kw["alpha"],
                   alpha_after_res=changes.get("alpha_after_res", False))
    return x.to(torch.bfloat16 if case.out_bf16 else torch.float32)


def _count(case, got):
    ref, rel = R.reference(case)
    return R.check(case, got, ref, rel)[0]


@pytest.mark.parametrize("ob", [False, True])
@pytest.mark.parametrize("epi", R.EXACT + R.INEXACT)
def test_checker_accepts_the_reference(epi, ob):
    case = _case(epi, ob)
    ref, rel = R.reference(case)
    got = _run(case)
    n, first, worst = R.check(case, got, ref, rel)
    assert n == 0 and first is None
    if rel is not None:   # an fp32 evaluation of the epilogue is inside the bound too
        o = R.operands(case)
        g32 = R.epilogue(o.S.double() * o.wscale, epi, o.bias, o.res, o.mask, o.alpha, torch.float32)
        assert R.check(case, g32.to(got.dtype), ref, rel)[0] == 0


@pytest.mark.parametrize("ob", [False, True])
@pytest.mark.parametrize("epi", ["affine", "lrelu", "swish", "gelu"])
def test_checker_rejects_wrong_kernels(epi, ob):
    case = _case(epi, ob)
    o = R.operands(case)
    A, W = o.A.double(), o.W.double()
    pre = A @ W.t()
    # an 8-element K chunk dropped at one 16 x 16 tile position
    p = pre.clone()
    p[16:32, 32:48] -= A[16:32, 64:72] @ W[32:48, 64:72].t()
    assert _count(case, _run(case, p)) > 0
    # two K steps swapped between two rows
    p = pre.clone()
    ks = slice(64, 128)
    p[5] += (A[6, ks] - A[5, ks]) @ W[:, ks].t()
    p[6] += (A[5, ks] - A[6, ks]) @ W[:, ks].t()
    assert _count(case, _run(case, p)) > 0
    # the row mask shifted by one row
    assert _count(case, _run(case, mask=torch.roll(o.mask, 1))) > 0
    # the bias shifted by four columns
    assert _count(case, _run(case, bias=torch.roll(o.bias, 4))) > 0
    # the last row / the last column quad left unwritten
    for sl in ((slice(-1, None), slice(None)), (slice(None), slice(-4, None))):
        got = _run(case)
        got[sl] = R.SENTINEL
        n, first, _ = R.check(case, got, *R.reference(case))
        assert n > 0 and (first[0] == case.M - 1 or first[1] == case.nout - 4)
    # alpha applied after the residual instead of before
    assert _count(case, _run(case, alpha_after_res=True)) > 0
    # a NaN anywhere
    got = _run(case)
    got[3, 7] = float("nan")
    assert _count(case, got) > 0


@pytest.mark.parametrize("ob", [False, True])
def test_checker_rejects_swapped_glu_halves(ob):
    case = _case("glu", ob)
    o = R.operands(case)
    pre = o.S.double() * o.wscale
    M, N = pre.shape
    swapped = pre.view(M, N // 32, 2, 16).flip(2).reshape(M, N)           # [gate16 | value16]
    bias = o.bias.view(N // 32, 2, 16).flip(1).reshape(N)
    assert _count(case, _run(case, swapped, bias=bias)) > 0
    assert _count(case, _run(case)) == 0


def test_checker_reports_the_first_element():
    a = torch.zeros(5, 9)
    b = a.clone()
    b[2, 7] = 1.0
    b[4, 0] = -0.0          # bitwise: -0 is not +0
    assert R.mismatch(a, b) == (2, (2, 7))
    assert R.mismatch(a, a.clone()) == (0, None)
    case = _case("affine")
    msg = R.describe(case, "out", 2, (2, 7), a, b)
    assert "sbk_gemm" in msg and "tile 2" in msg and "M=65" in msg and "epilogue=affine" in msg and "row 2, column 7" in msg


def test_guard_band_helper_sees_stray_stores():
    buf, view = R.place(None, (12, 1), "cpu", R.SENTINEL, off=1, shape=(3, 8), dtype=torch.float32)
    assert view.storage_offset() == R.PAD + 1 and buf.numel() >= R.PAD + 1 + 3 * 12 + R.PAD
    view.fill_(1.0)
    assert R.outside_untouched(buf, view, R.SENTINEL)
    for stray in (R.PAD, R.PAD + 1 + 8, R.PAD + 1 + 2 * 12 + 8, buf.numel() - 1):   # before, column N of row 0, past row M - 1
        b2 = buf.clone()
        b2[stray] = 0.0
        assert not R.outside_untouched(b2, b2.as_strided(view.shape, view.stride(), view.storage_offset()), R.SENTINEL)


def test_ln_reference_zero_variance_row():
    case = R.gemm_ln_cases("bf16-0")[-1]
    o = R.operands(case)
    out, u64, rel = R.reference_ln(case, o)
    r = case.M // 2
    assert o.mask[r] and torch.equal(out[r], torch.full((256,), 3.0))
    assert torch.equal(u64[r].float(), o.ln_b) and rel >= 1e-5
