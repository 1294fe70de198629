"""CPU test of the MXFP8 GEMM probes (tests/mx_ref.py): the conditions the
bit-exactness argument rests on hold for every case test_gpu_mx_tiles.py
launches, the one-block family's scale bytes differ wherever a wrong pick
could land, the quantiser's edge cases are present and the quantiser agrees
with oracle.wav2vec.mx_round, and the checker rejects eleven wrong "kernels"
modelled in torch — so a pass on the GPU means something."""
import dataclasses
import math

import pytest
import torch

import mx_ref as R
import oracle.wav2vec as OW

GROUPS = R.all_cases()


def _as_output(case, val):
    """What a kernel computing `val` (float64) would store -> (out, scales)."""
    if case.out == R.OUT_MX:
        return R.mx_quantise(val.float())
    return val.float().to(torch.bfloat16 if case.out == R.OUT_BF16 else torch.float32), None


def _rejected(case, val):
    ref, rel = R.reference(case)
    return bool(R.check(case, *_as_output(case, val), ref, rel))


@pytest.mark.parametrize("group", list(GROUPS))
def test_probe_conditions(group):
    """Integer codes only, the sum bound below 2^24 units of the output, the
    exact epilogue representable in fp32 (asserted inside reference()), the
    case on the kernel it names, K <= 2048."""
    seen = set()
    for case in GROUPS[group]:
        assert case.K <= 2048 and case.K % 128 == 0 and case.N % 128 == 0, str(case)
        if case.entry_point != "sbk_mx_gemm256":
            assert R.expected_kernel(case.M, case.N) == case.kernel, str(case)
        else:
            assert case.N % 256 == 0, str(case)
        key = (case.fam, case.M, case.N, case.K, case.flat, case.gelu, case.conv, case.seed)
        if key in seen:
            continue
        seen.add(key)
        if case.M > 12000:      # the split-K shape: 16 K = 2^15 units of 2^-3, integer bias and residual, alpha 0.5:
            assert case.fam == "F" and not case.gelu      # multiples of 2^-4 below 2^13; its tail tiles are
            continue                                      # asserted representable where the GPU test builds them
        o = R.operands(case)
        c = R.probe_conditions(case, o)
        assert c["codes"], str(case)
        assert c["sum_units"] < 2 ** 24, (str(case), c["sum_units"])
        if case.epi or case.fam == "E" or case.conv:
            ref, rel = R.reference(case)
            assert (rel is None) == (not case.gelu)
            if case.gelu:   # pre-activations O(1)
                assert float(R.product(case, o).abs().max()) < 8, str(case)
        if case.conv:
            assert torch.equal(R.conv_product(case, o), R.product(case, o)), str(case)


def test_case_lists_cover_the_issue():
    for kern in R.KERNELS:
        for act in R.ACTS:
            for out in R.OUTS:
                cs = GROUPS[f"inst-{kern}-{act}-{out}"]
                assert cs and all((c.kernel, c.act, c.out) == (kern, act, out) and (c.epi or c.fam == "E") for c in cs)
                fams = {c.fam for c in cs}
                assert fams >= ({"F", "X"} if act == R.ACT_GELU else {"F", "B", "BT"})
                assert ("E" in fams) == (act != R.ACT_GELU and out == R.OUT_MX)
        assert {c.fam for c in GROUPS[f"conv-{kern}"]} == {"F", "B", "BT"}
    sh = {k: set(v) for k, v in R.SHAPES.items()}
    assert sh["k128"] >= {(M, N, K) for M in (1, 127, 128, 129, 257) for N in (128, 384) for K in (128, 256, 384, 512)}
    assert any((-(-M // 128) * (N // 128)) % 8 == 0 for M, N, _ in sh["k128"])
    assert sh["k256x128"] == {(M, N, K) for M in (4096, 4097, 4351) for N in (128, 1024)
                              for K in (128, 256, 384, 512, 896)}
    assert sh["k256"] == {(M, N, K) for M in (1, 255, 256, 257, 513, 2305) for N in (256, 512) for K in (128, 256, 384)}
    for kern in R.KERNELS:   # conv: a batch boundary inside a tile, the last batch ending inside one
        B, T_in, C, k, stride, N = R.CONV[kern]
        T_out, bm = (T_in - k) // stride + 1, 128 if kern == "k128" else 256
        assert stride * C < k * C and T_out % bm and (B * T_out) % bm
        assert R.expected_kernel(B * T_out, N) == kern or kern == "k256"
    d = R.dispatch_cases()
    assert -(-d["at"].M // 256) * (d["at"].N // 256) == 180 and -(-d["below"].M // 256) * (d["below"].N // 256) == 176
    assert {(c.act, c.res) for c in R.split_cases()} == {(R.ACT_RELU, True), (R.ACT_RELU, False)}
    assert all((c.M, c.N, c.K) == (17820, 1024, 2048) for c in R.split_cases())


def test_scale_pattern_is_distinct_everywhere():
    """Adjacent blocks, rows 32 / 64 / 128 apart and SA against SW at the same
    index all differ (also under the GELU shift); the one-block rows use every
    block of every K-tile inside every 32-row MFMA tile, with no zero element
    (both 16-byte lane halves are live)."""
    for base in (R.SW_BASE, R.SW_BASE - R.GELU_SHIFT):
        sa, sw = R.pattern_sa(4400, 28).long(), R.pattern_sw(4400, 28, base).long()
        for s in (sa, sw):
            assert bool((s[:, 1:] != s[:, :-1]).all())
            for d in (32, 64, 128):
                assert bool((s[d:] != s[:-d]).all())
            assert int(s.min()) >= 100 and int(s.max()) <= 130
        assert bool((sa != sw).all())
        assert not (set(sa.unique().tolist()) & set(sw.unique().tolist()))
    for kern in R.KERNELS:
        for case in R.instantiation_cases(kern, R.ACT_NONE, R.OUT_F32):
            if case.fam not in ("B", "BT"):
                continue
            o = R.operands(case)
            q = (o.X if case.fam == "B" else o.W)
            nz = ((q & 0x7F) != 0).view(q.shape[0], -1, 32)
            assert bool((nz.sum((1, 2)) == 32).all()) and bool((nz.all(2).sum(1) == 1).all()), str(case)
            blk = nz.all(2).long().argmax(1)
            for g in range(q.shape[0] // 32):
                assert set(blk[32 * g:32 * g + 32].tolist()) == set(range(case.K // 32)), (str(case), g)
            other = (o.W if case.fam == "B" else o.X)
            assert bool(((other & 0x7F) != 0).view(other.shape[0], -1, 32).any(2).all())


def _rne_bruteforce(q):
    """Nearest e4m3fn value, ties to the even code, by search over the table."""
    tab = R.e4m3_table()[:0x7F]
    d = (q.abs()[:, None] - tab[None, :]).abs()
    best = d.min(1).values
    cand = d == best[:, None]
    code = torch.arange(0x7F)[None, :].expand_as(cand)
    even = cand & (code % 2 == 0)
    pick = torch.where(cand.sum(1) > 1, even.long().argmax(1), cand.long().argmax(1))
    return pick.to(torch.uint8) | (torch.signbit(q).to(torch.uint8) << 7)


def test_quantiser_is_pinned():
    """scale_bytes against math.frexp, the e4m3 cast against a brute-force
    nearest-even search, and the whole quantiser against
    oracle.wav2vec.mx_round on the dequantised values."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(64, 256, generator=g) * torch.logspace(-6, 4, 256)[None, :]
    x = torch.cat([x, R.edge_residual(80, 256)])
    x[3, :32] = 0.0
    am = x.view(x.shape[0], -1, 32).abs().amax(-1)
    sb = R.scale_bytes(am)
    assert sb.flatten().tolist() == [R.scale_byte_scalar(float(a)) for a in am.flatten()]
    for a, b in zip(am.flatten().tolist(), sb.flatten().tolist()):   # the smallest power of two that fits 448
        if a > 0:
            assert a / 2.0 ** (b - 127) <= 448 < a / 2.0 ** (b - 128)
    q, s = R.mx_quantise(x)
    scaled = torch.ldexp(x.double().view(x.shape[0], -1, 32), (127 - s.long())[..., None].expand(-1, -1, 32))
    assert torch.equal(q.flatten(), _rne_bruteforce(scaled.flatten()))
    assert torch.equal(R.dequantise(q, s), OW.mx_round(x).double())
    # the modelled truncation and scale slip really differ from it
    assert not torch.equal(R.mx_quantise(x, truncate=True)[0], q)
    assert bool((R.e4m3_table()[R.mx_quantise(x, truncate=True)[0].long()].abs() <= scaled.abs().view(x.shape)).all())


def test_quantiser_edge_cases_are_present():
    eb = R.edge_blocks()
    names = [n for n, _ in eb]
    tab = R.e4m3_table()[:0x7F]
    mid = (tab[1:] + tab[:-1]) / 2
    tie_exps, ties = set(), 0
    for n, v in eb:
        am = float(v.abs().max())
        sb = R.scale_byte_scalar(am)
        lane = int(v.abs().argmax())
        if n.startswith("zero"):
            assert sb == 0 and am == 0.0
            continue
        assert lane in (0, 31) and f"lane {lane}" in n
        m, e = math.frexp(am)
        q = v.double().abs() / 2.0 ** (sb - 127)
        if " at " in n:        # amax = 448 * 2^k exactly: ma = 0.875, not above it; stored as 448
            assert m == 0.875 and float(q.max()) == 448.0 and sb == e - 9 + 127
        if "above" in n:       # one step above: the next scale byte, q just over 224
            assert m > 0.875 and sb == e - 8 + 127 and 224.0 < float(q.max()) < 224.001
        if "below" in n:
            assert m < 0.875 and 447.9 < float(q.max()) < 448.0
        if "neg" in n:
            assert float(v[lane]) < 0
        if n.startswith("ties"):
            t = int(torch.isin(q, mid).sum())
            assert t >= 12, (n, t)
            ties += t
            tie_exps.add(sb)
            assert bool((q[torch.isin(q, mid)] < 2.0 ** -8).any())    # ties among the subnormals too
    assert len(tie_exps) == 3 and ties >= 72
    assert sum(" at " in n for n in names) >= 6 and sum("above" in n for n in names) >= 6
    assert sum("neg" in n for n in names) >= 6 and "zero" in names
    # every edge block reaches every column-block position of the E cases
    for kern in R.KERNELS:
        for case in R.instantiation_cases(kern, R.ACT_NONE, R.OUT_MX):
            if case.fam == "E":
                assert case.M >= len(eb) and case.alpha == R.ALPHA and R.operands(case).bias is None
                ref, _ = R.reference(case)
                assert torch.equal(ref, R.operands(case).res)
                q, s = R.mx_quantise(ref)
                zero = s == 0
                assert bool(zero.any()) and bool(((q & 0x7F) == 0).view(case.M, -1, 32)[zero].all())


def test_bf16_rounding_and_ties_occur():
    for kern in R.KERNELS:
        for act in (R.ACT_NONE, R.ACT_RELU):
            for case in R.instantiation_cases(kern, act, R.OUT_BF16):
                ref, _ = R.reference(case)
                bits = ref.view(torch.int32) & 0xFFFF
                assert bool((bits != 0).any()), str(case)
                if case.fam == "F":
                    assert bool((bits == 0x8000).any()), str(case)


def _inst(kern, fam, act=R.ACT_NONE, out=R.OUT_F32):
    return [c for c in R.instantiation_cases(kern, act, out) if c.fam == fam][0]


@pytest.mark.parametrize("kern", R.KERNELS)
@pytest.mark.parametrize("kind", R.WRONG_PRODUCT)
def test_checker_rejects_wrong_products(kern, kind):
    """A wrong scale pick must fail the one-block family (each in the role
    that exposes it), a wrong K-tile the flat family."""
    fams = {"block^1": ("B", "BT"), "row^32": ("BT",), "sw_from_sa": ("B", "BT"), "halves_swapped": ("B", "F"),
            "ktile_skipped": ("F",), "ktile_twice": ("F",)}[kind]
    for fam in fams:
        for out in R.OUTS:
            case = _inst(kern, fam, out=out)
            o = R.operands(case)
            assert _rejected(case, R.epilogue(R.product(case, o, wrong=kind), case, o)), (str(case), kind)
            assert not _rejected(case, R.epilogue(R.product(case, o), case, o)), str(case)
    if kind == "block^1":     # and in the shape table (no epilogue), through the conv addressing too
        for case in [c for c in R.shape_cases(kern, 128) if c.fam in ("B", "BT")][:2] + R.conv_cases(kern)[1:]:
            o = R.operands(case)
            assert _rejected(case, R.product(case, o, wrong=kind)), str(case)


@pytest.mark.parametrize("kern", R.KERNELS)
def test_checker_rejects_wrong_epilogues_and_stores(kern):
    # alpha before the activation (only GELU tells: ReLU commutes with alpha > 0), the residual scaled by alpha
    for out in (R.OUT_F32, R.OUT_BF16):
        case = _inst(kern, "F", R.ACT_GELU, out)
        o = R.operands(case)
        pre = R.product(case, o)
        assert _rejected(case, R.epilogue(pre, case, o, alpha_first=True)), str(case)
        assert _rejected(case, R.epilogue(pre, case, o, res_scaled=True)), str(case)
        assert not _rejected(case, R.epilogue(pre, case, o)), str(case)
    for out in R.OUTS:
        case = _inst(kern, "F", R.ACT_RELU, out)
        o = R.operands(case)
        assert _rejected(case, R.epilogue(R.product(case, o), case, o, res_scaled=True)), str(case)
    # the last row tile's rows stored one row down: a wrong row inside, a moved sentinel below
    case = _inst(kern, "F")
    ref, _ = R.reference(case)
    buf = R.rows_stored_past_m(ref, 128 if kern == "k128" else 256)
    assert R.check(case, buf[:case.M].contiguous(), None, ref) and bool((buf[case.M] != R.SENTINEL).any())
    # MXFP8 store: the scale byte one too high at amax = 448 * 2^k (ma >= 0.875 for ma > 0.875), truncation for RNE
    for fam in ("E", "F"):
        case = _inst(kern, fam, out=R.OUT_MX)
        ref, _ = R.reference(case)
        slip = lambda sb, am: sb + ((torch.frexp(am)[0] == 0.875) & (am > 0)).to(torch.uint8)
        q, s = R.mx_quantise(ref, scale_off=slip)
        assert R.check(case, q, s, ref) or fam == "F", str(case)   # (F meets the boundary only by chance)
        q, s = R.mx_quantise(ref, truncate=True)
        assert R.check(case, q, s, ref), str(case)
        assert not R.check(case, *R.mx_quantise(ref), ref)


def test_tile_order_and_split_tail():
    """tile_of is a bijection on the grids used, and the split-K tail of the
    test shape on 256 compute units is the 24 tiles the rule gives."""
    for ntn, ntm in ((1, 1), (2, 10), (4, 70), (4, 45), (2, 3)):
        tiles = {R.tile_of(i, ntn, ntm) for i in range(ntn * ntm)}
        assert tiles == {(tm, tn) for tm in range(ntm) for tn in range(ntn)}
    M, N, K = R.SPLIT_SHAPE
    t = R.split_tail_tiles(M, N, K, 256)
    assert len(t) == 280 % 256 and len(set(t)) == len(t)
    assert R.split_tail_tiles(M, N, 1024, 256) == [] and R.split_tail_tiles(M, N, K, 304) == []
