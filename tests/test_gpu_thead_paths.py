"""Fused transducer head (csrc/thead.hip), path by path, through the C ABI and
through transducer_head_loss under bf16 autocast, against the float64
reference on the kernels' operand rounding (tests/thead_ref.py, pinned on the
CPU by test_transducer_ref_cpu.py).

What test_gpu_thead.py never runs: a blank other than 0 (in the second and
third 128-column vocabulary chunk, and as the only valid column of the last
one), the identity and ReLU joints, J = 512, an online log-sum-exp whose
maximum moves between chunks, a per-utterance gradient scale, dS element by
element, the weight-gradient kernel on its own, reduction="sum", empty
transcripts and single frames, and label padding.

Measured on an MI355X (worst observed error over the stated bound):
forward rows 0.004, moving maximum 0.004, dS elements 0.95, wgrad 0.014."""
import numpy as np
import pytest
import torch

import thead_ref as TR

pytestmark = pytest.mark.gpu

SENT = 12345.0
SCALES = (1.0, -2.0, 0.5, 3.0)


def _lib():
    from speechbrain_amd._lib import check, lib, ptr
    return lib(), ptr, check


def _pad_w(w, dev):
    """(V, J) fp32 -> (Vp, J) bf16 on the device, rows >= V zero."""
    L, _, _ = _lib()
    V, J = w.shape
    out = torch.zeros(int(L.sbk_thead_vpad(V)), J, dtype=torch.bfloat16)
    out[:V] = w.to(torch.bfloat16)
    return out.to(dev)


def _case(B, T, U1, J, V, blank, seed, Tl=None, Ul=None):
    """Random head inputs on the CPU; the labels avoid the blank and include
    the columns 127, 128 and V - 1 (the chunk edges) where they exist."""
    g = torch.Generator().manual_seed(seed)
    tn = torch.randn(B, T, J, generator=g)
    pn = torch.randn(B, U1, J, generator=g)
    w = torch.randn(V, J, generator=g) / J ** 0.5
    labels = TR.labels_other_than(np.random.default_rng(seed), blank, V, (B, U1 - 1))
    forced = [c for c in (127, 128, V - 1) if c < V and c != blank]
    for n, c in enumerate(forced):
        labels[n % B, n % (U1 - 1)] = c
    Tl = np.array([T - (2 * i) % max(T // 2, 1) for i in range(B)] if Tl is None else Tl, np.int32)
    Ul = np.array([(U1 - 1) - (2 * i) % max((U1 - 1) // 2, 1) for i in range(B)] if Ul is None else Ul, np.int32)
    return tn, pn, w, labels, Tl, Ul


def _fwd(dev, tn, pn, w, labels, blank, act):
    """sbk_thead_fwd into three buffers of M + 64 floats filled with a
    sentinel; returns them on the CPU (lse, lpb, lpl)."""
    L, ptr, check = _lib()
    B, T, J = tn.shape
    U1, V = pn.shape[1], w.shape[0]
    M = B * T * U1
    code, slope, _ = TR.ACTS[act]
    d = [t.to(dev).contiguous() for t in (tn, pn)]
    wb = _pad_w(w, dev)
    lab = torch.from_numpy(labels).to(dev)
    outs = [torch.full((M + 64,), SENT, device=dev) for _ in range(3)]
    check(L.sbk_thead_fwd(ptr(d[0]), ptr(d[1]), ptr(wb), ptr(lab), B, T, U1, J, V, blank, code, slope,
                          ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), None), "sbk_thead_fwd")
    torch.cuda.synchronize()
    return [o.cpu() for o in outs]


def _check_rows(outs, ref, M):
    """lse, lp_blank, lp_label of every row at 1e-4 * max(1, |ref|); the
    sentinels past M survive.  Returns the worst error / bound."""
    worst = 0.0
    for name, got, want in zip(("lse", "lpb", "lpl"), outs, (ref.lse, ref.lp_blank, ref.lp_label)):
        assert torch.all(got[M:] == SENT), f"{name}: written past row M"
        want = want.reshape(-1)
        err = (got[:M].double() - want).abs()
        tol = 1e-4 * want.abs().clamp_min(1.0)
        bad = ~(err <= tol)
        assert not bad.any(), (f"{name}: {int(bad.sum())} / {M} rows, first {int(bad.nonzero()[0])}, "
                               f"max err {float(err.max()):.3e}")
        worst = max(worst, float((err / tol).max()))
    return worst


# (B, T, U1): M = 70 (one partial tile), 162, 256 (two full tiles)
M70, M162, M256 = (2, 5, 7), (2, 9, 9), (2, 8, 16)


@pytest.mark.parametrize("shape,J,V,blank,act", [
    (M70, 128, 37, 0, "leaky"),
    (M70, 256, 37, 36, "identity"),
    (M162, 512, 128, 127, "relu"),        # the last column of a full chunk
    (M162, 256, 129, 128, "identity"),    # the only valid column of the last chunk
    (M256, 1024, 129, 127, "leaky"),
    (M256, 128, 257, 128, "relu"),        # second chunk
    (M70, 512, 257, 256, "leaky"),        # third chunk, its only valid column
    (M162, 1024, 257, 127, "identity"),
    (M256, 256, 128, 0, "relu"),
    (M70, 128, 129, 0, "identity"),
    (M256, 512, 257, 0, "identity"),
    (M162, 128, 257, 256, "relu"),
])
def test_forward_rows(dev, shape, J, V, blank, act):
    """sbk_thead_fwd, row by row: every J instance, V below / at / one past /
    two past the 128-column chunk, the blank at 0, 127, 128 and V - 1, the
    three joints, labels on the chunk edges."""
    B, T, U1 = shape
    tn, pn, w, labels, Tl, Ul = _case(B, T, U1, J, V, blank, seed=J + V + blank)
    ref = TR.head_reference(tn, pn, w, labels, Tl, Ul, blank, act)
    worst = _check_rows(_fwd(dev, tn, pn, w, labels, blank, act), ref, B * T * U1)
    print(f"forward rows: worst error / bound {worst:.3f}")


def test_online_softmax_moving_maximum(dev):
    """tn and W share a direction d: the rows of W in chunk 0 carry +4d, the
    one of the last chunk -4d, and tn carries +-10d, so that for half of the
    rows chunk 0 holds the row maximum by more than 30 and for the others the
    last chunk does — there the running sum of the earlier chunks has to be
    rescaled by exp(old max - new max) ~ e^-40; dropped, the lse is off by
    log of the stale sum."""
    B, T, U1, J, V, blank = 2, 5, 7, 128, 257, 128
    tn, pn, w, labels, Tl, Ul = _case(B, T, U1, J, V, blank, seed=99)
    d = torch.ones(J) / J ** 0.5
    sign = torch.tensor([1.0, -1.0]).repeat(T)[:T]
    tn = 0.3 * tn + 10.0 * sign[None, :, None] * d
    pn = 0.3 * pn
    w = 0.3 * w
    w[:128] += 4.0 * d
    w[256:] -= 4.0 * d
    ref = TR.head_reference(tn, pn, w, labels, Tl, Ul, blank, "identity")
    lg = ref.logits.reshape(-1, V)
    first, mid, last = lg[:, :128].amax(1), lg[:, 128:256].amax(1), lg[:, 256:].amax(1)
    n_first = int((first - torch.maximum(mid, last) >= 30).sum())
    n_last = int((last - torch.maximum(first, mid) >= 30).sum())
    assert n_first >= 20 and n_last >= 20, (n_first, n_last)
    worst = _check_rows(_fwd(dev, tn, pn, w, labels, blank, "identity"), ref, B * T * U1)
    print(f"moving maximum: {n_first} rows led by chunk 0, {n_last} by the last; worst error / bound {worst:.3f}")


@pytest.mark.parametrize("scale_per_b", [0, 1])
@pytest.mark.parametrize("shape,J,V,blank,act", [
    ((3, 4, 6), 128, 129, 128, "leaky"),
    ((3, 6, 9), 256, 257, 127, "identity"),
    ((3, 4, 6), 512, 37, 36, "relu"),
    ((3, 6, 9), 1024, 128, 0, "leaky"),
    ((4, 8, 8), 256, 129, 5, "relu"),      # M = 256: full tiles only
])
def test_dlogits_elements(dev, shape, J, V, blank, act, scale_per_b):
    """sbk_thead_dlogits, element by element, fed the float64 reference's
    lse and sparse gradients (rounded to fp32): every dS element a against
    the reference b at
        |a - b| <= 2^-8 |b| + 1e-4 |scale_b| (|g_blank| + |g_label|) of its row
    (the first term is bf16 round-to-nearest itself: 8 significand bits, half
    a unit in the last place is at most 2^-8 |b|; the second covers the fp32
    logit error through p (g_b + g_l), where the one-hot cancels — measured
    worst error / bound 0.95, i.e. the rounding term is met, not exceeded).
    Columns >= V are exactly zero, rows past M keep the buffer's sentinel.
    The per-utterance scale (1, -2, 0.5, 3) tells scale[b] from scale[0];
    scale_per_b = 0 passes the single value -1.5.  No element is exempt."""
    L, ptr, check = _lib()
    B, T, U1 = shape
    M = B * T * U1
    tn, pn, w, labels, Tl, Ul = _case(B, T, U1, J, V, blank, seed=J + V + blank + 1)
    scale = list(SCALES[:B]) if scale_per_b else [-1.5]
    ref = TR.head_reference(tn, pn, w, labels, Tl, Ul, blank, act, scale if scale_per_b else scale * B)
    code, slope, _ = TR.ACTS[act]
    Vp = int(L.sbk_thead_vpad(V))
    d_tn, d_pn = tn.to(dev).contiguous(), pn.to(dev).contiguous()
    wb = _pad_w(w, dev)
    lab = torch.from_numpy(labels).to(dev)
    lse, gb, gl = (t.reshape(-1).float().to(dev) for t in (ref.lse, ref.gb, ref.gl))
    sc = torch.tensor(scale, device=dev)
    ds = torch.full((M + 8, Vp), SENT, device=dev, dtype=torch.bfloat16)
    check(L.sbk_thead_dlogits(ptr(d_tn), ptr(d_pn), ptr(wb), ptr(lab), B, T, U1, J, V, blank, code, slope, ptr(lse),
                              ptr(gb), ptr(gl), ptr(sc), scale_per_b, ptr(ds), None), "sbk_thead_dlogits")
    torch.cuda.synchronize()
    ds = ds.cpu().double()
    assert torch.all(ds[M:] == float(torch.tensor(SENT).bfloat16())), "rows past M written"
    assert torch.all(ds[:M, V:] == 0.0), "columns >= V not zero"
    want = ref.dS.reshape(M, V)
    scb = torch.tensor(scale if scale_per_b else scale * B, dtype=torch.float64).abs().reshape(B, 1, 1)
    gsum = ((ref.gb.abs() + ref.gl.abs()) * scb).reshape(M, 1)
    err = (ds[:M, :V] - want).abs()
    tol = 2.0 ** -8 * want.abs() + 1e-4 * gsum
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    print(f"dS: worst error / bound {float(ratio.max()):.3f}")
    bad = ~(err <= tol)
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} elements, first (row, v) = {bad.nonzero()[0].tolist()}"
    # rows outside an utterance's lattice carry no gradient at all
    full = ds[:M, :V].reshape(B, T, U1, V)
    for b in range(B):
        assert torch.all(full[b, Tl[b]:] == 0) and torch.all(full[b, :, Ul[b] + 1:] == 0)


@pytest.mark.parametrize("T,U1,Tl,act", [
    (40, 5, (1, 13, 40), "leaky"),      # T_b U1 = 5, 65, 200
    (9, 8, (8, 9, 3), "relu"),          # 64 (one full step exactly), 72, 24
    (30, 7, (30, 29), "identity"),      # 210, 203: t = r / 7 by float reciprocal
    (67, 3, (67, 22), "leaky"),         # 201, 66: t = r / 3
])
def test_wgrad_alone(dev, T, U1, Tl, act):
    """sbk_thead_wgrad on a bf16 dS of the test's own making (random, zero
    for t >= T_b and in columns >= V), J = 256 and V = 129 (two tiles each
    way): dW against float64 dS^T z elementwise at 1e-5 sum_r |dS| |z| (fp32
    accumulation of a few hundred bf16 x bf16 products, exact each).  Covers
    the row skipping past T_b U1, the r -> (t, u) split by float reciprocal
    and its +-1 correction, and the v >= V store guard: dw has Vp rows and
    those past V keep their sentinel."""
    L, ptr, check = _lib()
    B, J, V = len(Tl), 256, 129
    Vp = int(L.sbk_thead_vpad(V))
    g = torch.Generator().manual_seed(T * U1)
    tn = torch.randn(B, T, J, generator=g)
    pn = torch.randn(B, U1, J, generator=g)
    ds = torch.zeros(B, T, U1, Vp)
    ds[..., :V] = torch.randn(B, T, U1, V, generator=g)
    for b in range(B):
        ds[b, Tl[b]:] = 0.0
    ds = ds.to(torch.bfloat16)
    code, slope, _ = TR.ACTS[act]
    _, z = TR.joint_bf16(tn, pn, slope)
    d64 = ds.double().reshape(-1, Vp)[:, :V]
    z64 = z.reshape(-1, J)
    want = d64.t() @ z64
    bound = 1e-5 * (d64.abs().t() @ z64.abs())
    dw = torch.full((Vp, J), SENT, device=dev)
    dw[:V] = 0.0
    d_ds, d_tn, d_pn = ds.to(dev).contiguous(), tn.to(dev), pn.to(dev)
    d_tl = torch.tensor(Tl, dtype=torch.int32, device=dev)
    check(L.sbk_thead_wgrad(ptr(d_ds), ptr(d_tn), ptr(d_pn), ptr(d_tl), B, T, U1, J, V, code, slope, ptr(dw), None),
          "sbk_thead_wgrad")
    torch.cuda.synchronize()
    dw = dw.cpu().double()
    assert torch.all(dw[V:] == SENT), "dw rows >= V written"
    err = (dw[:V] - want).abs()
    print(f"wgrad: worst error / bound {float((err / bound).max()):.3f}")
    bad = ~(err <= bound)
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} elements, first (v, j) = {bad.nonzero()[0].tolist()}"


def _nrel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


def _head(dev, tn, pn, w, labels, Tl, Ul, blank, act, reduction, use_torchaudio, go):
    from speechbrain_amd.nnet.loss.transducer_head import transducer_head_loss
    T, U = tn.shape[1], labels.shape[1]
    leaves = [t.to(dev).clone().requires_grad_() for t in (tn, pn, w)]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = transducer_head_loss(*leaves, torch.from_numpy(labels).to(dev), torch.from_numpy(Tl / T).float().to(dev),
                                   torch.from_numpy(Ul / U).float().to(dev), blank, reduction, use_torchaudio,
                                   TR.ACTS[act][2]())
    out.backward(torch.ones_like(out) if go is None else torch.tensor(go, device=dev))
    return out.detach().cpu(), [t.grad.cpu() for t in leaves]


@pytest.mark.parametrize("use_torchaudio", [True, False])
@pytest.mark.parametrize("reduction", ["sum", "none"])
@pytest.mark.parametrize("act", ["identity", "relu"])
@pytest.mark.parametrize("J,V,blank", [(128, 37, 5), (256, 129, 128)])
def test_head_loss_end_to_end(dev, J, V, blank, act, reduction, use_torchaudio):
    """transducer_head_loss under bf16 autocast with a blank other than 0
    (5, and V - 1 = 128: alone in the last chunk), the identity and ReLU
    joints, reduction "sum" and "none" with the grad_output (1, -2, 0.5), both
    loss semantics, in a batch that holds a single frame (T_b = 1) and an
    empty transcript (U_b = 0).  Tolerances of test_thead_vs_oracle_rnnt:
    loss 1e-4 relative, gradients 1e-2 normwise (dS and dZ are rounded to
    bf16 before the gradient GEMMs)."""
    B, T, U = 3, 7, 4
    Tl, Ul = np.array([T, 1, T - 2], np.int32), np.array([U, 2, 0], np.int32)
    tn, pn, w, labels, _, _ = _case(B, T, U + 1, J, V, blank, seed=V + blank, Tl=Tl, Ul=Ul)
    go = SCALES[:B] if reduction == "none" else None
    out, grads = _head(dev, tn, pn, w, labels, Tl, Ul, blank, act, reduction, use_torchaudio, go)
    ref = TR.head_reference(tn, pn, w, labels, Tl, Ul, blank, act, TR.grad_scale(B, use_torchaudio, reduction, go))
    want = TR.head_loss(ref, use_torchaudio, reduction)
    assert out.shape == want.shape
    assert torch.all((out.double() - want).abs() <= 1e-4 * want.abs()), (out, want)
    for name, a, b in zip(("dtn", "dpn", "dW"), grads, (ref.dtn, ref.dpn, ref.dW)):
        e = _nrel(a, b)
        print(f"{name}: normwise rel err vs reference {e:.2e}")
        assert e <= 1e-2, f"{name}: {e}"


@pytest.mark.parametrize("use_torchaudio", [True, False])
def test_head_padding_labels_are_never_used(dev, use_torchaudio):
    """Labels at u >= U_b set to 0, -1, V + 3 and 2^31 - 1 in turn: the loss
    and the three gradients are bit-identical and NaN-free (the head's label
    capture and its dS one-hot read labels[b, u] for every u < U).  B = 2, so
    that dW's two fp32 atomic contributions commute."""
    B, T, U, J, V, blank = 2, 5, 4, 128, 129, 128
    Tl, Ul = np.array([T, 3], np.int32), np.array([2, 0], np.int32)
    tn, pn, w, base, _, _ = _case(B, T, U + 1, J, V, blank, seed=5, Tl=Tl, Ul=Ul)
    outs = []
    for pad in (0, -1, V + 3, 2 ** 31 - 1):
        labels = base.copy()
        for b in range(B):
            labels[b, Ul[b]:] = pad
        outs.append(_head(dev, tn, pn, w, labels, Tl, Ul, blank, "leaky", "none", use_torchaudio, (1.0, -2.0)))
    out0, g0 = outs[0]
    ref = TR.head_reference(tn, pn, w, base, Tl, Ul, blank, "leaky", (1.0, -2.0))
    want = TR.head_loss(ref, use_torchaudio, "none")
    assert torch.all((out0.double() - want).abs() <= 1e-4 * want.abs()), (out0, want)
    for a, b in zip(g0, (ref.dtn, ref.dpn, ref.dW)):
        assert _nrel(a, b) <= 1e-2
    for out, g in outs:
        assert torch.isfinite(out).all() and all(torch.isfinite(t).all() for t in g)
        assert torch.equal(out, out0)
        for a, b in zip(g, g0):
            assert (a + 0.0).numpy().tobytes() == (b + 0.0).numpy().tobytes()
