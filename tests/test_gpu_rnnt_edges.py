"""RNN-T loss kernels (csrc/rnnt.hip) at the edges the main suite
(test_gpu_rnnt.py) never reaches: a blank that is not symbol 0, the corners
of the (T_b, U_b) lattice, lattices wider than one wave / one block, and
label padding past U_b.

References: oracle/rnnt.py — `transducer_forward` (the reference's fp32
operation order, which the kernels restate; also run in float64) and
`brute_force_nll` (float64 path enumeration, independent of any α/β
recursion).  Tolerances are those of test_gpu_rnnt.py: 1e-6 in log-prob mode
(same fp32 operations as the oracle) and for the loss, 1e-5 for the gradient
wrt logits (the kernel's fp32 log-softmax against the oracle's float64 one),
all as |a - b| <= rtol * max(1, |b|)."""
import numpy as np
import pytest
import torch

from conftest import assert_close
import oracle.rnnt as OR
import thead_ref as TR

pytestmark = pytest.mark.gpu

MODES = ("lp", "numba", "torchaudio")  # Transducer.apply | transducer_loss(use_torchaudio=False | True)


def _run(dev, mode, logits, labels, Tl, Ul, blank, reduction, go=None):
    """(loss, dense gradient) of one entry point on the GPU, as numpy.
    "lp" feeds the float32 log-probs of the logits to Transducer.apply."""
    from speechbrain_amd.nnet.loss.transducer_loss import Transducer
    from speechbrain_amd.nnet.losses import transducer_loss
    T, U = logits.shape[1], labels.shape[1]
    lab = torch.from_numpy(np.asarray(labels, np.int32)).to(dev)
    if mode == "lp":
        lp = OR.log_softmax(logits.astype(np.float64)).astype(np.float32)
        x = torch.from_numpy(lp).to(dev).requires_grad_()
        loss = Transducer.apply(x, lab, torch.from_numpy(Tl).to(dev), torch.from_numpy(Ul).to(dev), blank, reduction)
    else:
        x = torch.from_numpy(logits).to(dev).requires_grad_()
        loss = transducer_loss(x, lab, torch.from_numpy(Tl / T).float().to(dev),
                               torch.from_numpy(Ul / U).float().to(dev), blank, reduction,
                               use_torchaudio=mode == "torchaudio")
    loss.backward(torch.ones_like(loss) if go is None else torch.as_tensor(go, dtype=torch.float32, device=dev))
    return loss.detach().cpu().numpy(), x.grad.cpu().numpy()


def _oracle(mode, logits, labels, Tl, Ul, blank, reduction, go=None, dtype=np.float32):
    """(loss, dense gradient, per-utterance -log P) of the same entry point
    from oracle/rnnt.py in `dtype` arithmetic."""
    B = logits.shape[0]
    lp = OR.log_softmax(logits.astype(np.float64)).astype(np.float32).astype(dtype)
    loss_b, g_lp, _, beta = OR.transducer_forward(lp, labels, Tl, Ul, blank, "none", dtype)
    if mode == "torchaudio":
        loss_b = -beta[:, 0, 0]
    loss = {"mean": loss_b.mean(dtype=dtype), "sum": loss_b.sum(dtype=dtype), "none": loss_b}[reduction]
    scale = TR.grad_scale(B, mode == "torchaudio", reduction, go).numpy().reshape(B, 1, 1, 1)
    g = g_lp if mode == "lp" else g_lp - np.exp(lp.astype(np.float64)) * g_lp.sum(-1, keepdims=True)
    return np.asarray(loss), g * scale, -beta[:, 0, 0]


def _brute(logits, labels, Tl, Ul, blank):
    lp = OR.log_softmax(logits.astype(np.float64))
    return np.array([OR.brute_force_nll(lp[b], labels[b], int(Tl[b]), int(Ul[b]), blank) for b in range(len(Tl))])


def _per_utterance(mode, nll, Tl):
    return nll if mode == "torchaudio" else nll / Tl


def _assert_zero_outside(g, Tl, Ul):
    for b in range(g.shape[0]):
        assert np.all(g[b, Tl[b]:] == 0.0), f"utterance {b}: gradient at t >= T_b"
        assert np.all(g[b, :, Ul[b] + 1:] == 0.0), f"utterance {b}: gradient at u > U_b"


GO3 = (1.0, -2.0, 0.5)


@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("V,blank", [(7, 0), (7, 3), (7, 6), (70, 0), (70, 3), (70, 69)])
def test_blank_position(dev, V, blank, mode, reduction):
    """blank in {0, 3, V - 1}; V = 70 takes a second pass of the 64-lane
    vocabulary loops.  Labels come from the other V - 1 symbols, so a kernel
    that took symbol 0 (or any fixed column) for the blank reads a label's or
    an unrelated log-prob instead.  "none" is driven by the non-uniform
    grad_output (1, -2, 0.5): a kernel that scaled every utterance by the
    first entry fails.  The loss is also held to brute-force enumeration at
    1e-5 (fp32 lattice of T + U <= 10 steps on fp32 log-probs)."""
    B, T, U = 3, 6, 4
    rng = np.random.default_rng(1000 * V + blank)
    logits = rng.standard_normal((B, T, U + 1, V)).astype(np.float32)
    labels = TR.labels_other_than(rng, blank, V, (B, U))
    Tl = np.array([T, T - 2, 3], np.int32)
    Ul = np.array([U, 2, U - 1], np.int32)
    go = GO3 if reduction == "none" else None
    loss, g = _run(dev, mode, logits, labels, Tl, Ul, blank, reduction, go)
    ref_loss, ref_g, _ = _oracle(mode, logits, labels, Tl, Ul, blank, reduction, go)
    assert_close(loss, ref_loss, rtol=1e-6, name="loss")
    assert_close(g, ref_g, rtol=1e-6 if mode == "lp" else 1e-5, name="grad")
    _assert_zero_outside(g, Tl, Ul)
    per_b = _per_utterance(mode, _brute(logits, labels, Tl, Ul, blank), Tl)
    want = {"mean": per_b.mean(), "sum": per_b.sum(), "none": per_b}[reduction]
    assert_close(loss, np.asarray(want), rtol=1e-5, name="loss vs brute force")


@pytest.mark.parametrize("mode", MODES)
def test_lattice_corners(dev, mode):
    """(T_b, U_b) = (T, U), (1, U), (T, 0), (1, 0), (T - 1, 1) in one batch: a
    single frame (every label emitted at t = 0), an empty transcript (blanks
    only), the 1 x 1 lattice (one blank) and the full one.  Loss against
    brute force, gradients against the oracle, exact zeros outside each
    utterance's lattice; blank = 2 of V = 6."""
    B, T, U, V, blank = 5, 5, 3, 6, 2
    rng = np.random.default_rng(7)
    logits = rng.standard_normal((B, T, U + 1, V)).astype(np.float32)
    labels = TR.labels_other_than(rng, blank, V, (B, U))
    Tl = np.array([T, 1, T, 1, T - 1], np.int32)
    Ul = np.array([U, U, 0, 0, 1], np.int32)
    go = (1.0, -2.0, 0.5, 3.0, -1.0)
    loss, g = _run(dev, mode, logits, labels, Tl, Ul, blank, "none", go)
    ref_loss, ref_g, _ = _oracle(mode, logits, labels, Tl, Ul, blank, "none", go)
    assert np.isfinite(loss).all() and np.isfinite(g).all()
    assert_close(loss, _per_utterance(mode, _brute(logits, labels, Tl, Ul, blank), Tl), rtol=1e-5, name="loss vs brute")
    assert_close(loss, ref_loss, rtol=1e-6, name="loss")
    assert_close(g, ref_g, rtol=1e-6 if mode == "lp" else 1e-5, name="grad")
    _assert_zero_outside(g, Tl, Ul)
    # the 1 x 1 lattice is one blank: -log P = -lp[0, 0, blank]
    lp = OR.log_softmax(logits.astype(np.float64))
    assert_close(loss[3:4], np.array([-lp[3, 0, 0, blank]]), rtol=1e-6, name="1x1")


@pytest.mark.parametrize("U1", [65, 129, 257, 301])
def test_wide_lattice(dev, U1):
    """U + 1 = 65, 129, 257 launch the lattice kernel with 128, 192 and 256
    threads; 257 and 301 take the `u += blockDim.x` loop.  B = 2, T = 4, V = 5,
    U_b = U and U - 3, log-prob mode, where the kernel restates the oracle's
    fp32 operation order: loss, gradient, α and β hold the suite's 1e-6
    against the fp32 oracle even though the α/β sums reach about -500 at
    U = 300.  For the record the test also prints the kernel's distance to the
    float64 oracle over the fp32 oracle's own distance to it (gradients,
    |a - b| / max(1, |b|)); measured on an MI355X: ratio 1.000 at every width
    (both distances 3.5e-5, 7.6e-5, 3.7e-4 and 4.7e-4 at U + 1 = 65, 129, 257
    and 301: the kernel lands on the fp32 oracle's own values)."""
    from speechbrain_amd.nnet.loss.transducer_loss import rnnt_grad, rnnt
    B, T, V, blank, U = 2, 4, 5, 1, U1 - 1
    rng = np.random.default_rng(U1)
    logits = rng.standard_normal((B, T, U1, V)).astype(np.float32)
    labels = TR.labels_other_than(rng, blank, V, (B, U))
    Tl = np.array([T, T - 1], np.int32)
    Ul = np.array([U, U - 3], np.int32)
    lp = OR.log_softmax(logits.astype(np.float64)).astype(np.float32)
    ref_loss, ref_g, ref_a, ref_b = OR.transducer_forward(lp, labels, Tl, Ul, blank, "none")
    _, g64, _, _ = OR.transducer_forward(lp, labels, Tl, Ul, blank, "none", dtype=np.float64)
    x = torch.from_numpy(lp).to(dev)
    lab, tl, ul = (torch.from_numpy(a).to(dev) for a in (labels, Tl, Ul))
    loss, ws = rnnt(x, lab, tl, ul, blank, 2, False, 0)
    go = torch.tensor([1.0, -2.0], device=dev)
    g = rnnt_grad(x, lab, ws, go, blank, 0).cpu().numpy()
    n = B * T * U1
    alpha = ws[3 * n:4 * n].reshape(B, T, U1).cpu().numpy()
    beta = ws[4 * n:5 * n].reshape(B, T, U1).cpu().numpy()
    scale = np.array([1.0, -2.0]).reshape(B, 1, 1, 1)

    def dist(a, b):
        return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
    d_kernel, d_oracle = dist(g.astype(np.float64), g64 * scale), dist(ref_g.astype(np.float64) * scale, g64 * scale)
    print(f"U1={U1}: kernel-f64 {d_kernel:.3e}, fp32 oracle-f64 {d_oracle:.3e}, ratio {d_kernel / d_oracle:.3f}")
    for b in range(B):  # the lattice inside (T_b, U_b); the workspace outside it is not initialised
        sl = (b, slice(0, Tl[b]), slice(0, Ul[b] + 1))
        assert_close(alpha[sl], ref_a[sl], rtol=1e-6, name=f"alpha{b}")
        assert_close(beta[sl], ref_b[sl], rtol=1e-6, name=f"beta{b}")
    assert_close(loss, np.asarray(ref_loss), rtol=1e-6, name="loss")
    assert_close(g, ref_g * scale, rtol=1e-6, name="grad")
    _assert_zero_outside(g, Tl, Ul)


PADDINGS = (0, -1, None, 2 ** 31 - 1)  # None: V + 3


def _bits(a):
    """The array's bytes with -0.0 folded into +0.0: a row outside the
    lattice is 0 * grad_output, whose sign follows grad_output's."""
    return (a + 0.0).tobytes()


@pytest.mark.parametrize("blank", [0, 4])
@pytest.mark.parametrize("mode", MODES)
def test_padding_labels_are_never_used(dev, mode, blank):
    """Both gathers read labels[b, u] for every u < U, whatever U_b is.  The
    values there — 0, -1, V + 3, 2^31 - 1 — must stay out of the loss and the
    dense gradient: bit-identical across the four paddings, no NaN (an
    out-of-range label inside U_b does poison its utterance: test_gpu_rnnt.py).
    With blank = 0 the padding 0 is the blank itself, with blank = 4 it is a
    symbol other utterances emit."""
    B, T, U, V = 3, 5, 4, 9
    rng = np.random.default_rng(11)
    logits = rng.standard_normal((B, T, U + 1, V)).astype(np.float32)
    base = TR.labels_other_than(rng, blank, V, (B, U))
    Tl = np.array([T, 3, T - 1], np.int32)
    Ul = np.array([2, 0, U - 1], np.int32)
    outs = []
    for pad in PADDINGS:
        labels = base.copy()
        for b in range(B):
            labels[b, Ul[b]:] = V + 3 if pad is None else pad
        outs.append(_run(dev, mode, logits, labels, Tl, Ul, blank, "none", GO3))
    loss0, g0 = outs[0]
    assert np.isfinite(loss0).all() and np.isfinite(g0).all()
    ref_loss, ref_g, _ = _oracle(mode, logits, base, Tl, Ul, blank, "none", GO3)
    assert_close(loss0, ref_loss, rtol=1e-6, name="loss")
    assert_close(g0, ref_g, rtol=1e-6 if mode == "lp" else 1e-5, name="grad")
    _assert_zero_outside(g0, Tl, Ul)
    for pad, (loss, g) in zip(PADDINGS[1:], outs[1:]):
        assert np.isfinite(loss).all() and np.isfinite(g).all(), f"padding {pad}: NaN"
        assert _bits(loss) == _bits(loss0), f"padding {pad} changed the loss"
        assert _bits(g) == _bits(g0), f"padding {pad} changed the gradient"
