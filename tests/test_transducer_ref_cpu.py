"""tests/thead_ref.py (the float64 yardstick of the transducer-head and RNN-T
edge tests on the GPU) against two independent statements of the same
algebra, on the CPU:

  * torch.autograd in float64: the joint with a straight-through bf16
    rounding, the projection, log-softmax and an α-only lattice written with
    torch.logsumexp — no β, no hand-written gradient — give dS, dtn, dpn, dW;
  * oracle.rnnt.brute_force_nll: the loss by path enumeration.

Cases: blank at 0, in the middle and at V - 1; an empty transcript (U_b = 0);
a single frame (T_b = 1); identity, ReLU and LeakyReLU joints; a non-uniform
per-utterance gradient scale."""
import numpy as np
import pytest
import torch

import oracle.rnnt as OR
import thead_ref as TR

B, T, U, J, V = 3, 4, 3, 8, 6
TL = np.array([4, 1, 3])
UL = np.array([3, 2, 0])
SCALE = (1.0, -2.0, 0.5)


def _case(blank, seed=0):
    g = torch.Generator().manual_seed(seed)
    tn = torch.randn(B, T, J, generator=g)
    pn = torch.randn(B, U + 1, J, generator=g)
    w = torch.randn(V, J, generator=g)
    labels = TR.labels_other_than(np.random.default_rng(seed), blank, V, (B, U))
    return tn, pn, w, labels


def _nll_torch(lp, y, Tb, Ub, blank):
    alpha = {}
    for t in range(Tb):
        for u in range(Ub + 1):
            terms = []
            if t > 0:
                terms.append(alpha[t - 1, u] + lp[t - 1, u, blank])
            if u > 0:
                terms.append(alpha[t, u - 1] + lp[t, u - 1, int(y[u - 1])])
            alpha[t, u] = torch.logsumexp(torch.stack(terms), 0) if terms else lp.new_zeros(())
    return -(alpha[Tb - 1, Ub] + lp[Tb - 1, Ub, blank])


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("act", ["identity", "relu", "leaky"])
@pytest.mark.parametrize("blank", [0, 2, V - 1])
def test_reference_vs_float64_autograd(act, blank):
    tn, pn, w, labels = _case(blank)
    ref = TR.head_reference(tn, pn, w, labels, TL, UL, blank, act, SCALE)
    slope = TR.ACTS[act][1]
    tn64, pn64, w64 = (t.double().requires_grad_() for t in (tn, pn, w))
    pre = tn64[:, :, None, :] + pn64[:, None, :, :]
    a = torch.where(pre >= 0, pre, pre * slope)
    z = a + (ref.z - a).detach()                      # bf16 rounding, straight through
    wq = w64 + (ref.wb - w64).detach()
    logits = z @ wq.t()
    logits.retain_grad()
    lp = torch.log_softmax(logits, -1)
    nll = torch.stack([_nll_torch(lp[b], labels[b], int(TL[b]), int(UL[b]), blank) for b in range(B)])
    (nll * torch.tensor(SCALE, dtype=torch.float64)).sum().backward()
    assert _rel(ref.nll, nll.detach()) <= 1e-12
    assert _rel(ref.loss_numba, nll.detach() / torch.from_numpy(TL)) <= 1e-12
    assert _rel(ref.logits, logits.detach()) <= 1e-12
    assert _rel(ref.lse, torch.logsumexp(logits.detach(), -1)) <= 1e-12
    assert _rel(ref.lp_blank, lp.detach()[..., blank]) <= 1e-12
    for u in range(U):
        for b in range(B):
            assert _rel(ref.lp_label[b, :, u], lp.detach()[b, :, u, int(labels[b, u])]) <= 1e-12
    assert torch.all(ref.lp_label[:, :, U] == 0)
    for name, got, want in (("dS", ref.dS, logits.grad), ("dtn", ref.dtn, tn64.grad), ("dpn", ref.dpn, pn64.grad),
                            ("dW", ref.dW, w64.grad)):
        assert _rel(got, want) <= 1e-10, (name, _rel(got, want))
    # exact zeros outside each utterance's lattice
    for b in range(B):
        assert torch.all(ref.dS[b, TL[b]:] == 0) and torch.all(ref.dS[b, :, UL[b] + 1:] == 0)
    # sparse gradients: dS row = onehot_blank * gb + onehot_label * gl - p * (gb + gl), scaled
    p = lp.detach().exp()
    sc = torch.tensor(SCALE, dtype=torch.float64).reshape(B, 1, 1)
    want = -p * ((ref.gb + ref.gl) * sc)[..., None]
    want[..., blank] += ref.gb * sc
    for b in range(B):
        for u in range(int(UL[b])):
            want[b, :, u, int(labels[b, u])] += (ref.gl * sc)[b, :, u]
    assert _rel(ref.dS, want) <= 1e-12


@pytest.mark.parametrize("act", ["identity", "relu", "leaky"])
@pytest.mark.parametrize("blank", [0, 2, V - 1])
def test_reference_loss_vs_brute_force(act, blank):
    tn, pn, w, labels = _case(blank, seed=1)
    ref = TR.head_reference(tn, pn, w, labels, TL, UL, blank, act)
    lp = torch.log_softmax(ref.logits, -1).numpy()
    for b in range(B):
        bf = OR.brute_force_nll(lp[b], labels[b], int(TL[b]), int(UL[b]), blank)
        assert abs(float(ref.nll[b]) - bf) <= 1e-10 * max(1.0, abs(bf)), (b, float(ref.nll[b]), bf)
    for use_torchaudio in (True, False):
        per_b = ref.nll if use_torchaudio else ref.nll / torch.from_numpy(TL)
        assert torch.equal(TR.head_loss(ref, use_torchaudio, "none"), per_b)
        assert float(TR.head_loss(ref, use_torchaudio, "sum")) == pytest.approx(float(per_b.sum()), rel=1e-14)
        assert float(TR.head_loss(ref, use_torchaudio, "mean")) == pytest.approx(float(per_b.mean()), rel=1e-14)


def test_grad_scale_semantics():
    """The torchaudio mean divides by B; the Numba semantics never do."""
    assert torch.equal(TR.grad_scale(4, True, "mean"), torch.full((4,), 0.25, dtype=torch.float64))
    assert torch.equal(TR.grad_scale(4, False, "mean"), torch.ones(4, dtype=torch.float64))
    assert torch.equal(TR.grad_scale(4, True, "sum"), torch.ones(4, dtype=torch.float64))
    assert torch.equal(TR.grad_scale(3, True, "none", SCALE), torch.tensor(SCALE, dtype=torch.float64))


def test_joint_rounding_is_the_kernels():
    """z is rounded from the fp32 sum (not from a float64 one), and the
    activations are max(v, slope v): ReLU and identity are the slope 0 and 1."""
    tn, pn, _, _ = _case(0, seed=2)
    pre, z = TR.joint_bf16(tn, pn, 0.0)
    assert pre.dtype == torch.float32 and torch.equal(pre, tn[:, :, None, :] + pn[:, None, :, :])
    assert torch.equal(z, torch.relu(pre).to(torch.bfloat16).double())
    assert torch.equal(TR.joint_bf16(tn, pn, 1.0)[1], pre.to(torch.bfloat16).double())
    assert torch.equal(TR.joint_bf16(tn, pn, 0.01)[1],
                       torch.nn.functional.leaky_relu(pre, 0.01).to(torch.bfloat16).double())
