"""HIP CTC loss (csrc/ctc.hip) against the reference fixtures and against
torch.nn.functional.ctc_loss in float64 on the CPU."""
import functools

import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu

REDS = ("mean", "sum", "none", "batch", "batchmean")


def _close_nonfinite_aware(a, b, name):
    """assert_close on the finite entries of b; its inf / NaN entries (the
    reference's own 0/0 and x/0 of reduction "batch") must match exactly."""
    a = a.detach().cpu().numpy()
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin), name
    assert np.array_equal(a[~fin], b[~fin], equal_nan=True), name
    assert_close(a[fin], b[fin], rtol=1e-4, name=name)


@pytest.mark.parametrize("case", ["ctc0", "ctc1", "ctc2", "ctc3"])
@pytest.mark.parametrize("mode", ["lp", "logits"])
def test_fixtures(golden, dev, case, mode):
    from speechbrain_amd.nnet.losses import ctc_loss, ctc_loss_from_logits
    g = golden("losses")
    fn = ctc_loss if mode == "lp" else ctc_loss_from_logits
    gkey = "grad" if mode == "lp" else "grad_logits"
    targets = torch.from_numpy(g[case + ".targets"]).to(dev)
    ilen = torch.from_numpy(g[case + ".ilen"]).to(dev)
    tlen = torch.from_numpy(g[case + ".tlen"]).to(dev)
    blank = int(g[case + ".blank"])
    n_grads = 0
    for red in REDS:
        x = torch.from_numpy(g[f"{case}.{mode}"]).to(dev).requires_grad_()
        out = fn(x, targets, ilen, tlen, blank, reduction=red)
        _close_nonfinite_aware(out, g[f"{case}.{red}.out"], f"{case} {mode} {red} out")
        if f"{case}.{red}.{gkey}" in g.files:
            out.backward(torch.from_numpy(g[f"{case}.{red}.go"]).to(dev))
            assert_close(x.grad, g[f"{case}.{red}.{gkey}"], rtol=1e-4, name=f"{case} {mode} {red} grad")
            # the infeasible row (3) has loss 0 and an all-zero gradient; frames past input_len too
            assert not x.grad[3].any()
            n_grads += 1
    assert n_grads == 4


# (B, T, V, L)
SHAPES = [(3, 50, 1027, 20), (2, 130, 37, 32), (2, 300, 37, 130), (2, 720, 37, 350), (4, 376, 5000, 120)]


def _inputs(B, T, V, L):
    g = torch.Generator().manual_seed(B * 1000003 + T * 1009 + V * 13 + L)
    logits = torch.randn(B, T, V, generator=g)
    targets = torch.randint(1, V, (B, L), generator=g)
    il = torch.tensor([T - 7 * b for b in range(B)])          # uneven, row 0 full
    tl = torch.tensor([L - 3 * b for b in range(B)])
    return logits, targets, il, tl


def _torch_cpu(x, targets, il, tl, is_logits, dtype):
    """Per-utterance loss and the gradient of their sum wrt x: torch's own
    ctc_loss on the CPU in dtype (the function the reference calls)."""
    x = x.detach().to(dtype).clone().requires_grad_()
    lp = x.log_softmax(-1) if is_logits else x
    loss = torch.nn.functional.ctc_loss(lp.transpose(0, 1), targets, il, tl, 0, reduction="none", zero_infinity=True)
    loss.sum().backward()
    return loss.detach(), x.grad


@functools.lru_cache(maxsize=None)
def _case(shape, is_logits):
    logits, targets, il, tl = _inputs(*shape)
    x = logits if is_logits else logits.log_softmax(-1)
    l64, g64 = _torch_cpu(x, targets, il, tl, is_logits, torch.float64)
    l32, g32 = _torch_cpu(x, targets, il, tl, is_logits, torch.float32)
    return x, targets, il, tl, l64, g64, (l32.double() - l64).abs().max().item(), (g32.double() - g64).abs().max().item()


def _ours(dev, x, targets, il, tl, is_logits):
    from speechbrain_amd.nnet.losses import ctc_loss, ctc_loss_from_logits
    B, T, _ = x.shape
    xd = x.to(dev).requires_grad_()
    loss = (ctc_loss_from_logits if is_logits else ctc_loss)(
        xd, targets.to(dev), (il / T).float().to(dev), (tl / targets.shape[1]).float().to(dev), 0, reduction="none")
    loss.sum().backward()
    return loss.detach(), xd.grad


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("is_logits", [False, True], ids=["lp", "logits"])
def test_vs_float64(dev, shape, is_logits):
    """Loss at 1e-4 relative.  Gradient: max|ours - f64| <= max(1e-4,
    2 x max|torch CPU fp32 - f64|) on the same inputs — at nll in the
    thousands torch's own fp32 gradient is ~1e-3 off float64 (cancellation in
    α + β + nll - lp); the factor 2 allows a different, equally valid
    summation order."""
    x, targets, il, tl, l64, g64, torch_loss_err, torch_grad_err = _case(shape, is_logits)
    loss, grad = _ours(dev, x, targets, il, tl, is_logits)
    loss_err = ((loss.cpu().double() - l64).abs() / l64.abs()).max().item()
    grad_err = (grad.cpu().double() - g64).abs().max().item()
    bound = max(1e-4, 2 * torch_grad_err)
    print(f"ctc {shape} {'logits' if is_logits else 'lp'}: nll max {l64.max().item():.1f}, loss rel err "
          f"{loss_err:.3e} (torch fp32 abs {torch_loss_err:.3e}), grad abs err {grad_err:.3e}, "
          f"torch fp32 grad abs err {torch_grad_err:.3e}, bound {bound:.3e}")
    assert torch.isfinite(l64).all() and (l64 > 0).all()
    assert loss_err <= 1e-4
    assert grad_err <= bound
    B, T, _ = x.shape
    for b in range(B):
        assert not grad[b, int(il[b]):].any()      # frames past input_len: exactly zero


def test_gradient_is_bit_identical_between_runs(dev):
    x, targets, il, tl = _case((2, 300, 37, 130), True)[:4]
    _, g1 = _ours(dev, x, targets, il, tl, True)
    _, g2 = _ours(dev, x, targets, il, tl, True)
    assert torch.equal(g1, g2)
    _, g3 = _ours(dev, x.log_softmax(-1), targets, il, tl, False)
    _, g4 = _ours(dev, x.log_softmax(-1), targets, il, tl, False)
    assert torch.equal(g3, g4)


@pytest.mark.parametrize("is_logits", [False, True], ids=["lp", "logits"])
def test_graph_capture_replays_the_eager_result(dev, is_logits):
    """Forward + backward hold no host synchronisation: captured once with
    torch.cuda.graph and replayed twice, the replay equals eager exactly."""
    from speechbrain_amd.nnet.losses import ctc_loss, ctc_loss_from_logits
    fn = ctc_loss_from_logits if is_logits else ctc_loss
    x, targets, il, tl = _case((3, 50, 1027, 20), is_logits)[:4]
    B, T, _ = x.shape
    tg, ilr, tlr = targets.to(dev), (il / T).float().to(dev), (tl / targets.shape[1]).float().to(dev)

    def eager():
        # its own leaf, and no autograd graph outliving the call: a live graph
        # would keep that leaf's gradient-accumulation node, bound to the
        # stream it was built on, and a backward captured later on another
        # stream would fork the capture through that stream
        xe = x.to(dev).requires_grad_()
        loss = fn(xe, tg, ilr, tlr, 0)
        loss.backward()
        return loss.detach().clone(), xe.grad.clone()

    eager_loss, eager_grad = eager()
    xs = x.to(dev).requires_grad_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        xs.grad = None
        fn(xs, tg, ilr, tlr, 0).backward()
    torch.cuda.current_stream().wait_stream(side)
    xs.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_loss = fn(xs, tg, ilr, tlr, 0)
        static_loss.backward()
    for _ in range(2):
        xs.grad.fill_(-1.0)
        static_loss.detach().fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_loss.detach(), eager_loss)
        assert torch.equal(xs.grad, eager_grad)


def test_padding_values_are_never_read(dev):
    """targets[b, j >= target_len[b]] holds V-1 in one run and 0 in another:
    identical results, equal to torch's."""
    B, T, V, L = 3, 30, 11, 6
    g = torch.Generator().manual_seed(7)
    logits = torch.randn(B, T, V, generator=g)
    targets = torch.randint(1, V - 1, (B, L), generator=g)
    il, tl = torch.tensor([30, 22, 9]), torch.tensor([6, 3, 0])
    res = []
    for pad in (V - 1, 0):
        tp = targets.clone()
        for b in range(B):
            tp[b, int(tl[b]):] = pad
        res.append(_ours(dev, logits, tp, il, tl, True))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    l64, g64 = _torch_cpu(logits, targets, il, tl, True, torch.float64)
    assert_close(res[0][0], l64.float(), rtol=1e-4, name="loss")
    assert_close(res[0][1], g64.float(), rtol=1e-4, name="grad")


def test_state_bound_has_its_own_error(dev):
    from speechbrain_amd._lib import SbkError
    from speechbrain_amd.nnet.losses import ctc_loss
    x = torch.zeros(1, 2, 3, device=dev)
    with pytest.raises(SbkError, match="1002"):
        ctc_loss(x, torch.ones(1, 1537, dtype=torch.long, device=dev), torch.ones(1, device=dev),
                 torch.ones(1, device=dev), 0)
