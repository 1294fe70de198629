"""kldiv_loss / nll_loss on the HIP row kernel (csrc/ctc.hip) against the
reference fixtures and float64 torch."""
import numpy as np
import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu

REDS = ("mean", "batchmean", "batch", "sum", "none")
CASES = ["seq0", "seq1", "seq2", "seq3", "seq4"]


def _call(fn, lp, tg, ln, ls, red):
    from speechbrain_amd.nnet import losses
    if fn == "kldiv":
        return losses.kldiv_loss(lp, tg, ln, label_smoothing=ls, pad_idx=0, reduction=red)
    return losses.nll_loss(lp, tg, ln, label_smoothing=ls, reduction=red)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("fn", ["kldiv", "nll"])
def test_fixtures_every_reduction(golden, dev, case, fn):
    g = golden("losses")
    tg = torch.from_numpy(g[case + ".targets"]).to(dev)
    ln = torch.from_numpy(g[case + ".length"]).to(dev) if case + ".length" in g.files else None
    raises = set(str(r) for r in g[case + ".raises"])
    n = 0
    for li, ls in enumerate((0.0, 0.1)):
        for red in REDS:
            key = f"{fn}.ls{li}.{red}"
            if key in raises:      # the reference itself refuses this combination
                continue
            lp = torch.from_numpy(g[case + ".lp"]).to(dev).requires_grad_()
            out = _call(fn, lp, tg, ln, ls, red)
            assert_close(out, g[f"{case}.{key}.out"], rtol=1e-4, name=f"{case} {key} out")
            out.backward(torch.from_numpy(g[f"{case}.{key}.go"]).to(dev))
            assert_close(lp.grad, g[f"{case}.{key}.grad"], rtol=1e-4, name=f"{case} {key} grad")
            n += 1
    assert n >= 4


def test_length_difference_of_four_raises(golden, dev):
    from speechbrain_amd.nnet import losses
    g = golden("losses")
    lp = torch.from_numpy(g["seq0.lp"]).to(dev)
    tg = torch.from_numpy(g["seq0.targets"]).to(dev)
    with pytest.raises(ValueError, match="same length"):
        losses.nll_loss(lp, torch.cat([tg, tg[:, :4]], 1))
    with pytest.raises(ValueError, match="same length"):
        losses.kldiv_loss(lp, tg[:, :2])


@pytest.fixture(scope="module")
def big():
    B, U, V = 4, 33, 5000
    g = torch.Generator().manual_seed(11)
    lp = torch.randn(B, U, V, generator=g).log_softmax(-1)
    tg = torch.randint(1, V, (B, U), generator=g)
    tg[1, 20:] = 0
    tg[3, 29:] = 0
    ln = torch.tensor([1.0, 0.6, 0.9, 0.88])   # length * U away from integers: one mask in fp32 and fp64
    return lp, tg, ln


def _ref64(fn, lp, tg, ln, ls, red):
    """The reference's formulas (losses.py:405-452, 525-594, 623-687) in
    float64 torch on the CPU."""
    x = lp.double().clone().requires_grad_()
    B, U, V = x.shape
    if fn == "kldiv" and ls > 0:
        q = torch.full_like(x.detach(), ls / (V - 1)).scatter_(2, tg.unsqueeze(-1), 1 - ls)
        loss = torch.nn.functional.kl_div(x, q, reduction="none").masked_fill((tg == 0).unsqueeze(-1), 0)
        out = {"mean": loss.sum(), "batchmean": loss.sum() / B, "batch": loss.view(B, -1).sum(1) / ln.double()}[red]
    else:
        mask = (torch.arange(U)[None, :] < (ln.double() * U)[:, None]).double()
        nll = torch.nn.functional.nll_loss(x.transpose(1, -1), tg, reduction="none") * mask
        reg = x.mean(-1) * mask
        if red == "mean":
            nll, reg = nll.sum() / mask.sum(), reg.sum() / mask.sum()
        elif red == "batchmean":
            nll, reg = nll.sum() / B, reg.sum() / B
        else:
            nll, reg = nll.sum(1) / mask.sum(1), reg.sum(1) / mask.sum(1)
        out = nll if ls == 0 else -ls * reg + (1 - ls) * nll
    go = torch.ones_like(out) if out.dim() == 0 else torch.linspace(0.5, 1.5, out.numel(), dtype=out.dtype)
    out.backward(go)
    return out.detach(), go, x.grad


@pytest.mark.parametrize("fn,ls", [("kldiv", 0.1), ("kldiv", 0.0), ("nll", 0.1)])
@pytest.mark.parametrize("red", ["mean", "batchmean", "batch"])
def test_recipe_vocabulary_vs_float64(dev, big, fn, ls, red):
    lp, tg, ln = big
    ref_out, go, ref_grad = _ref64(fn, lp, tg, ln, ls, red)
    x = lp.to(dev).requires_grad_()
    out = _call(fn, x, tg.to(dev), ln.to(dev), ls, red)
    out.backward(go.float().to(dev))
    assert_close(out, ref_out.float(), rtol=1e-4, name="out")
    assert_close(x.grad, ref_grad.float(), rtol=1e-4, name="grad")


def test_row_kernel_takes_an_unaligned_vocabulary_and_a_slice(dev):
    """V = 1027 (no vector width divides it) and predictions 2 longer than
    the targets (rows of the U-slice are strided across b, not copied)."""
    from speechbrain_amd.nnet import losses
    g = torch.Generator().manual_seed(5)
    lp = torch.randn(3, 9, 1027, generator=g).log_softmax(-1)
    tg = torch.randint(1, 1027, (3, 7), generator=g)
    x = lp.to(dev).requires_grad_()
    out = losses.nll_loss(x, tg.to(dev), reduction="batch")
    out.sum().backward()
    x64 = lp.double().requires_grad_()
    ref = torch.nn.functional.nll_loss(x64[:, :7].transpose(1, -1), tg, reduction="none").sum(1) / 7
    ref.sum().backward()
    assert_close(out, ref.float(), rtol=1e-4, name="out")
    assert_close(x.grad, x64.grad.float(), rtol=1e-4, name="grad")
    assert not x.grad[:, 7:].any()
