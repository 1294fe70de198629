"""Drop-ins for speechbrain.nnet.losses: transducer_loss (losses.py:27-85),
ctc_loss (:245-294), nll_loss (:405-452) and kldiv_loss (:525-594), plus
ctc_loss_from_logits (the fused log-softmax mode, as TransducerLogits).

transducer_loss, use_torchaudio=False: the SpeechBrain Numba semantics
(time-normalised loss, un-normalised gradients), pinned by the reference's
known-answer test.  use_torchaudio=True: torchaudio.functional.rnnt_loss
semantics (-log P, mean over the batch, standard gradients) computed by the
same HIP kernels — torchaudio is not a dependency; this mode's parity is
unpinned by the reference's tests.

ctc_loss: the lattice and the dense gradient are HIP kernels (csrc/ctc.hip);
the reduction over the B per-utterance losses is device-side torch.
nll_loss / kldiv_loss: one HIP pass over the (B, U, V) log-probs gives each
row's target log-prob t and row sum s; loss value and gradient follow from
those two (B, U) tensors, so no (B, U, V) temporary (one-hot, smoothed
distribution, transposed copy) is built.

ContrastiveLoss (:1198-1251): one HIP kernel per row of x scores the positive
and the negatives (cosine similarity, neg_is_pos, log-sum-exp, arg-max) with
the candidate rows read in place; the sum over rows and the accuracy ratio are
device-side torch (csrc/w2vloss.hip).
"""
import math

import torch
import torch.nn as nn

from .loss.ctc_loss import ctc_nll, row_stats
from .loss.transducer_loss import TransducerLogits


def transducer_loss(logits, targets, input_lens, target_lens, blank_index, reduction="mean", use_torchaudio=True):
    input_lens = (input_lens * logits.shape[1]).round().int()
    target_lens = (target_lens * targets.shape[1]).round().int()
    if use_torchaudio:
        return TransducerLogits.apply(logits, targets, input_lens, target_lens, blank_index, reduction, 1)
    return TransducerLogits.apply(logits, targets, input_lens, target_lens, blank_index, reduction, 0)


def _ctc(x, targets, input_lens, target_lens, blank_index, reduction, is_logits):
    if reduction not in ("mean", "sum", "none", "batch", "batchmean"):
        raise ValueError("{} is not a valid value for reduction".format(reduction))
    input_lens = (input_lens * x.shape[1]).round().int()
    target_lens = (target_lens * targets.shape[1]).round().int()
    loss = ctc_nll(x, targets, input_lens, target_lens, blank_index, is_logits)
    if reduction == "mean":
        # torch: each utterance's loss over its target length, then the batch mean
        return (loss / target_lens.clamp(min=1).to(loss.dtype)).mean()
    if reduction == "sum":
        return loss.sum()
    if reduction == "batchmean":
        return loss.sum() / targets.shape[0]
    if reduction == "batch":
        N = loss.size(0)
        return loss.view(N, -1).sum(1) / target_lens.view(N, -1).sum(1)
    return loss


def ctc_loss(log_probs, targets, input_lens, target_lens, blank_index, reduction="mean"):
    """losses.py:245-294: log_probs (B, T, V), targets (B, L) without blanks,
    relative lengths; reductions mean | sum | none | batch | batchmean.  An
    utterance without a valid alignment gives loss 0 and a zero gradient
    (zero_infinity=True)."""
    return _ctc(log_probs, targets, input_lens, target_lens, blank_index, reduction, False)


def ctc_loss_from_logits(logits, targets, input_lens, target_lens, blank_index, reduction="mean"):
    """ctc_loss(logits.log_softmax(-1), ...) with the log-softmax fused into
    the loss: no log-prob tensor, and the gradient wrt the logits
    (softmax - occupancy) is written in one pass."""
    return _ctc(logits, targets, input_lens, target_lens, blank_index, reduction, True)


def truncate(predictions, targets, allowed_len_diff=3):
    """losses.py:597-620."""
    len_diff = predictions.shape[1] - targets.shape[1]
    if len_diff == 0:
        return predictions, targets
    elif abs(len_diff) > allowed_len_diff:
        raise ValueError("Predictions and targets should be same length, but got %s and "
                         "%s respectively." % (predictions.shape[1], targets.shape[1]))
    elif len_diff < 0:
        return predictions, targets[:, : predictions.shape[1]]
    else:
        return predictions[:, : targets.shape[1]], targets


def nll_loss(log_probabilities, targets, length=None, label_smoothing=0.0, allowed_len_diff=3, reduction="mean"):
    """losses.py:405-452 with compute_masked_loss (:623-687): log_probabilities
    (B, V) or (B, U, V), targets (B,) or (B, U), relative length (B,).
    reduction mean | batch | batchmean; any other value returns the masked
    per-position losses, as the reference does."""
    if len(log_probabilities.shape) == 3:
        log_probabilities, targets = truncate(log_probabilities, targets, allowed_len_diff)
        lp3, tg2 = log_probabilities, targets
    else:
        lp3, tg2 = log_probabilities.unsqueeze(1), targets.unsqueeze(1)
    V = lp3.shape[2]
    t, s = row_stats(lp3, tg2)
    mask = torch.ones_like(t)
    if length is not None:
        U = targets.shape[1]
        mask = (torch.arange(U, device=t.device, dtype=length.dtype)[None, :] < (length * U)[:, None]).to(t.dtype)
    t, s, mask = (v.reshape(targets.shape) for v in (t, s, mask))

    def reduce(v):
        N = v.size(0)
        if reduction == "mean":
            return v.sum() / mask.sum()
        if reduction == "batchmean":
            return v.sum() / N
        if reduction == "batch":
            return v.reshape(N, -1).sum(1) / mask.reshape(N, -1).sum(1)
        return v

    loss = reduce(-t * mask)
    if label_smoothing == 0:
        return loss
    loss_reg = reduce(s / V * mask)  # torch.mean(predictions, dim=1) * mask
    return -label_smoothing * loss_reg + (1 - label_smoothing) * loss


def _xlogx(v):
    return v * math.log(v) if v > 0 else 0.0


def kldiv_loss(log_probabilities, targets, length=None, label_smoothing=0.0, allowed_len_diff=3, pad_idx=0,
               reduction="mean"):
    """losses.py:525-594.  label_smoothing > 0: KL(q || p) of the smoothed
    target q (1 - ls at the target, ls / (V - 1) elsewhere), zero on rows
    whose target is pad_idx; per row that is
    C - (eps·(s - t) + (1 - ls)·t), C = (V - 1)·eps·log eps + (1 - ls)·log(1 - ls).
    label_smoothing == 0: nll_loss."""
    if label_smoothing > 0:
        if log_probabilities.dim() == 2:
            log_probabilities = log_probabilities.unsqueeze(1)
        bz, time, n_class = log_probabilities.shape
        targets = targets.long().detach()
        confidence = 1 - label_smoothing
        eps = label_smoothing / (n_class - 1)
        targets = targets.reshape(bz, time)
        ignore = targets == pad_idx
        targets = targets.masked_fill(ignore, 0)
        t, s = row_stats(log_probabilities, targets)
        const = (n_class - 1) * _xlogx(eps) + _xlogx(confidence)
        rows = (const - (eps * (s - t) + confidence * t)).masked_fill(ignore, 0)
        if reduction == "mean":
            return rows.sum().mean()
        elif reduction == "batchmean":
            return rows.sum() / bz
        elif reduction == "batch":
            return rows.view(bz, -1).sum(1) / length
        elif reduction == "sum":
            return rows.sum()
        else:
            # the reference returns the elementwise (B·U, V) KL terms here: the
            # dense result is the output itself, written with device-side torch
            lp = log_probabilities.reshape(-1, n_class)
            hit = torch.arange(n_class, device=lp.device)[None, :] == targets.reshape(-1, 1)
            loss = torch.where(hit, _xlogx(confidence) - confidence * lp, _xlogx(eps) - eps * lp)
            return loss.masked_fill(ignore.reshape(-1, 1), 0)
    else:
        return nll_loss(log_probabilities, targets, length, reduction=reduction)


class ContrastiveLoss(nn.Module):
    """losses.py:1198-1251.  forward(x, y, negs) → (loss, accuracy) for x, y
    (B, T, C) and negs either
      float (N, B, T, C)   the reference's call (sample_negatives): the kernel
                           reads the candidate rows straight from negs;
      integer (B, T·N)     lobes.models.wav2vec.sample_negative_indices: row
                           indices into y.view(-1, C), negs is never built.
    Both give the same values and gradients (wrt x, y and float negs).
    Always computed in fp32, also under bf16 autocast: the reference's
    `.type_as(x)` would round the cosine logits to x's dtype before the
    cross-entropy; here they stay fp32 and the loss is returned in fp32."""

    def __init__(self, logit_temp):
        super().__init__()
        self.logit_temp = logit_temp

    def forward(self, x, y, negs):
        from .. import _w2v
        rowloss, correct, _ = _w2v.contrastive_rows(x, y, negs, self.logit_temp)
        return rowloss.sum(), correct.detach().sum() / correct.numel()
