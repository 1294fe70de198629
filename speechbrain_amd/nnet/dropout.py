"""Drop-in for speechbrain.nnet.dropout.Dropout2d (dropout.py:13-56).

The reference moves (batch, time, channel1, channel2) to (batch, channel1,
channel2, time) before nn.Dropout2d, so the feature maps it drops are the
(batch, channel1) pairs: for the CRDNN's (B, T, F, C) activations, whole
frequency bins of an utterance.  `mask(B, F, device)` draws exactly that
(B, F) keep / (1 - p) mask with torch's own feature dropout on the device;
forward multiplies by it.  The fused CNN_Block kernel takes the mask as its
scale operand instead (lobes/models/CRDNN.py).  Plumbing, no kernels."""
import torch
import torch.nn as nn


class Dropout2d(nn.Module):
    def __init__(self, drop_rate, inplace=False):
        super().__init__()
        self.drop_rate = drop_rate
        self.inplace = inplace
        self.drop = nn.Dropout2d(p=self.drop_rate, inplace=self.inplace)

    def mask(self, B, F, device):
        """(B, F) fp32: 0 or 1 / (1 - p) per (utterance, bin); None when nothing is dropped."""
        if not self.training or self.drop_rate == 0:
            return None
        return self.drop(torch.ones(B, F, 1, 1, device=device)).view(B, F)

    def forward(self, x, mask=None):
        if mask is None:
            mask = self.mask(x.shape[0], x.shape[2], x.device)
        if mask is None:
            return x
        mask = mask.to(x.dtype).view(x.shape[0], 1, x.shape[2], *([1] * (x.dim() - 3)))
        return x.mul_(mask) if self.inplace else x * mask
