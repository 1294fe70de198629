"""Drop-in for speechbrain.nnet.normalization.LayerNorm (normalization.py:172-223)
on the HIP LayerNorm kernel (state_dict keys: norm.weight, norm.bias), and
BatchNorm1d (normalization.py:12-100; norm.weight, norm.bias, norm.running_*)
as a thin wrapper over torch's device batch norm."""
import math

import torch

from .. import _autograd as A
from .. import _enc


class LayerNorm(torch.nn.Module):
    def __init__(self, input_size=None, input_shape=None, eps=1e-05, elementwise_affine=True):
        super().__init__()
        self.eps = eps
        self.elementwise_affine = elementwise_affine
        if input_shape is not None:
            input_size = input_shape[2:]
        self.norm = torch.nn.LayerNorm(input_size, eps=self.eps, elementwise_affine=self.elementwise_affine)

    def forward(self, x):
        shp = self.norm.normalized_shape
        D = int(math.prod(shp))
        if not self.elementwise_affine:
            raise NotImplementedError("LayerNorm without affine parameters is not on the hot path")
        if A.needs_grad(self, x):
            return A.layer_norm(x.float().reshape(-1, D), self.norm).view(x.shape)
        y, _ = _enc.layernorm(x.float().reshape(-1, D).contiguous(), self.norm.weight.detach().reshape(-1),
                              self.norm.bias.detach().reshape(-1), self.eps)
        return y.view(x.shape)


class BatchNorm1d(torch.nn.Module):
    def __init__(self, input_shape=None, input_size=None, eps=1e-05, momentum=0.1, affine=True,
                 track_running_stats=True, combine_batch_time=False, skip_transpose=False):
        super().__init__()
        self.combine_batch_time = combine_batch_time
        self.skip_transpose = skip_transpose
        if input_size is None:
            input_size = input_shape[1] if skip_transpose else input_shape[-1]
        self.norm = torch.nn.BatchNorm1d(input_size, eps=eps, momentum=momentum, affine=affine,
                                         track_running_stats=track_running_stats)

    def forward(self, x):
        shp = x.shape
        if self.combine_batch_time:
            x = x.reshape(shp[0] * shp[1], shp[2]) if x.ndim == 3 else x.reshape(shp[0] * shp[1], shp[3], shp[2])
            return self.norm(x).reshape(shp)
        if self.skip_transpose:
            return self.norm(x)
        return self.norm(x.transpose(-1, 1)).transpose(1, -1)
