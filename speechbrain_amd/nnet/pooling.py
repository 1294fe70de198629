"""Drop-ins for speechbrain.nnet.pooling.Pooling1d / Pooling2d
(pooling.py:19-240): the reference's constructors and `pool_layer` child, as
thin wrappers over torch's device pooling ops — plumbing, no kernels.  Inside
the CRDNN lobe the frequency max-pool of a CNN_Block runs in the fused
conv + LayerNorm kernel instead (lobes/models/CRDNN.py)."""
import torch
import torch.nn as nn


class Pooling1d(nn.Module):
    def __init__(self, pool_type, kernel_size, input_dims=3, pool_axis=1, ceil_mode=False, padding=0, dilation=1,
                 stride=None):
        super().__init__()
        self.pool_axis = pool_axis
        self.kernel_size = kernel_size
        self.stride = kernel_size if stride is None else stride
        if input_dims not in (3, 4):
            raise ValueError("input_dims must be 3 or 4")
        four = input_dims == 4
        if pool_type == "avg":
            self.pool_layer = (nn.AvgPool2d((1, kernel_size), stride=(1, self.stride), padding=(0, padding),
                                            ceil_mode=ceil_mode) if four else
                               nn.AvgPool1d(kernel_size, stride=self.stride, padding=padding, ceil_mode=ceil_mode))
        elif pool_type == "max":
            self.pool_layer = (nn.MaxPool2d((1, kernel_size), stride=(1, self.stride), padding=(0, padding),
                                            dilation=(1, dilation), ceil_mode=ceil_mode) if four else
                               nn.MaxPool1d(kernel_size, stride=self.stride, padding=padding, dilation=dilation,
                                            ceil_mode=ceil_mode))
        else:
            raise ValueError("pool_type must be 'avg' or 'max'")
        # what the fused CNN_Block kernel can take over: a plain max over kernel = stride bins
        self.plain_max = (pool_type == "max" and self.stride == kernel_size and padding == 0 and dilation == 1
                          and not ceil_mode)

    def forward(self, x):
        # the pooled axis goes last for torch's pooling and back again
        return self.pool_layer(x.transpose(-1, self.pool_axis)).transpose(-1, self.pool_axis)


class Pooling2d(nn.Module):
    def __init__(self, pool_type, kernel_size, pool_axis=(1, 2), ceil_mode=False, padding=0, dilation=1, stride=None):
        super().__init__()
        self.pool_type = pool_type
        self.kernel_size = kernel_size
        self.pool_axis = pool_axis
        self.ceil_mode = ceil_mode
        self.padding = padding
        self.dilation = dilation
        self.stride = kernel_size if stride is None else stride
        cls = nn.AvgPool2d if pool_type == "avg" else nn.MaxPool2d
        self.pool_layer = cls(self.kernel_size, stride=self.stride, padding=self.padding, ceil_mode=self.ceil_mode)

    def forward(self, x):
        # the two pooled axes go last (in their order), every other axis keeps its order
        ax = tuple(self.pool_axis)
        return torch.movedim(self.pool_layer(torch.movedim(x, ax, (-2, -1))), (-2, -1), ax)
