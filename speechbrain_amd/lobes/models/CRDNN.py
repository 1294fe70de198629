"""Drop-in for speechbrain.lobes.models.CRDNN (CRDNN, CNN_Block, DNN_Block;
CRDNN.py:14-311): the `enc:` of the LibriSpeech / TIMIT seq2seq recipes and
of the LibriSpeech transducer recipe.  Constructor arguments, defaults and
state_dict keys are the reference's (CNN.block_0.conv_1.conv.weight,
CNN.block_0.norm_1.norm.weight, DNN.block_0.linear.w.weight,
DNN.block_0.norm.norm.running_mean, RNN.*), so its checkpoints load with
strict=True.

A CNN_Block is twice (Conv2d 3x3 stride 1 "same" reflect -> LayerNorm over
(freq, chan) -> LeakyReLU), a max-pool and a Dropout2d.  With
CRDNN.USE_FUSED_CNN each conv + norm + activation is one launch of
csrc/convln.hip (_autograd.CnnBlockFn), the second one with the 1-D
frequency pool and the Dropout2d mask folded in; shapes outside that kernel's
set, and every shape with the flag off, run on im2col + MFMA GEMM + wide
LayerNorm + LeakyReLU (_autograd.ConvBlockFn) followed by the pooling and
dropout wrappers.  The RNN is the package's LiGRU / LSTM / GRU, the DNN
blocks its Linear (MFMA GEMM) + BatchNorm1d + LeakyReLU + Dropout.  Shapes
are inferred arithmetically: no dummy forward runs at construction."""
import torch
import torch.nn as nn

from ... import _autograd as A
from ... import _enc
from ...nnet.CNN import Conv2d
from ...nnet.RNN import LiGRU
from ...nnet.dropout import Dropout2d
from ...nnet.linear import Linear
from ...nnet.normalization import BatchNorm1d, LayerNorm
from ...nnet.pooling import Pooling1d, Pooling2d
from .convolution import _Named


class _Seq(_Named):
    """Named layers applied in order; of a tuple (an RNN's output, state) the first goes on."""

    def forward(self, x):
        for layer in self.children():
            x = layer(x)
            if isinstance(x, tuple):
                x = x[0]
        return x


def _concrete(shape):
    """The reference Sequential's stand-ins for unknown sizes: batch 1, any other axis 256."""
    return tuple((1 if i == 0 else 256) if d is None else int(d) for i, d in enumerate(shape))


class CNN_Block(_Seq):
    def __init__(self, input_shape, channels, kernel_size=[3, 3], activation=torch.nn.LeakyReLU, using_2d_pool=False,
                 pooling_size=2, dropout=0.15):
        super().__init__()
        shape = _concrete(input_shape)
        for i in (1, 2):
            conv = self.add(f"conv_{i}", Conv2d(out_channels=channels, kernel_size=tuple(kernel_size),
                                               input_shape=shape))
            shape = conv.out_shape(shape)
            self.add(f"norm_{i}", LayerNorm(input_shape=shape))
            self.add(f"act_{i}", activation())
        if using_2d_pool:
            self.add("pooling", Pooling2d(pool_type="max", kernel_size=(pooling_size, pooling_size), pool_axis=(1, 2)))
            shape = (shape[0], shape[1] // pooling_size, shape[2] // pooling_size, shape[3])
        else:
            self.add("pooling", Pooling1d(pool_type="max", input_dims=4, kernel_size=pooling_size, pool_axis=2))
            shape = (shape[0], shape[1], shape[2] // pooling_size, shape[3])
        self.add("drop", Dropout2d(drop_rate=dropout))
        self.out_shape = shape
        self._wc = _enc.WeightCache()

    def _kernel_layer(self, i):
        """conv_i + norm_i + act_i as one conv + LayerNorm + LeakyReLU call (A.cnn_block)."""
        conv, norm, act = getattr(self, f"conv_{i}"), getattr(self, f"norm_{i}"), getattr(self, f"act_{i}")
        return (isinstance(act, nn.LeakyReLU) and isinstance(norm, LayerNorm) and norm.elementwise_affine
                and tuple(conv.kernel_size) == (3, 3) and conv.stride == (1, 1) and conv.dilation == (1, 1)
                and conv.padding == "same" and conv.padding_mode == "reflect" and conv.groups == 1
                and not conv.skip_transpose)

    def forward(self, x):
        if x.dim() == 3:
            x = x.unsqueeze(-1)
        dtype = _enc.compute_dtype()
        fused = CRDNN.USE_FUSED_CNN
        # the 1-D frequency max-pool and the Dropout2d mask ride in the second layer's launch
        fold = (fused and self._kernel_layer(2) and isinstance(self.pooling, Pooling1d) and self.pooling.plain_max
                and self.pooling.pool_axis == 2)
        for i in (1, 2):
            conv, norm, act = getattr(self, f"conv_{i}"), getattr(self, f"norm_{i}"), getattr(self, f"act_{i}")
            if not self._kernel_layer(i):
                x = act(norm(conv(x)))
                continue
            pool, scale = 1, None
            if i == 2 and fold:
                pool = self.pooling.kernel_size
                scale = self.drop.mask(x.shape[0], x.shape[2] // pool, x.device)
            x = A.cnn_block(x, conv.conv.weight, conv.conv.bias, norm.norm.weight, norm.norm.bias, norm.eps,
                            act.negative_slope, pool, scale, dtype, self._wc, f"img_{i}", fused=fused)
        return x if fold else self.drop(self.pooling(x))


class DNN_Block(_Seq):
    def __init__(self, input_shape, neurons, activation=torch.nn.LeakyReLU, dropout=0.15):
        super().__init__()
        shape = _concrete(input_shape)
        self.add("linear", Linear(n_neurons=neurons, input_shape=shape))
        self.out_shape = shape[:-1] + (neurons,)
        self.add("norm", BatchNorm1d(input_shape=self.out_shape))
        self.add("act", activation())
        self.add("dropout", torch.nn.Dropout(p=dropout))


class CRDNN(_Seq):
    # the CNN blocks on csrc/convln.hip (one launch per conv + norm + act
    # [+ pool + dropout mask]) rather than im2col + GEMM + LayerNorm +
    # activation + torch pool.  Off by default: profiles/crdnn_ab.log has it
    # ahead in three of the four runs (and at a third of the peak memory) but
    # behind in fp32 forward + backward, and the default follows all four.
    USE_FUSED_CNN = False

    def __init__(self, input_size=None, input_shape=None, activation=torch.nn.LeakyReLU, dropout=0.15, cnn_blocks=2,
                 cnn_channels=[128, 256], cnn_kernelsize=(3, 3), time_pooling=False, time_pooling_size=2,
                 freq_pooling_size=2, rnn_class=LiGRU, inter_layer_pooling_size=[2, 2], using_2d_pooling=False,
                 rnn_layers=4, rnn_neurons=512, rnn_bidirectional=True, rnn_re_init=False, dnn_blocks=2,
                 dnn_neurons=512, projection_dim=-1, use_rnnp=False):
        super().__init__()
        if input_size is None and input_shape is None:
            raise ValueError("Must specify one of input_size or input_shape")
        if input_shape is None:
            input_shape = [None, None, input_size]
        shape = _concrete(input_shape)

        if cnn_blocks > 0:
            cnn = self.add("CNN", _Seq())
        for i in range(cnn_blocks):
            blk = cnn.add(f"block_{i}", CNN_Block(input_shape=shape, channels=cnn_channels[i],
                                                  kernel_size=cnn_kernelsize, using_2d_pool=using_2d_pooling,
                                                  pooling_size=inter_layer_pooling_size[i], activation=activation,
                                                  dropout=dropout))
            shape = blk.out_shape

        if time_pooling:
            self.add("time_pooling", Pooling1d(pool_type="max", input_dims=4, kernel_size=time_pooling_size,
                                               pool_axis=1))
            shape = (shape[0], shape[1] // time_pooling_size) + tuple(shape[2:])

        if projection_dim != -1:
            proj = self.add("projection", _Seq())
            proj.add("linear", Linear(n_neurons=projection_dim, input_shape=shape, bias=True, combine_dims=True))
            shape = (shape[0], shape[1], projection_dim)
            proj.add("norm", LayerNorm(input_shape=shape))
            proj.add("act", activation())

        if rnn_layers > 0:
            width = rnn_neurons * (2 if rnn_bidirectional else 1)
            if use_rnnp:
                # the reference's construction: an empty "RNN" container, then the
                # layers appended to the lobe itself under their position as name
                self.add("RNN", _Seq())
                for _ in range(rnn_layers):
                    self.add(str(len(self._modules)), rnn_class(hidden_size=rnn_neurons, num_layers=1,
                                                               bidirectional=rnn_bidirectional, re_init=rnn_re_init,
                                                               input_shape=shape))
                    shape = (shape[0], shape[1], width)
                    self.add(str(len(self._modules)), Linear(n_neurons=dnn_neurons, input_shape=shape, bias=True,
                                                            combine_dims=True))
                    shape = (shape[0], shape[1], dnn_neurons)
                    self.add(str(len(self._modules)), torch.nn.Dropout(p=dropout))
            else:
                self.add("RNN", rnn_class(hidden_size=rnn_neurons, num_layers=rnn_layers, dropout=dropout,
                                          bidirectional=rnn_bidirectional, re_init=rnn_re_init, input_shape=shape))
                shape = (shape[0], shape[1], width)

        if dnn_blocks > 0:
            dnn = self.add("DNN", _Seq())
        for i in range(dnn_blocks):
            blk = dnn.add(f"block_{i}", DNN_Block(input_shape=shape, neurons=dnn_neurons, activation=activation,
                                                  dropout=dropout))
            shape = blk.out_shape
        self.out_shape = shape
