"""Drop-in for speechbrain.lobes.models.ECAPA_TDNN (ECAPA_TDNN.py:18-575):
TDNNBlock, Res2NetBlock, SEBlock, AttentiveStatisticsPooling, SERes2NetBlock,
ECAPA_TDNN and Classifier, with the reference's constructors, attribute
names, construction order and state_dict keys (blocks.0.conv.conv.weight,
blocks.1.res2net_block.blocks.0.norm.norm.running_mean, asp.tdnn.*, fc.conv.*),
so its checkpoints load with strict=True.

Two forward paths, chosen per call (_fused_ok):

unfused — the reference's sequence in torch device ops on nnet.CNN.Conv1d and
nnet.normalization.BatchNorm1d, with autograd: training mode, any gradient
needed, groups != 1, weight_norm, an activation other than ReLU / LeakyReLU,
a layer or chunk width (C / res2net_scale, attention_channels) that is no
multiple of 8, pooled channels that are no multiple of 16, or
ECAPA_TDNN.USE_FUSED off.

fused — eval mode on csrc/ecapa.hip (_ecapa), time major: activations stay
(N, L, C) as the input arrives, so neither of the reference's transposes
happens.  A TDNNBlock (conv -> act -> BatchNorm on running statistics) is one
sbk_tdnn launch; a Res2Net block is one sbk_res2net launch, u_i = x_i +
y_{i-1} resident in LDS and every step reflect-padding its own input as the
reference does (chunks wider than 128 channels: one sbk_tdnn launch per
step, the sum taken as the input is staged); the SE mean comes
from the column sums of tdnn2's launch, the gate from sbk_se_gate, and
sbk_se_apply writes s * x + residual straight into the block's slot of one
(N, L, 3 C) buffer, which mfa reads with no torch.cat.  The pooling builds
neither the (N, 3C, L) concatenation nor the (N, C, L) attention: the global
context enters asp.tdnn as a per-utterance bias W_m mean + W_s std + b (one
sbk_gemm), sbk_asp_pool runs the softmax over time online; asp_bn folds into
fc (one sbk_gemm).  The sub-blocks called on their own take the same kernels
behind a transposed copy at their (N, C, L) boundary.  CPU tensors are
refused on both paths."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import _autograd as A
from ... import _ecapa as K
from ... import _enc
from ..._lib import require_device
from ...nnet.CNN import Conv1d as _Conv1d
from ...nnet.linear import Linear
from ...nnet.normalization import BatchNorm1d as _BatchNorm1d


class Conv1d(_Conv1d):
    def __init__(self, *args, **kwargs):
        super().__init__(skip_transpose=True, *args, **kwargs)


class BatchNorm1d(_BatchNorm1d):
    def __init__(self, *args, **kwargs):
        super().__init__(skip_transpose=True, *args, **kwargs)


def length_to_mask(length, max_len, device):
    """dataio.py:699-744 for the calls of this lobe."""
    mask = torch.arange(max_len, device=length.device, dtype=length.dtype).expand(len(length), max_len) \
        < length.unsqueeze(1)
    return torch.as_tensor(mask, dtype=length.dtype, device=device)


def _fused_ok(module, *tensors):
    """The fused path serves this call: flag on, eval mode, no gradient needed, every layer on the kernels' set."""
    if not ECAPA_TDNN.USE_FUSED or module.training or A.needs_grad(module, *[t for t in tensors if t is not None]):
        return False
    # the kernels read parameters as fp32: a module converted to another dtype stays on torch
    if next(module.parameters()).dtype != torch.float32:
        return False
    ok = module.__dict__.get("_fused_struct")
    if ok is None:  # the structure is fixed at construction: walked once
        ok = all(not (isinstance(m, TDNNBlock) and not m._kernel_layer())
                 and not (isinstance(m, _Conv1d) and not _kernel_conv(m))
                 and not (isinstance(m, Res2NetBlock) and m.scale < 2) for m in module.modules())
        module.__dict__["_fused_struct"] = ok
    return ok


def _kernel_conv(conv):
    k, d = conv.kernel_size, conv.dilation
    return (conv.groups == 1 and not conv.weight_norm and conv.stride == 1 and conv.padding == "same"
            and conv.padding_mode == "reflect" and k % 2 == 1 and k <= 5 and (k - 1) * d <= 32)


def _conv_args(conv, wc, dtype):
    """The sbk_tdnn arguments of a Conv1d: weight image (cached per dtype), Ci, k, d, bias."""
    cv = conv.conv
    wp = wc.get(("w", dtype), [cv.weight], lambda: K.tdnn_weight(cv.weight, dtype))
    return dict(wp=wp, Ci=cv.in_channels, k=conv.kernel_size, d=conv.dilation,
                bias=None if cv.bias is None else cv.bias.detach())


def _check_len(conv, L):
    if conv.same_pad() >= L:
        raise ValueError("Conv1d: reflect padding needs more frames than the padding")


class TDNNBlock(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, dilation, activation=nn.ReLU, groups=1):
        super().__init__()
        self.conv = Conv1d(in_channels=in_channels, out_channels=out_channels, kernel_size=kernel_size,
                           dilation=dilation, groups=groups)
        self.activation = activation()
        self.norm = BatchNorm1d(input_size=out_channels)
        self._wc = _enc.WeightCache()

    def _kernel_layer(self):
        return (type(self.activation) in (nn.ReLU, nn.LeakyReLU) and _kernel_conv(self.conv)
                and self.conv.conv.out_channels % 8 == 0 and self.norm.norm.track_running_stats)

    def _tm(self, x, dtype, **kw):
        """The layer on time-major x (N, L, Ci) in one launch."""
        _check_len(self.conv, x.shape[1])
        bn = self.norm.norm
        scale, shift = self._wc.get("aff", [bn.weight, bn.bias, bn.running_mean, bn.running_var],
                                    lambda: K.bn_affine(bn))
        args = _conv_args(self.conv, self._wc, dtype)
        args.update(kw)
        return K.tdnn(x, slope=getattr(self.activation, "negative_slope", 0.0), scale=scale, shift=shift, **args)

    def forward(self, x):
        require_device(x)
        if _fused_ok(self, x):
            dtype = _enc.compute_dtype()
            return self._tm(K.to_time_major(x, dtype), dtype).transpose(1, 2).float()
        return self.norm(self.activation(self.conv(x)))


class Res2NetBlock(torch.nn.Module):
    def __init__(self, in_channels, out_channels, scale=8, kernel_size=3, dilation=1):
        super().__init__()
        assert in_channels % scale == 0
        assert out_channels % scale == 0
        in_channel = in_channels // scale
        hidden_channel = out_channels // scale
        self.blocks = nn.ModuleList([TDNNBlock(in_channel, hidden_channel, kernel_size=kernel_size,
                                               dilation=dilation) for i in range(scale - 1)])
        self.scale = scale
        self._wc = _enc.WeightCache()

    def _images(self, dtype):
        """Step weights (scale - 1, k, w, w padded to 32), biases and folded BatchNorms (scale - 1, w) of sbk_res2net."""
        convs, bns = [b.conv.conv for b in self.blocks], [b.norm.norm for b in self.blocks]
        wp = self._wc.get(("w", dtype), [c.weight for c in convs],
                          lambda: torch.stack([K.tdnn_weight(c.weight, dtype) for c in convs]).contiguous())
        bias = None
        if convs[0].bias is not None:
            bias = self._wc.get("b", [c.bias for c in convs],
                                lambda: torch.stack([c.bias.detach().float() for c in convs]).contiguous())
        aff = self._wc.get("aff", [t for bn in bns for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var)],
                           lambda: [torch.stack(t).contiguous() for t in zip(*[K.bn_affine(bn) for bn in bns])])
        return wp, bias, aff[0], aff[1]

    def _tm(self, x, dtype):
        """The block on time-major x in one launch (sbk_res2net); a chunk wider than 128 channels or a halo past
        its LDS rows: chunk 0 copied through and one sbk_tdnn launch per step, x_i + y_{i-1} summed as it is staged."""
        w = x.shape[2] // self.scale
        cv = self.blocks[0].conv
        wo = cv.conv.out_channels
        if x.shape[2] != w * self.scale or w != wo:
            raise ValueError("Res2NetBlock: the fused path needs equal input and output chunk widths")
        if K.res2net_supported(w, self.scale, cv.kernel_size, cv.dilation):
            _check_len(cv, x.shape[1])
            return K.res2net(x, self.scale, cv.kernel_size, cv.dilation, *self._images(dtype))
        y = torch.empty_like(x)
        y[:, :, :w].copy_(x[:, :, :w])
        for i in range(1, self.scale):
            self.blocks[i - 1]._tm(x[:, :, i * w:(i + 1) * w], dtype, add=y[:, :, (i - 1) * w:i * w] if i > 1 else None,
                                   out=y[:, :, i * w:(i + 1) * w])
        return y

    def forward(self, x):
        require_device(x)
        if _fused_ok(self, x) and x.shape[1] // self.scale == self.blocks[0].conv.conv.out_channels:
            dtype = _enc.compute_dtype()
            return self._tm(K.to_time_major(x, dtype), dtype).transpose(1, 2).float()
        y = []
        for i, x_i in enumerate(torch.chunk(x, self.scale, dim=1)):
            if i == 0:
                y_i = x_i
            elif i == 1:
                y_i = self.blocks[i - 1](x_i)
            else:
                y_i = self.blocks[i - 1](x_i + y_i)
            y.append(y_i)
        return torch.cat(y, dim=1)


def _valid(lengths, N, L, device):
    """int32 valid-frame counts of a call (None: every frame)."""
    return None if lengths is None else K.valid_counts(lengths.to(device), L)


class SEBlock(nn.Module):
    def __init__(self, in_channels, se_channels, out_channels):
        super().__init__()
        self.conv1 = Conv1d(in_channels=in_channels, out_channels=se_channels, kernel_size=1)
        self.relu = torch.nn.ReLU(inplace=True)
        self.conv2 = Conv1d(in_channels=se_channels, out_channels=out_channels, kernel_size=1)
        self.sigmoid = torch.nn.Sigmoid()

    def _gate(self, part, valid, L):
        c1, c2 = self.conv1.conv, self.conv2.conv
        return K.se_gate(part, valid, L, c1.weight.detach().squeeze(-1), None if c1.bias is None else c1.bias.detach(),
                         c2.weight.detach().squeeze(-1), None if c2.bias is None else c2.bias.detach())

    def forward(self, x, lengths=None):
        require_device(x)
        L = x.shape[-1]
        if _fused_ok(self, x, lengths) and self.conv1.conv.in_channels == self.conv2.conv.out_channels:
            # standalone: the masked mean comes from sbk_asp_stats, passed to the gate as the one partial of one frame
            dtype = _enc.compute_dtype()
            xt = K.to_time_major(x, dtype)
            valid = _valid(lengths, x.shape[0], L, x.device)
            mean, _ = K.asp_stats(xt, valid)
            s = self._gate(mean.unsqueeze(1), None, 1)
            out = torch.empty_like(xt)
            K.se_apply(xt, s, None, out)
            return out.transpose(1, 2).float()
        if lengths is not None:
            mask = length_to_mask(lengths * L, max_len=L, device=x.device).unsqueeze(1)
            total = mask.sum(dim=2, keepdim=True)
            s = (x * mask).sum(dim=2, keepdim=True) / total
        else:
            s = x.mean(dim=2, keepdim=True)
        s = self.relu(self.conv1(s))
        s = self.sigmoid(self.conv2(s))
        return s * x


class AttentiveStatisticsPooling(nn.Module):
    def __init__(self, channels, attention_channels=128, global_context=True):
        super().__init__()
        self.eps = 1e-12
        self.global_context = global_context
        if global_context:
            self.tdnn = TDNNBlock(channels * 3, attention_channels, 1, 1)
        else:
            self.tdnn = TDNNBlock(channels, attention_channels, 1, 1)
        self.tanh = nn.Tanh()
        self.conv = Conv1d(in_channels=attention_channels, out_channels=channels, kernel_size=1)
        self._wc = _enc.WeightCache()

    def _tm(self, x, valid, dtype):
        """x (N, L, C) time major -> (N, 2 C) fp32 [mean | std]."""
        C = x.shape[2]
        mu, sd = K.asp_stats(x, valid)
        t, cv = self.tdnn, self.tdnn.conv.conv
        bn = t.norm.norm
        scale, shift = t._wc.get("aff", [bn.weight, bn.bias, bn.running_mean, bn.running_var], lambda: K.bn_affine(bn))
        bias = None if cv.bias is None else cv.bias.detach()
        if self.global_context:
            # W [x; mean; std] + b = W_x x + (W_m mean + W_s std + b): the bracket is a per-utterance bias
            wx = self._wc.get(("wx", dtype), [cv.weight], lambda: K.tdnn_weight(cv.weight[:, :C], dtype))
            wg = self._wc.get("wg", [cv.weight], lambda: cv.weight.detach()[:, C:, 0].float().contiguous())
            bias = _enc.gemm(torch.cat([mu, sd], 1), wg, bias=bias)
        else:
            wx = self._wc.get(("wx", dtype), [cv.weight], lambda: K.tdnn_weight(cv.weight, dtype))
        h = K.tdnn(x, wx, C, 1, 1, bias=bias, slope=getattr(t.activation, "negative_slope", 0.0), scale=scale,
                   shift=shift, tanh=True)
        cc = self.conv.conv
        wc = self._wc.get(("wc", dtype), [cc.weight], lambda: cc.weight.detach()[:, :, 0].to(dtype).contiguous())
        return K.asp_pool(h, wc, None if cc.bias is None else cc.bias.detach(), x, mu, valid)

    def forward(self, x, lengths=None):
        require_device(x)
        L = x.shape[-1]
        if _fused_ok(self, x, lengths) and x.shape[1] % 16 == 0:
            dtype = _enc.compute_dtype()
            out = self._tm(K.to_time_major(x, dtype), _valid(lengths, x.shape[0], L, x.device), dtype)
            return out.unsqueeze(2)

        def _compute_statistics(x, m, dim=2, eps=self.eps):
            mean = (m * x).sum(dim)
            std = torch.sqrt((m * (x - mean.unsqueeze(dim)).pow(2)).sum(dim).clamp(eps))
            return mean, std

        if lengths is None:
            lengths = torch.ones(x.shape[0], device=x.device)
        mask = length_to_mask(lengths * L, max_len=L, device=x.device).unsqueeze(1)
        if self.global_context:
            total = mask.sum(dim=2, keepdim=True).float()
            mean, std = _compute_statistics(x, mask / total)
            mean = mean.unsqueeze(2).repeat(1, 1, L)
            std = std.unsqueeze(2).repeat(1, 1, L)
            attn = torch.cat([x, mean, std], dim=1)
        else:
            attn = x
        attn = self.conv(self.tanh(self.tdnn(attn)))
        attn = attn.masked_fill(mask == 0, float("-inf"))
        attn = F.softmax(attn, dim=2)
        mean, std = _compute_statistics(x, attn)
        return torch.cat((mean, std), dim=1).unsqueeze(2)


class SERes2NetBlock(nn.Module):
    def __init__(self, in_channels, out_channels, res2net_scale=8, se_channels=128, kernel_size=1, dilation=1,
                 activation=torch.nn.ReLU, groups=1):
        super().__init__()
        self.out_channels = out_channels
        self.tdnn1 = TDNNBlock(in_channels, out_channels, kernel_size=1, dilation=1, activation=activation,
                               groups=groups)
        self.res2net_block = Res2NetBlock(out_channels, out_channels, res2net_scale, kernel_size, dilation)
        self.tdnn2 = TDNNBlock(out_channels, out_channels, kernel_size=1, dilation=1, activation=activation,
                               groups=groups)
        self.se_block = SEBlock(out_channels, se_channels, out_channels)
        self.shortcut = None
        if in_channels != out_channels:
            self.shortcut = Conv1d(in_channels=in_channels, out_channels=out_channels, kernel_size=1)
        self._wc = _enc.WeightCache()

    def _tm(self, x, valid, dtype, out):
        """x (N, L, Ci) time major (possibly a channel range) -> out (N, L, Co), likewise."""
        residual = x
        if self.shortcut is not None:
            residual = K.tdnn(x, slope=1.0, **_conv_args(self.shortcut, self._wc, dtype))
        h = self.res2net_block._tm(self.tdnn1._tm(x, dtype), dtype)
        h, part = self.tdnn2._tm(h, dtype, valid=valid, colsum=True)
        s = self.se_block._gate(part, valid, x.shape[1])
        return K.se_apply(h, s, residual, out)

    def forward(self, x, lengths=None):
        require_device(x)
        if _fused_ok(self, x, lengths):
            dtype = _enc.compute_dtype()
            xt = K.to_time_major(x, dtype)
            out = torch.empty(xt.shape[0], xt.shape[1], self.out_channels, device=x.device, dtype=dtype)
            self._tm(xt, _valid(lengths, x.shape[0], x.shape[-1], x.device), dtype, out)
            return out.transpose(1, 2).float()
        residual = x
        if self.shortcut:
            residual = self.shortcut(x)
        x = self.tdnn1(x)
        x = self.res2net_block(x)
        x = self.tdnn2(x)
        x = self.se_block(x, lengths)
        return x + residual


class ECAPA_TDNN(torch.nn.Module):
    # the eval forward on csrc/ecapa.hip rather than on torch device ops.  Off by
    # default: at the recipe shape profiles/ecapa_ab.log has it behind in both
    # dtypes (bf16 5.76 against 5.15 ms, fp32 12.73 against 7.72 ms), ahead
    # only in peak memory (243 against 1324 MB, 390 against 1596 MB)
    USE_FUSED = False

    def __init__(self, input_size, device="cpu", lin_neurons=192, activation=torch.nn.ReLU,
                 channels=[512, 512, 512, 512, 1536], kernel_sizes=[5, 3, 3, 3, 1], dilations=[1, 2, 3, 4, 1],
                 attention_channels=128, res2net_scale=8, se_channels=128, global_context=True,
                 groups=[1, 1, 1, 1, 1]):
        super().__init__()
        assert len(channels) == len(kernel_sizes)
        assert len(channels) == len(dilations)
        self.channels = channels
        self.blocks = nn.ModuleList()
        self.blocks.append(TDNNBlock(input_size, channels[0], kernel_sizes[0], dilations[0], activation, groups[0]))
        for i in range(1, len(channels) - 1):
            self.blocks.append(SERes2NetBlock(channels[i - 1], channels[i], res2net_scale=res2net_scale,
                                              se_channels=se_channels, kernel_size=kernel_sizes[i],
                                              dilation=dilations[i], activation=activation, groups=groups[i]))
        self.mfa = TDNNBlock(channels[-1], channels[-1], kernel_sizes[-1], dilations[-1], activation,
                             groups=groups[-1])
        self.asp = AttentiveStatisticsPooling(channels[-1], attention_channels=attention_channels,
                                              global_context=global_context)
        self.asp_bn = BatchNorm1d(input_size=channels[-1] * 2)
        self.fc = Conv1d(in_channels=channels[-1] * 2, out_channels=lin_neurons, kernel_size=1)
        self._wc = _enc.WeightCache()

    def _fc_folded(self):
        """fc(asp_bn(p)) = (W * scale) p + (W shift + b), fp32."""
        scale, shift = K.bn_affine(self.asp_bn.norm)
        w = self.fc.conv.weight.detach()[:, :, 0].float()
        b = (w * shift[None]).sum(1)  # elementwise: a matmul here would run in bf16 under autocast
        if self.fc.conv.bias is not None:
            b = b + self.fc.conv.bias.detach().float()
        return (w * scale[None]).contiguous(), b.contiguous()

    def _fused(self, x, lengths):
        dtype = _enc.compute_dtype()
        N, L, _ = x.shape
        valid = _valid(lengths, N, L, x.device)
        h = self.blocks[0]._tm(_enc.to_compute(x, dtype), dtype)
        widths = [b.out_channels for b in self.blocks[1:]]
        cat = torch.empty(N, L, sum(widths), device=x.device, dtype=dtype)
        off = 0
        for blk, w in zip(self.blocks[1:], widths):
            h = blk._tm(h, valid, dtype, cat[:, :, off:off + w])
            off += w
        h = self.mfa._tm(cat, dtype)
        pooled = self.asp._tm(h, valid, dtype)
        bn = self.asp_bn.norm
        w, b = self._wc.get("fc", [self.fc.conv.weight, self.fc.conv.bias, bn.weight, bn.bias, bn.running_mean,
                                   bn.running_var], self._fc_folded)
        return _enc.gemm(pooled, w, bias=b).unsqueeze(1)

    def forward(self, x, lengths=None):
        """x (batch, time, channel) -> (batch, 1, lin_neurons)."""
        require_device(x)
        if _fused_ok(self, x, lengths) and self.channels[-1] % 16 == 0 and len(self.blocks) > 1:
            return self._fused(x, lengths)
        x = x.transpose(1, 2)
        xl = []
        for layer in self.blocks:
            try:
                x = layer(x, lengths=lengths)
            except TypeError:
                x = layer(x)
            xl.append(x)
        x = torch.cat(xl[1:], dim=1)
        x = self.mfa(x)
        x = self.asp(x, lengths=lengths)
        x = self.asp_bn(x)
        x = self.fc(x)
        return x.transpose(1, 2)


class Classifier(torch.nn.Module):
    def __init__(self, input_size, device="cpu", lin_blocks=0, lin_neurons=192, out_neurons=1211):
        super().__init__()
        self.blocks = nn.ModuleList()
        for block_index in range(lin_blocks):
            self.blocks.extend([_BatchNorm1d(input_size=input_size), Linear(input_size=input_size,
                                                                            n_neurons=lin_neurons)])
            input_size = lin_neurons
        self.weight = nn.Parameter(torch.FloatTensor(out_neurons, input_size, device=device))
        nn.init.xavier_uniform_(self.weight)

    def forward(self, x):
        for layer in self.blocks:
            x = layer(x)
        x = F.linear(F.normalize(x.squeeze(1)), F.normalize(self.weight))
        return x.unsqueeze(1)
