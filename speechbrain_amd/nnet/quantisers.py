"""Drop-in for speechbrain.nnet.quantisers.GumbelVectorQuantizer
(quantisers.py:13-123) on HIP.

The projection runs on the MFMA GEMM in the compute dtype; everything after
the logits is one fp32 kernel (csrc/w2vloss.hip): arg-max, hard-code counts,
softmax column sums, the chosen code, in training the Gumbel softmax, and the
output written as the selected `vars` rows — no one-hot tensor, no
(B·T, G·V, D) product.  The two perplexities are device-side torch on the
(G, V) sums.  The Gumbel noise is drawn as F.gumbel_softmax draws it
(`-torch.empty_like(logits).exponential_().log()` from torch's generator of
the logits' device) and handed to the kernel.  Backward: straight-through to
the logits (training), the gradient of prob_perplex through the softmax
sums, and dvars as a deterministic per-code sum.  Device tensors only
(SbkError otherwise)."""
import torch
import torch.nn as nn

from .. import _autograd as A
from .. import _enc
from .. import _w2v
from .._lib import OPS, require_device


class GumbelVectorQuantizer(nn.Module):
    def __init__(self, input_dim, num_vars, temp_tuple, groups, vq_dim):
        super().__init__()
        self.groups = groups
        self.input_dim = input_dim
        self.num_vars = num_vars
        self.vq_dim = vq_dim
        assert (
            vq_dim % groups == 0
        ), f"dim {vq_dim} must be divisible by groups {groups} for concatenation"
        var_dim = vq_dim // groups
        self.vars = nn.Parameter(torch.FloatTensor(1, groups * num_vars, var_dim))
        nn.init.uniform_(self.vars)
        self.weight_proj = nn.Linear(self.input_dim, groups * num_vars)
        nn.init.normal_(self.weight_proj.weight, mean=0, std=1)
        nn.init.zeros_(self.weight_proj.bias)
        assert len(temp_tuple) == 3, temp_tuple
        self.max_temp, self.min_temp, self.temp_decay = temp_tuple
        self.curr_temp = self.max_temp
        self.max_ent = nn.Parameter(torch.log(torch.tensor(float(self.num_vars * self.groups))), requires_grad=False)
        self._wc = _enc.WeightCache()

    def update_temp(self, steps):
        """ Update the temperature given the current step """
        self.curr_temp = max(self.max_temp * self.temp_decay ** steps, self.min_temp)

    def quantise(self, logits, gumbels=None):
        """Everything after the projection, on logits (B·T·G, V) fp32:
        (quantised (B·T, vq_dim), code_perplexity, prob_perplex).  gumbels:
        the noise of the training-mode Gumbel softmax (same shape), None for
        the eval-mode arg-max."""
        require_device(logits, gumbels, self.vars)
        logits = logits.float().contiguous()
        gumbels = None if gumbels is None else gumbels.float().contiguous()
        out, _, counts, psum, _ = OPS.gumbel_vq(logits, gumbels, self.vars.view(self.groups * self.num_vars, -1),
                                                float(self.curr_temp), self.groups)
        rows = logits.shape[0] // self.groups
        hard_probs = counts.view(self.groups, -1).float() / rows
        code_perplexity = torch.exp(-torch.sum(hard_probs * torch.log(hard_probs + 1e-7), dim=-1)).sum()
        avg_probs = psum.view(self.groups, -1) / rows
        prob_perplex = torch.exp(-torch.sum(avg_probs * torch.log(avg_probs + 1e-7), dim=-1)).sum()
        return out, code_perplexity, prob_perplex

    def forward(self, x):
        """(B, T, input_dim) → {"x": (B, T, vq_dim), "code_perplexity",
        "prob_perplex", "num_vars", "temp"} (quantisers.py:75-123)."""
        require_device(x, self.vars)
        result = {"num_vars": self.num_vars * self.groups, "temp": self.curr_temp}
        bsz, tsz, fsz = x.shape
        lin = self.weight_proj
        logits = A.linear(x.reshape(-1, fsz), lin.weight, lin.bias, _enc.compute_dtype(), self._wc, "vq_proj")
        logits = logits.view(bsz * tsz * self.groups, -1)
        gumbels = None
        if self.training:
            # F.gumbel_softmax's draw, on the logits' device
            gumbels = -torch.empty_like(logits, memory_format=torch.legacy_contiguous_format).exponential_().log()
        out, result["code_perplexity"], result["prob_perplex"] = self.quantise(logits, gumbels)
        result["x"] = out.view(bsz, tsz, -1)
        return result
