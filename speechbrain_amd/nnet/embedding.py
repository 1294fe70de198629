"""Drop-in for speechbrain.nnet.embedding.Embedding (embedding.py:14-114) on HIP
(state_dict key: Embedding.weight).

One-hot mode (`consider_as_one_hot=True`, the transducer recipes' `emb`): the
frozen table is the reference's — the identity with a zero row at `blank_id` —
and forward writes the dense (..., V-1) fp32 rows with one kernel
(sbk_embed_onehot).  The returned tensor also carries the token ids and the
blank id as a private tag (`_sbk_onehot`), which speechbrain_amd.nnet.RNN.GRU
uses to gather rows of W_ih^T instead of multiplying by the one-hot matrix; any
other consumer reads the dense tensor.

Trainable mode: forward is a row gather (sbk_embed_gather); the weight
gradient is a per-id sum over a stable device sort of the ids
(sbk_segsum_rows) — no float atomics, bitwise reproducible.  Device tensors
only (SbkError otherwise, no fallback).
"""
import torch

from .._lib import check, lib, ptr, require_device, stream_of

_f32 = torch.float32


def segsum_rows(src, codes, ncodes):
    """(ncodes, D) fp32: rows of src (items, D) summed per code (codes (items,)
    integer; a code outside [0, ncodes) is dropped), in the order of a stable
    sort."""
    items, D = src.shape
    skeys, order = torch.sort(codes.reshape(-1).to(torch.int64), stable=True)
    offs = torch.searchsorted(skeys, torch.arange(ncodes + 1, device=src.device, dtype=torch.int64))
    out = torch.empty(ncodes, D, device=src.device, dtype=_f32)
    check(lib().sbk_segsum_rows(ptr(src), ptr(order), ptr(offs), items, ncodes, D, ptr(out), stream_of(src)),
          "sbk_segsum_rows")
    return out


class _GatherFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, weight):
        V, D = weight.shape
        w = weight.detach().float().contiguous()
        out = torch.empty(*ids.shape, D, device=w.device, dtype=_f32)
        check(lib().sbk_embed_gather(ptr(ids), ptr(w), ids.numel(), V, D, ptr(out), stream_of(w)), "sbk_embed_gather")
        ctx.save_for_backward(ids)
        ctx.V = V
        return out

    @staticmethod
    def backward(ctx, dy):
        (ids,) = ctx.saved_tensors
        dy2 = dy.detach().float().reshape(ids.numel(), -1).contiguous()
        return None, segsum_rows(dy2, ids, ctx.V)


class Embedding(torch.nn.Module):
    def __init__(self, num_embeddings, embedding_dim=128, consider_as_one_hot=False, blank_id=0):
        super().__init__()
        self.num_embeddings = num_embeddings
        self.consider_as_one_hot = consider_as_one_hot
        if self.consider_as_one_hot:
            self.embedding_dim = self.num_embeddings - 1
        else:
            self.embedding_dim = embedding_dim
        self.blank_id = blank_id
        if self.consider_as_one_hot:
            self.Embedding = torch.nn.Embedding(self.num_embeddings, self.embedding_dim, padding_idx=self.blank_id)
            one_hot = torch.eye(self.embedding_dim)
            if self.blank_id + 1 != self.num_embeddings:
                self.Embedding.weight.data[self.blank_id + 1:] = one_hot[self.blank_id:]
            if self.blank_id != 0:
                self.Embedding.weight.data[: self.blank_id] = one_hot[: self.blank_id]
            self.Embedding.weight.requires_grad = False
        else:
            self.Embedding = torch.nn.Embedding(self.num_embeddings, self.embedding_dim)

    def forward(self, x):
        require_device(x, self.Embedding.weight)
        if x.numel() == 0:
            raise ValueError("Embedding: empty input")
        ids = x.detach().to(torch.int32).contiguous()
        if ids.data_ptr() == x.data_ptr():
            ids = ids.clone()  # the tag must not follow a later in-place update of the caller's ids
        if not self.consider_as_one_hot:
            return _GatherFn.apply(ids, self.Embedding.weight)
        out = torch.empty(*ids.shape, self.embedding_dim, device=ids.device, dtype=_f32)
        check(lib().sbk_embed_onehot(ptr(ids), ids.numel(), self.num_embeddings, int(self.blank_id), ptr(out),
                                     stream_of(ids)), "sbk_embed_onehot")
        out._sbk_onehot = (ids, int(self.blank_id), out._version)
        return out
