"""Incremental transformer decoding on csrc/kvdec.hip: the two decode-step
attention ops and the state TransformerASR.decode_step carries between steps.

  * kv_decode_self_attn — one step of the decoder's masked self-attention.
    The key / value caches are (cap, N, E) per layer, position-major and
    append-only: the op stores the step's k / v into slot L−1 and row n reads
    position j from row anc[n][j].  A beam permutation therefore moves only
    the (N, cap) int32 ancestry table (DecodeState.permute), never the
    2 · layers · L · N · E cached floats.
  * kv_decode_cross_attn — one step of cross-attention over encoder keys /
    values projected once per search for the B utterances (not once per step
    for the N = B · group beam rows); a workgroup serves one (utterance, head)
    and reads each K / V row once for the beams of that utterance.
  * kv_decode_self_attn_masked — the self-attention step with a key mask, for
    TransformerLM.decode_step (the LM masks the keys whose token is its
    padding index); LMDecodeState carries the mask beside the caches.
  * log_softmax_fuse — base + w · log_softmax(logits · inv_t) in one kernel
    (csrc/lmfuse.hip): the tail of LM fusion in the beam search.
fp32, exact softmax; no CPU fallback.
"""
from typing import Optional

import torch

from ._lib import check, custom_op, lib, ptr, require_device, stream_of

_f32 = torch.float32

SELF_DH_MAX = 128   # csrc/kvdec.hip kDhMax
INITIAL_CAPACITY = 32


def _f32_rows(t, what):
    if t.dtype != _f32 or t.stride(-1) != 1:
        raise TypeError(f"{what} must be fp32 with contiguous rows (got {t.dtype}, strides {t.stride()})")


@custom_op("sbk::kv_decode_self_attn", mutates_args=("kc", "vc"))
def kv_decode_self_attn(qkv: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, anc: torch.Tensor, H: int,
                        L: int) -> torch.Tensor:
    """qkv (N, 3E) fp32 — the in_proj output, blocks [q | k | v]; kc, vc (cap, N, E) fp32 contiguous; anc
    (N, ≥ L) int32 with anc[:, L−1] = arange(N) → (N, E).  Slot L−1 of kc / vc receives this step's k / v."""
    require_device(qkv, kc, vc, anc)
    _f32_rows(qkv, "qkv")
    N, E3 = qkv.shape
    E = E3 // 3
    if (kc.dtype != _f32 or vc.dtype != _f32 or not kc.is_contiguous() or not vc.is_contiguous()
            or kc.shape != vc.shape or tuple(kc.shape[1:]) != (N, E) or E * 3 != E3 or E % H):
        raise ValueError(f"kv_decode_self_attn: caches {tuple(kc.shape)} / {tuple(vc.shape)} do not fit qkv "
                         f"{tuple(qkv.shape)} with {H} heads")
    if anc.dtype != torch.int32 or anc.dim() != 2 or anc.shape[0] != N or anc.stride(1) != 1:
        raise ValueError("kv_decode_self_attn: anc must be (N, ≥ L) int32 with contiguous rows")
    out = torch.empty(N, E, device=qkv.device, dtype=_f32)
    check(lib().sbk_kv_decode_self_attn(ptr(qkv[:, :E]), ptr(qkv[:, E:2 * E]), ptr(qkv[:, 2 * E:]), qkv.stride(0),
                                        ptr(kc), ptr(vc), kc.shape[0], ptr(anc), anc.stride(0), N, H, E // H, L,
                                        ptr(out), stream_of(qkv)), "sbk_kv_decode_self_attn")
    return out


@kv_decode_self_attn.register_fake
def _(qkv, kc, vc, anc, H, L):
    return qkv.new_empty(qkv.shape[0], qkv.shape[1] // 3)


@custom_op("sbk::kv_decode_cross_attn", mutates_args=())
def kv_decode_cross_attn(q: torch.Tensor, kv: torch.Tensor, klen: Optional[torch.Tensor], group: int, H: int,
                         need_probs: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """q (N, E) fp32 (row stride ≥ E); kv (B, S, 2E) fp32 contiguous — blocks [k | v], B = N / group; klen (N)
    int32 | None → (out (N, E), probs (N, H, S), or a 0-element tensor without need_probs)."""
    require_device(q, kv, klen)
    _f32_rows(q, "q")
    N, E = q.shape
    if kv.dtype != _f32 or not kv.is_contiguous() or kv.dim() != 3 or kv.shape[2] != 2 * E or E % H:
        raise ValueError(f"kv_decode_cross_attn: kv {tuple(kv.shape)} does not fit q {tuple(q.shape)}")
    B, S = kv.shape[:2]
    if group < 1 or B * group != N:
        raise ValueError(f"kv_decode_cross_attn: {N} rows are not {B} utterances x group {group}")
    if klen is not None and (klen.dtype != torch.int32 or klen.shape != (N,) or not klen.is_contiguous()):
        raise ValueError("kv_decode_cross_attn: klen must be (N) int32")
    out = torch.empty(N, E, device=q.device, dtype=_f32)
    probs = torch.empty((N, H, S) if need_probs else (0,), device=q.device, dtype=_f32)
    kv2 = kv.view(B * S, 2 * E)
    check(lib().sbk_kv_decode_cross_attn(ptr(q), q.stride(0), ptr(kv2[:, :E]), ptr(kv2[:, E:]), 2 * E, ptr(klen), N,
                                         group, H, E // H, S, ptr(out), ptr(probs) if need_probs else None,
                                         stream_of(q)), "sbk_kv_decode_cross_attn")
    return out, probs


@kv_decode_cross_attn.register_fake
def _(q, kv, klen, group, H, need_probs):
    N, E = q.shape
    return q.new_empty(N, E), q.new_empty((N, H, kv.shape[1]) if need_probs else (0,))


@custom_op("sbk::kv_decode_self_attn_masked", mutates_args=("kc", "vc"))
def kv_decode_self_attn_masked(qkv: torch.Tensor, kc: torch.Tensor, vc: torch.Tensor, anc: torch.Tensor,
                               keymask: torch.Tensor, H: int, L: int) -> torch.Tensor:
    """kv_decode_self_attn with keymask (cap, N) uint8, nonzero = masked, slot L−1 already filled: row n's key
    at j < L−1 is masked by keymask[j][anc[n][j]], its new key by keymask[L−1][n].  A (row, head) with every
    key masked gives NaN; an all-zero mask gives kv_decode_self_attn's result bit for bit."""
    require_device(qkv, kc, vc, anc, keymask)
    _f32_rows(qkv, "qkv")
    N, E3 = qkv.shape
    E = E3 // 3
    if (kc.dtype != _f32 or vc.dtype != _f32 or not kc.is_contiguous() or not vc.is_contiguous()
            or kc.shape != vc.shape or tuple(kc.shape[1:]) != (N, E) or E * 3 != E3 or E % H):
        raise ValueError(f"kv_decode_self_attn_masked: caches {tuple(kc.shape)} / {tuple(vc.shape)} do not fit qkv "
                         f"{tuple(qkv.shape)} with {H} heads")
    if anc.dtype != torch.int32 or anc.dim() != 2 or anc.shape[0] != N or anc.stride(1) != 1:
        raise ValueError("kv_decode_self_attn_masked: anc must be (N, ≥ L) int32 with contiguous rows")
    if (keymask.dtype != torch.uint8 or not keymask.is_contiguous() or keymask.dim() != 2 or keymask.shape[1] != N
            or keymask.shape[0] < L):
        raise ValueError(f"kv_decode_self_attn_masked: keymask must be (≥ {L}, {N}) uint8 contiguous "
                         f"(got {keymask.dtype}, {tuple(keymask.shape)})")
    out = torch.empty(N, E, device=qkv.device, dtype=_f32)
    # cap: the positions both the caches and the mask hold
    check(lib().sbk_kv_decode_self_attn_masked(ptr(qkv[:, :E]), ptr(qkv[:, E:2 * E]), ptr(qkv[:, 2 * E:]),
                                               qkv.stride(0), ptr(kc), ptr(vc), min(kc.shape[0], keymask.shape[0]),
                                               ptr(anc), anc.stride(0), ptr(keymask), N, H, E // H, L, ptr(out),
                                               stream_of(qkv)), "sbk_kv_decode_self_attn_masked")
    return out


@kv_decode_self_attn_masked.register_fake
def _(qkv, kc, vc, anc, keymask, H, L):
    return qkv.new_empty(qkv.shape[0], qkv.shape[1] // 3)


@custom_op("sbk::log_softmax_fuse", mutates_args=())
def log_softmax_fuse(logits: torch.Tensor, base: Optional[torch.Tensor], inv_t: float, w: float) -> torch.Tensor:
    """logits (N, V) fp32 (row stride ≥ V); base (N, V) fp32 (row stride ≥ V) | None →
    base + w · log_softmax(logits · inv_t, dim=−1) (N, V), one kernel (csrc/lmfuse.hip)."""
    require_device(logits, base)
    _f32_rows(logits, "logits")
    if logits.dim() != 2:
        raise ValueError(f"log_softmax_fuse: logits must be (N, V) (got {tuple(logits.shape)})")
    N, V = logits.shape
    if base is not None:
        _f32_rows(base, "base")
        if base.shape != logits.shape:
            raise ValueError(f"log_softmax_fuse: base {tuple(base.shape)} != logits {tuple(logits.shape)}")
    out = torch.empty(N, V, device=logits.device, dtype=_f32)
    check(lib().sbk_log_softmax_fuse(ptr(logits), logits.stride(0), ptr(base), base.stride(0) if base is not None else 0,
                                     N, V, float(inv_t), float(w), ptr(out), stream_of(logits)),
          "sbk_log_softmax_fuse")
    return out


@log_softmax_fuse.register_fake
def _(logits, base, inv_t, w):
    return logits.new_empty(logits.shape)


class DecodeState:
    """What TransformerASR.decode_step keeps between steps: per decoder layer
    the cross-attention [K | V] (B, S, 2E), computed once, and the
    self-attention caches (cap, N, E); the ancestry table anc (N, cap) int32;
    klen (N) int32 or None; the number of decoded positions `steps` (a host
    integer).  The capacity starts at INITIAL_CAPACITY positions and doubles
    by copy, so a search holds what it decoded, not max_decode_steps."""

    def __init__(self, cross_kv, klen, group, nhead):
        self.cross_kv = cross_kv
        self.klen = klen
        self.group = group
        self.nhead = nhead
        B, _, E2 = cross_kv[0].shape
        self.rows = B * group
        self.d_model = E2 // 2
        self.device = cross_kv[0].device
        self.capacity = INITIAL_CAPACITY
        self.steps = 0
        self.kc = [self._cache(self.capacity) for _ in cross_kv]
        self.vc = [self._cache(self.capacity) for _ in cross_kv]
        self.anc = torch.zeros(self.rows, self.capacity, device=self.device, dtype=torch.int32)
        self._row_ids = torch.arange(self.rows, device=self.device, dtype=torch.int32)

    def _cache(self, cap):
        return torch.empty(cap, self.rows, self.d_model, device=self.device, dtype=_f32)

    def _grow(self):
        cap = 2 * self.capacity
        for caches in (self.kc, self.vc):
            for i, old in enumerate(caches):
                new = self._cache(cap)
                new[:self.capacity] = old
                caches[i] = new
        anc = torch.zeros(self.rows, cap, device=self.device, dtype=torch.int32)
        anc[:, :self.capacity] = self.anc
        self.anc = anc
        self.capacity = cap

    def begin_step(self):
        """Make room for one more position and point it at the row itself → L, the positions attended."""
        if self.steps == self.capacity:
            self._grow()
        self.anc[:, self.steps] = self._row_ids
        return self.steps + 1

    def permute(self, index):
        """New row n continues old row index[n]: the ancestry rows move, the caches stay."""
        self.anc = self.anc.index_select(0, index)
        return self


class LMDecodeState(DecodeState):
    """What TransformerLM.decode_step keeps between steps: DecodeState without
    cross-attention — per encoder layer the self-attention caches
    (cap, N, E), the ancestry table anc (N, cap) — plus keymask (cap, N)
    uint8, 1 where the token a row fed at that position was the padding
    index.  It is indexed like the caches (position, then the row that wrote
    it), so a beam permutation moves anc only."""

    def __init__(self, rows, layers, d_model, nhead, device):
        self.cross_kv = []
        self.klen = None
        self.group = 1
        self.nhead = nhead
        self.rows = rows
        self.d_model = d_model
        self.device = device
        self.capacity = INITIAL_CAPACITY
        self.steps = 0
        self.kc = [self._cache(self.capacity) for _ in range(layers)]
        self.vc = [self._cache(self.capacity) for _ in range(layers)]
        self.anc = torch.zeros(rows, self.capacity, device=device, dtype=torch.int32)
        self.keymask = torch.zeros(self.capacity, rows, device=device, dtype=torch.uint8)
        self._row_ids = torch.arange(rows, device=device, dtype=torch.int32)

    def _grow(self):
        old = self.capacity
        super()._grow()
        keymask = torch.zeros(self.capacity, self.rows, device=self.device, dtype=torch.uint8)
        keymask[:old] = self.keymask
        self.keymask = keymask

    def begin_step(self, masked):
        """DecodeState.begin_step, and slot L−1 of keymask ← masked (N) bool."""
        L = super().begin_step()
        self.keymask[L - 1] = masked
        return L
