"""Time the wav2vec 2.0 pre-training objective (target quantiser, negatives,
contrastive loss; forward + backward) of the drop-ins against a torch-op
restatement of the reference's sequence, on the same GPU in the same process.

    python scripts/w2v_objective_timing.py [--log profiles/w2v_objective_time.log]

Shape (the LibriSpeech recipe): B 32 utterances, M 490 masked frames each,
latents 512 → 2 x 320 codes → C 256, N 100 negatives, logit temperature 0.1,
quantiser in training mode at tau 2.0, fp32.  Three paths over the same
weights, inputs, negative indices and Gumbel noise (same seed before each run):
  fused   W2VTargetQuantiser (HIP) + ContrastiveLoss on the indices of
          sample_negative_indices — negs is never built;
  float   W2VTargetQuantiser (HIP) + negs = targets[idx] gathered by torch +
          ContrastiveLoss on the float (N, B, M, C) negs — the unchanged recipe;
  torch   the reference's sequence with torch ops: weight_proj, arg-max one-hot,
          softmax mean, F.gumbel_softmax(hard=True), one-hot x codebook product,
          proj; index gather of negs, (y == negs).all, cat, cosine_similarity,
          -inf mask, transpose, cross_entropy(sum).
The negative indices are drawn once outside the timed region (the draw is the
same host code for all three).  Each path: 3 warm-up runs, then 20 timed with
device events (one pair per repetition; median, min, max) and
torch.cuda.max_memory_allocated over one further run, less what was allocated
before it.  The three losses are checked against each other before timing.
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechbrain_amd.lobes.models.wav2vec import W2VTargetQuantiser, sample_negative_indices  # noqa: E402
from speechbrain_amd.nnet.losses import ContrastiveLoss  # noqa: E402


def torch_quantiser(tq, x):
    """quantisers.py:75-123 + wav2vec.py:136-152 with torch ops."""
    q = tq.quantiser
    bsz, tsz, fsz = x.shape
    lg = F.linear(x.reshape(-1, fsz), q.weight_proj.weight, q.weight_proj.bias).view(bsz * tsz * q.groups, -1)
    k = lg.max(-1)[1]
    hard = lg.new_zeros(*lg.shape).scatter_(-1, k.view(-1, 1), 1.0).view(bsz * tsz, q.groups, -1)
    hp = torch.mean(hard.float(), dim=0)
    cp = torch.exp(-torch.sum(hp * torch.log(hp + 1e-7), dim=-1)).sum()
    ap = torch.softmax(lg.view(bsz * tsz, q.groups, -1).float(), dim=-1).mean(dim=0)
    pp = torch.exp(-torch.sum(ap * torch.log(ap + 1e-7), dim=-1)).sum()
    sel = F.gumbel_softmax(lg.float(), tau=q.curr_temp, hard=True).type_as(lg) if q.training else hard
    sel = sel.view(bsz * tsz, -1)
    o = (sel.unsqueeze(-1) * q.vars).view(bsz * tsz, q.groups, q.num_vars, -1).sum(-2).view(bsz, tsz, -1)
    nv = q.num_vars * q.groups
    return F.linear(o, tq.proj.weight, tq.proj.bias), (nv - pp) / nv, cp


def gather_negs(y, idx, N):
    B, T, C = y.shape
    return y.reshape(-1, C)[idx.view(-1)].view(B, T, N, C).permute(2, 0, 1, 3)


def torch_loss(x, y, negs, temp):
    """losses.py:1217-1251 with torch ops."""
    neg_is_pos = (y == negs).all(-1)
    cands = torch.cat([y.unsqueeze(0), negs], dim=0)
    logits = torch.cosine_similarity(x.float(), cands.float(), dim=-1).type_as(x)
    logits[1:][neg_is_pos] = float("-inf")
    logits = logits.transpose(0, 2).reshape(-1, logits.size(0))
    tg = torch.zeros(logits.size(0), dtype=torch.long, device=logits.device)
    loss = F.cross_entropy(logits / temp, tg, reduction="sum")
    return loss, torch.sum(logits.argmax(-1) == 0) / (logits.numel() / logits.size(-1))


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return statistics.median(ms), min(ms), max(ms), torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, M, D, C, N, V, temp, div_w = 32, 490, 512, 256, 100, 320, 0.1, 0.1
    torch.manual_seed(0)
    tq = W2VTargetQuantiser(D, C, num_vars=V).to(dev).train()
    crit = ContrastiveLoss(temp)
    latents = torch.randn(B, M, D, device=dev, requires_grad=True)
    emb = torch.randn(B, M, C, device=dev, requires_grad=True)
    idx = sample_negative_indices(emb, N)
    params = [latents, emb, *tq.parameters()]

    def clear():
        for p in params:
            p.grad = None

    def objective(path):
        torch.manual_seed(1)  # the same Gumbel noise on every path
        clear()
        if path == "torch":
            y, div, _ = torch_quantiser(tq, latents)
            loss, acc = torch_loss(emb, y, gather_negs(y, idx, N), temp)
        else:
            y, meta = tq(latents)
            div = meta["diversity_loss"]
            loss, acc = crit(emb, y, idx if path == "fused" else gather_negs(y, idx, N))
        total = loss + div * div_w * (B * M)
        total.backward()
        return total.detach(), acc.detach()

    y_fix = tq(latents)[0].detach().requires_grad_()

    def loss_only(path):
        emb.grad = y_fix.grad = None
        if path == "torch":
            loss, _ = torch_loss(emb, y_fix, gather_negs(y_fix, idx, N), temp)
        else:
            loss, _ = crit(emb, y_fix, idx if path == "fused" else gather_negs(y_fix, idx, N))
        loss.backward()
        return loss.detach()

    def close(a, b):
        return (a - b).abs() <= 1e-4 * b.abs().clamp(min=1.0)

    # loss alone, on the same targets: values and gradients must agree
    chk = {}
    for path in ("fused", "float", "torch"):
        chk[path] = (loss_only(path), emb.grad.clone(), y_fix.grad.clone())
    for path in ("float", "torch"):
        for what, a, b in zip(("loss", "d emb", "d targets"), chk["fused"], chk[path]):
            assert bool(close(a, b).all()), (path, what, float((a - b).abs().max()))
    # whole objective: the HIP and the torch projection round differently, so among
    # the 31,360 (frame, group) arg-maxes over noised logits a near-tie can fall the
    # other way and move that frame's target; the objective and the accuracy must
    # agree, and all but a few frames' gradients
    chk = {}
    for path in ("fused", "float", "torch"):
        total, acc = objective(path)
        chk[path] = (total, acc, emb.grad.clone(), latents.grad.clone())
    rows_off = {}
    for path in ("float", "torch"):
        for what, a, b in zip(("objective", "accuracy"), chk["fused"], chk[path]):
            assert bool(close(a, b).all()), (path, what, float(a), float(b))
        off = sum(int((~close(a, b).all(-1)).sum()) for a, b in zip(chk["fused"][2:], chk[path][2:]))
        assert off <= 2 * B * M // 1000, (path, off)
        rows_off[path] = off
    lines = [f"wav2vec 2.0 objective, forward + backward: B={B} M={M} latents={D} codes=2x{V} C={C} N={N} "
             f"logit_temp={temp} tau=2.0 (training), fp32; ms, median of 20 [min, max]; peak = "
             "torch.cuda.max_memory_allocated over one run less the bytes allocated before it"]
    res = {}
    for name, fn in (("quantiser + negatives + loss", objective), ("negatives + loss only", loss_only)):
        for path in ("fused", "float", "torch"):
            res[name, path] = t = timed(lambda: fn(path))
            lines.append(f"{name}: {path:5s} {t[0]:.3f} ms [{t[1]:.3f}, {t[2]:.3f}]; peak {t[3] / 2**20:.1f} MiB")
        f, fl, to = (res[name, p] for p in ("fused", "float", "torch"))
        lines.append(f"{name}: torch / fused = {to[0] / f[0]:.2f} (time), {to[3] / max(f[3], 1):.1f} (peak memory); "
                     f"torch / float = {to[0] / fl[0]:.2f} (time), {to[3] / max(fl[3], 1):.1f} (peak memory)")
    lines.append(f"check before timing: loss, d emb, d targets of the three paths agree to 1e-4 on the same targets; "
                 f"whole objective and accuracy agree to 1e-4; gradient rows (of {2 * B * M}) outside 1e-4 against "
                 f"fused: float {rows_off['float']}, torch {rows_off['torch']}")
    text = "\n".join(lines)
    print(text)
    if args.log:
        with open(args.log, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
