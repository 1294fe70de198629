"""Time one CTC prefix-scorer step (forward_step + permute_mem) of the drop-in
against a straightforward torch-op restatement of the same step, on the same
GPU in the same process.

    python scripts/ctc_prefix_timing.py [--log profiles/ctc_prefix_time.log]

Shape: B 32, beam 10 (N = 320 rows), T 376, V 5000, prefix length 20, in
"full" mode and in "partial" mode with C = 20 candidates.  The restatement is
the textbook form: a (T, 2, N, C) forward-variable tensor filled by a loop
over the frames with logaddexp, the prefix score by logsumexp, the survivors
picked by index_select.  Each side: 3 warm-up runs, then 20 timed with device
events (one event pair per repetition; median, min, max).  Both sides are
checked against each other before timing.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechbrain_amd.decoders.ctc import CTCPrefixScorer  # noqa: E402

NEG = -1e20


def torch_step(x, r_prev, psi_prev, last_tok, cand, last_frame, beam, prefix_len, blank, eos):
    """→ (psi − psi_prev (N, V), r (T, 2, N, C), psi (N, V)) with torch ops."""
    B, T, V = x.shape
    N = B * beam
    xr = x.repeat_interleave(beam, 0)                                   # (N, T, V)
    if cand is None:
        C, xc = V, xr
        tokens = torch.arange(V, device=x.device).expand(N, V)
    else:
        C, tokens = cand.shape[1], cand
        xc = xr.gather(2, cand[:, None, :].expand(N, T, C))
    xc = xc.transpose(0, 1)                                             # (T, N, C)
    xb = xr[:, :, blank].transpose(0, 1).unsqueeze(-1)                  # (T, N, 1)
    r_sum = torch.logsumexp(r_prev, 1)                                  # (T, N)
    phi = torch.where((tokens == last_tok[:, None])[None], r_prev[:, 1, :, None], r_sum[:, :, None])
    r = torch.full((T, 2, N, C), NEG, device=x.device)
    if prefix_len == 0:
        r[0, 0] = xc[0]
    start = max(1, prefix_len)
    for t in range(start, T):
        r[t, 0] = torch.logaddexp(r[t - 1, 0], phi[t - 1]) + xc[t]
        r[t, 1] = torch.logaddexp(r[t - 1, 0], r[t - 1, 1]) + xb[t]
    psi_c = torch.logsumexp(torch.cat([phi[start - 1:T - 1] + xc[start:T], r[start - 1, 0][None]], 0), 0)
    if cand is None:
        psi = psi_c
    else:
        psi = torch.full((N, V), NEG, device=x.device).scatter_(1, cand, psi_c)
    psi[:, eos] = r_sum[last_frame.repeat_interleave(beam), torch.arange(N, device=x.device)]
    psi[:, blank] = NEG
    return psi - psi_prev[:, None], r, psi


def torch_permute(r, psi, cand, index, beam):
    T, _, N, C = r.shape
    V = psi.shape[1]
    offset = torch.arange(N // beam, device=r.device)[:, None] * beam
    parent = (index // V + offset).reshape(-1)
    token = (index % V).reshape(-1)
    if cand is None:
        col = token
    else:
        hit = cand[parent] == token[:, None]
        col = torch.where(hit.any(1), hit.float().argmax(1), 0)
    r_new = r.reshape(T, 2, N * C).index_select(2, parent * C + col).contiguous()
    return r_new, psi[parent, token]


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
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, beam, T, V, L, C = 32, 10, 376, 5000, 20, 20
    N = B * beam
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, V, generator=gen).log_softmax(-1).to(dev)
    lens = torch.randint(T // 2, T + 1, (B,), generator=gen)
    lens[0] = T
    scorer = CTCPrefixScorer(x, lens.to(dev), B, beam, 0, 2)
    prefixes = torch.randint(3, V, (N, L), generator=gen).to(dev)
    # a state of the right magnitude: forward variables of an L-token prefix
    r_prev = (-8.0 * L - 4.0 * torch.rand(T, 2, N, generator=gen)).to(dev)
    psi_prev = (-8.0 * L - torch.rand(N, generator=gen)).to(dev)
    index = torch.stack([torch.randperm(beam * V, generator=gen)[:beam] for _ in range(B)]).to(dev)
    lines = [f"CTC prefix scorer step (forward_step + permute_mem), B={B} beam={beam} T={T} V={V} prefix length {L}, "
             "fp32; ms per step, median of 20 [min, max]"]
    for mode in ("full", "partial"):
        cand = None
        if mode == "partial":
            cand = torch.stack([torch.randperm(V, generator=gen)[:C] for _ in range(N)]).to(dev)
            par = torch.randint(0, beam, (B, beam), generator=gen).to(dev)
            index = par * V + cand.view(B, beam, C)[torch.arange(B, device=dev)[:, None], par, 0]   # candidates survive

        def hip():
            out, mem = scorer.forward_step(prefixes, (r_prev, psi_prev), cand, None)
            return out, scorer.permute_mem(mem, index)

        def ref():
            out, r, psi = torch_step(scorer.x, r_prev, psi_prev, prefixes[:, -1], cand, scorer._last_frame.long(),
                                     beam, L, 0, 2)
            return out, torch_permute(r, psi, cand, index, beam)

        (o1, (r1, p1)), (o2, (r2, p2)) = hip(), ref()
        for what, a, b in (("scores", o1, o2), ("r", r1, r2), ("psi", p1[:, 0], p2)):
            err = float(((a - b).abs() / b.abs().clamp(min=1.0)).max())
            assert err <= 1e-4, (mode, what, err)
        th, tr = timed(hip), timed(ref)
        nc = V if cand is None else C
        lines.append(f"{mode}: HIP step {th[0]:.3f} ms [{th[1]:.3f}, {th[2]:.3f}]; torch-op step {tr[0]:.3f} ms "
                     f"[{tr[1]:.3f}, {tr[2]:.3f}]; torch / HIP = {tr[0] / th[0]:.1f}")
        lines.append(f"{mode}: state written per step: HIP r (T, 2, N) = {T * 2 * N * 4} bytes; "
                     f"torch-op r (T, 2, N, C={nc}) = {T * 2 * N * nc * 4} bytes")
    text = "\n".join(lines)
    print(text)
    if args.log:
        with open(args.log, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
