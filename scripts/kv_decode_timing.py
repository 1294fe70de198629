"""Time one decoder step of S2STransformerBeamSearch (forward_step +
permute_mem) with the key/value cache (USE_KV_CACHE, TransformerASR.decode_step
on csrc/kvdec.hip) against the whole-prefix step (TransformerASR.decode), on
the same GPU in the same process.

    python scripts/kv_decode_timing.py [--log profiles/kv_decode_time.log]

Shapes: B 32, beam 10 (N = 320 rows), S 376 encoder frames, 6 decoder layers,
vocabulary 5000, d_ffn 2048, at d_model 256 / 4 heads and d_model 512 / 8 heads
(the reference's transformer.yaml decoder, head size 64); prefix lengths 1, 20
and 40 (the step that decodes position t − 1 of a t-token prefix).  Both
sides are checked against each other before timing.  Each side: 3 warm-up
runs, then 20 timed with device events, the two sides alternating repetition
by repetition (median, min, max).  FLOPs and bytes per step are arithmetic
from the shapes, not measurements.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechbrain_amd.decoders.seq2seq import S2STransformerBeamSearch  # noqa: E402
from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR  # noqa: E402
from speechbrain_amd.nnet.linear import Linear  # noqa: E402


def timed_pair(fa, fb, reps=20, warm=3):
    """fa and fb alternating → ((median, min, max) of fa, of fb) in ms."""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(reps):
        for fn, acc in zip((fa, fb), ms):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b))
    return tuple((statistics.median(m), min(m), max(m)) for m in ms)


def step_cost(N, B, t, S, E, F, V, layers, cached):
    """(FLOPs, bytes) of one step from the shapes.  FLOPs: 2 per multiply-add
    of every GEMM and attention product.  Bytes: fp32 weights read once, plus
    the streams that grow with the batch — encoder states and cross K / V,
    the self-attention keys / values, the vocabulary logits."""
    P = N * (1 if cached else t)          # positions run through the layers
    per_layer = (2 * P * E * 3 * E        # self in_proj
                 + 2 * P * E * E          # self out_proj
                 + 2 * P * E * E          # cross q
                 + 2 * P * E * E          # cross out_proj
                 + 4 * P * E * F)         # FFN
    weights = layers * (8 * E * E + 2 * E * F) * 4 + E * V * 4
    if cached:
        per_layer += 4 * N * t * E + 4 * N * S * E                  # q·K and P·V over the cache / the encoder keys
        stream = layers * (2 * N * t * E * 4                        # cached self K / V read (per beam row)
                           + 2 * B * S * E * 4)                     # cross K / V read once per utterance
        stream += N * t * 4 * 2                                     # the ancestry table's index_select
    else:
        per_layer += 4 * N * t * t * E + 4 * N * t * S * E          # the whole (t, t) and (t, S) maps
        per_layer += 4 * N * S * E * E                              # cross K and V projections of the N inflated rows
        stream = layers * (2 * N * S * E * 4                        # encoder states read by the K and V GEMMs
                           + 2 * 2 * N * S * E * 4)                 # cross K / V written, then read
    flops = layers * per_layer + 2 * P * E * V
    return flops, weights + stream + P * V * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, beam, S, layers, V, F = 32, 10, 376, 6, 5000, 2048
    N = B * beam
    lines = [f"Transformer beam-search decoder step (forward_step + permute_mem), B={B} beam={beam} (N={N}) S={S} "
             f"{layers} decoder layers, vocab {V}, d_ffn {F}, fp32; ms per step, median of 20 [min, max], cached and "
             "whole-prefix alternating"]
    for E, H in ((256, 4), (512, 8)):
        torch.manual_seed(0)
        tr = TransformerASR(tgt_vocab=V, input_size=80, d_model=E, nhead=H, num_encoder_layers=0,
                            num_decoder_layers=layers, d_ffn=F, dropout=0.0, activation=torch.nn.GELU,
                            normalize_before=True).to(dev).eval()
        modules = [tr, Linear(input_size=E, n_neurons=V).to(dev).eval(), Linear(input_size=E, n_neurons=V).to(dev).eval()]
        kw = dict(bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0, beam_size=beam)
        whole = S2STransformerBeamSearch(modules=modules, **kw)
        cached = S2STransformerBeamSearch(modules=modules, **kw)
        cached.USE_KV_CACHE = True
        gen = torch.Generator().manual_seed(1)
        enc = torch.randn(B, S, E, generator=gen).to(dev)
        enc_inf = enc.repeat_interleave(beam, 0)
        tokens = torch.randint(3, V, (N, 40), generator=gen).to(dev)
        index = (torch.randint(0, beam, (N,), generator=gen) + torch.arange(N) // beam * beam).to(dev)
        with torch.no_grad():
            for t in (1, 20, 40):
                state = tr.init_decode_state(enc, group=beam)
                for j in range(t - 1):
                    tr.decode_step(tokens[:, j], state)
                prefix = tokens[:, :t - 1] if t > 1 else None
                last = tokens[:, t - 1]

                def step_cached():
                    state.steps = t - 1
                    lp, mem, attn = cached.forward_step(last, state, enc_inf, None)
                    return lp, attn, cached.permute_mem(mem, index)

                def step_whole():
                    lp, mem, attn = whole.forward_step(last, prefix, enc_inf, None)
                    return lp, attn[:, -1:], whole.permute_mem(mem, index)

                (lp1, at1, _), (lp2, at2, _) = step_cached(), step_whole()
                state.anc[:, :t] = torch.arange(N, device=dev, dtype=torch.int32)[:, None]   # undo the check's permute
                for what, a, b in (("log-probs", lp1, lp2), ("attn", at1, at2)):
                    err = float(((a - b).abs() / b.abs().clamp(min=1.0)).max())
                    assert err <= 1e-4, (E, t, what, err)
                tc, tw = timed_pair(step_cached, step_whole)
                fc, bc = step_cost(N, B, t, S, E, F, V, layers, True)
                fw, bw = step_cost(N, B, t, S, E, F, V, layers, False)
                lines.append(f"E={E} H={H} prefix {t}: cached {tc[0]:.3f} ms [{tc[1]:.3f}, {tc[2]:.3f}]; whole-prefix "
                             f"{tw[0]:.3f} ms [{tw[1]:.3f}, {tw[2]:.3f}]; whole / cached = {tw[0] / tc[0]:.1f}")
                lines.append(f"E={E} H={H} prefix {t}: from the shapes, per step: cached {fc / 1e9:.2f} GFLOP, "
                             f"{bc / 1e6:.1f} MB; whole-prefix {fw / 1e9:.2f} GFLOP, {bw / 1e6:.1f} MB")
        once = layers * 4 * B * S * E * E
        lines.append(f"E={E} H={H}: cached path, once per search: cross K / V projections {once / 1e9:.2f} GFLOP, "
                     f"{layers * 2 * B * S * E * 4 / 1e6:.1f} MB kept")
    text = "\n".join(lines)
    print(text)
    if args.log:
        with open(args.log, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
