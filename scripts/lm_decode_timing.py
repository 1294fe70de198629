"""Time the LM-fusion part of one S2STransformerBeamSearch step —
lm_forward_step, the score add (_add_lm_scores) and permute_lm_mem — with the
LM's key/value cache (USE_LM_KV_CACHE: TransformerLM.decode_step on
csrc/kvdec.hip's masked decode step, the tail on csrc/lmfuse.hip) against the
whole-prefix step (TransformerLM.forward on the prefix, then divide,
log-softmax, scale, add), on the same GPU in the same process.

    python scripts/lm_decode_timing.py [--beams 10,66] [--log profiles/lm_decode_time.log]

Shapes: the LM of the LibriSpeech transformer.yaml / conformer_small.yaml
recipes (12 layers, d_model 768, 12 heads, d_ffn 3072, GELU, post-norm, vocab
5000), lm_weight 0.6, temperature_lm 1.15; B 32 utterances × beam 10 (N = 320
rows) and × the recipes' beam 66 (N = 2112); prefix lengths 1, 20 and 60 (the
step that decodes position t − 1 of a t-token prefix).  Both sides are checked
against each other before timing.  Each side: 3 warm-up runs, then 20 timed
with device events, the two sides alternating repetition by repetition
(median, min, max).  The tail is also timed on its own: the fused kernel
against the four torch passes it replaces, with the (N, V) arrays each side
reads and writes counted from the code.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speechbrain_amd._kvdec import log_softmax_fuse  # noqa: E402
from speechbrain_amd.decoders.seq2seq import S2STransformerBeamSearch  # noqa: E402
from speechbrain_amd.lobes.models.transformer.TransformerLM import TransformerLM  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--beams", default="10,66")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, V, E, H, F, layers, T = 32, 5000, 768, 12, 3072, 12, 60
    w, temp = 0.6, 1.15
    torch.manual_seed(0)
    lm = TransformerLM(vocab=V, d_model=E, nhead=H, num_encoder_layers=layers, num_decoder_layers=0, d_ffn=F,
                       dropout=0.0, activation=torch.nn.GELU, normalize_before=False).to(dev).eval()
    assert lm.decode_step_supported()
    lines = [f"LM-fusion part of a beam-search step (lm_forward_step + score add + permute_lm_mem), TransformerLM "
             f"{layers} layers d_model {E} {H} heads d_ffn {F} GELU post-norm vocab {V}, lm_weight {w}, "
             f"temperature_lm {temp}, B={B}, fp32; ms per step, median of 20 [min, max], cached and whole-prefix "
             "alternating"]
    kw = dict(modules=[None, None, None], bos_index=1, eos_index=2, min_decode_ratio=0.0, max_decode_ratio=1.0,
              lm_weight=w, lm_modules=lm, temperature_lm=temp)
    for beam in (int(b) for b in args.beams.split(",")):
        N = B * beam
        whole = S2STransformerBeamSearch(beam_size=beam, **kw)
        cached = S2STransformerBeamSearch(beam_size=beam, **kw)
        cached.USE_LM_KV_CACHE = True
        gen = torch.Generator().manual_seed(beam)
        tokens = torch.randint(1, V, (N, T), generator=gen).to(dev)
        base = torch.randn(N, V, generator=gen).log_softmax(-1).to(dev)
        index = (torch.randint(0, beam, (N,), generator=gen) + torch.arange(N) // beam * beam).to(dev)
        with torch.no_grad():
            state = lm.init_decode_state(N)
            for t in (1, 20, 60):
                while state.steps < t - 1:
                    lm.decode_step(tokens[:, state.steps], state)
                prefix = tokens[:, :t - 1] if t > 1 else None
                last = tokens[:, t - 1]

                def step_cached():
                    state.steps = t - 1
                    logits, mem = cached.lm_forward_step(last, state)
                    return cached._add_lm_scores(base, logits), cached.permute_lm_mem(mem, index)

                def step_whole():
                    lp, mem = whole.lm_forward_step(last, prefix)
                    return whole._add_lm_scores(base, lp), whole.permute_lm_mem(mem, index)

                anc = state.anc.clone()
                s1, s2 = step_cached()[0], step_whole()[0]
                state.anc = anc                                     # undo the check's permute
                err = float(((s1 - s2).abs() / s2.abs().clamp(min=1.0)).max())
                assert err <= 1e-4, (beam, t, err)
                tc, tw = timed_pair(step_cached, step_whole)
                # the timed steps wrote slot t − 1 under permuted ancestries: once more under the real one
                state.anc = anc
                state.steps = t - 1
                lm.decode_step(last, state)
                lines.append(f"beam {beam} (N={N}) prefix {t}: cached {tc[0]:.3f} ms [{tc[1]:.3f}, {tc[2]:.3f}]; "
                             f"whole-prefix {tw[0]:.3f} ms [{tw[1]:.3f}, {tw[2]:.3f}]; whole / cached = "
                             f"{tw[0] / tc[0]:.1f}; scores agree to {err:.1e}")
            logits = torch.randn(N, V, generator=gen).mul(8).to(dev)

            def tail_fused():
                return log_softmax_fuse(logits, base, 1.0 / temp, w)

            def tail_torch():
                return base + w * torch.log_softmax(logits / temp, dim=-1)

            tf, tt = timed_pair(tail_fused, tail_torch)
            lines.append(f"beam {beam} (N={N}) tail alone: fused {tf[0]:.3f} ms [{tf[1]:.3f}, {tf[2]:.3f}], 1 launch, "
                         f"2 (N, V) reads + 1 write; torch divide / log_softmax / scale / add {tt[0]:.3f} ms "
                         f"[{tt[1]:.3f}, {tt[2]:.3f}], 4 launches, 5 reads + 4 writes: 6 of 9 (N, V) passes saved "
                         f"({6 * N * V * 4 / 1e6:.1f} MB per step); torch / fused = {tt[0] / tf[0]:.1f}")
            del state
    text = "\n".join(lines)
    print(text)
    if args.log:
        with open(args.log, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
