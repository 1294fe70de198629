"""A/B of the AttentionalRNNDecoder drop-in against the reference's algorithm
in torch ops on the GPU (arm a: a Python loop over the tokens, GRUCell +
location-aware attention step by step, nnet/RNN.py:877-958 and
nnet/attention.py:189-234 of the reference) with the same weights and inputs,
forward and forward + backward, under bf16 autocast and in fp32.

    python scripts/attdec_ab.py --log profiles/attdec_ab.log [--rounds 3] [--steps 5] [--warmup 2]

Shape: the LibriSpeech seq2seq recipe's decoder (B 8, L 375, enc_dim 512, H 1024,
attn_dim 1024, 10 channels, kernel_size 100, input 128, T 100 tokens).

The driver runs no GPU work itself.  Every timed run is a child process of its
own (`--arm a|b`) under `timeout`, the arms alternating a, b, a, b, ... on one
box; the first child that fails ends the driver.  A child times the four
(precision, pass) combinations one after the other and records
torch.cuda.max_memory_allocated of each.  The log holds the ms per call of
every run, each arm's median and run-to-run spread (max - min), and whether the
drop-in's median beats the torch arm's by more than the sum of the two spreads.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

S = dict(B=8, L=375, E=512, H=1024, A=1024, C=10, ksz=100, I=128, T=100)
COMBOS = [("bf16", "fwd"), ("bf16", "fwdbwd"), ("fp32", "fwd"), ("fp32", "fwdbwd")]


class TorchDecoder:
    """The reference's forward on the drop-in's parameters, op for op."""

    def __init__(self, m):
        import torch
        self.t, self.m, self.F = torch, m, torch.nn.functional

    def parameters(self):
        return self.m.parameters()

    def __call__(self, inp, enc, wav_len):
        t, F, m, at = self.t, self.F, self.m, self.m.attn
        cell = m.rnn.rnn_cells[0]
        L = enc.shape[1]
        enc_len = t.round(L * wav_len).long()
        pre = at.mlp_enc(enc)
        mask = (t.arange(L, device=enc.device)[None] < enc_len[:, None]).float()
        prev = mask * (1 / enc_len.float()).unsqueeze(1)
        c = t.zeros(enc.shape[0], m.attn_dim, device=enc.device)
        h = t.zeros(enc.shape[0], m.hidden_size, device=enc.device)
        outs, attns = [], []
        for i in range(inp.shape[1]):
            h = cell(m.drop(t.cat([inp[:, i], c], dim=-1)), h)
            conv = at.mlp_loc(at.conv_loc(prev.unsqueeze(1)).transpose(1, 2))
            s = at.mlp_attn(t.tanh(pre + at.mlp_dec(h.unsqueeze(1)) + conv)).squeeze(-1)
            a = F.softmax(s.masked_fill(mask == 0, float("-inf")) * at.scaling, dim=-1)
            prev = a.detach()
            c = at.mlp_out(t.bmm(a.unsqueeze(1).to(enc.dtype), enc).squeeze(1))
            outs.append(m.proj(t.cat([c, h], dim=1)))
            attns.append(a)
        return t.stack(outs, dim=1), t.stack(attns, dim=1)


def child(args):
    import torch
    from speechbrain_amd.nnet.RNN import AttentionalRNNDecoder
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234)
    m = AttentionalRNNDecoder("gru", "location", S["H"], S["A"], 1, S["E"], S["I"], channels=S["C"],
                              kernel_size=S["ksz"]).to(dev)
    call = m if args.arm == "b" else TorchDecoder(m)
    inp = torch.randn(S["B"], S["T"], S["I"], device=dev, requires_grad=True)
    enc = torch.randn(S["B"], S["L"], S["E"], device=dev, requires_grad=True)
    wav_len = torch.linspace(1.0, 0.6, S["B"], device=dev)
    up = torch.randn(S["B"], S["T"], S["H"], device=dev)
    out = {"arm": args.arm}
    for prec, mode in COMBOS:
        def step():
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec == "bf16"):
                if mode == "fwd":
                    with torch.no_grad():
                        return call(inp, enc, wav_len)[0]
                y = call(inp, enc, wav_len)[0]
            y.backward(up.to(y.dtype))
            for p in m.parameters():
                p.grad = None
            inp.grad = enc.grad = None
            return y
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        out[f"{prec}_{mode}"] = round(1000.0 * (time.perf_counter() - t0) / args.steps, 3)
        out[f"{prec}_{mode}_mib"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print("ATTDEC_AB " + json.dumps(out), flush=True)


def run_child(arm, args, log, limit=300):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--arm", arm,
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("ATTDEC_AB ")), None)
    if r.returncode != 0 or line is None:
        log(f"arm {arm}: rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return None
    return json.loads(line[10:])


def driver(args):
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    fh = open(args.log, "w")

    def log(msg):
        print(msg, flush=True)
        fh.write(msg + "\n")
        fh.flush()

    log(f"attdec_ab: the reference's loop in torch ops (a) against the drop-in (b), ms per call, {args.rounds} "
        f"alternating rounds, {args.steps} timed calls after {args.warmup} warm-up calls per combination")
    log(f"shape: {S}")
    res = {"a": [], "b": []}
    for rnd in range(args.rounds):
        for arm in ("a", "b"):
            out = run_child(arm, args, log)
            if out is None:
                log("a run failed: stopping (nothing further is started)")
                return 1
            res[arm].append(out)
            log(f"  round {rnd} arm {arm}: " + ", ".join(f"{p}_{m} {out[p + '_' + m]} ms {out[p + '_' + m + '_mib']} MiB"
                                                         for p, m in COMBOS))
    for p, m in COMBOS:
        k = f"{p}_{m}"
        med, spread = {}, {}
        for arm in ("a", "b"):
            v = [r[k] for r in res[arm]]
            med[arm], spread[arm] = statistics.median(v), max(v) - min(v)
        ok = med["a"] - med["b"] > spread["a"] + spread["b"]
        log(f"  {k}: a median {med['a']:.3f} ms (spread {spread['a']:.3f}, peak {res['a'][-1][k + '_mib']} MiB), "
            f"b median {med['b']:.3f} ms (spread {spread['b']:.3f}, peak {res['b'][-1][k + '_mib']} MiB); "
            f"a / b = {med['a'] / med['b']:.2f}; {'passes' if ok else 'DOES NOT PASS'} (gap > sum of spreads)")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("a", "b"))
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "attdec_ab.log"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.arm:
        child(a)
    else:
        sys.exit(driver(a))
