"""A/B of the LiGRU drop-in: the reference's algorithm restated in plain torch
ops on the GPU (arm a: cat([x, x.flip(1)]), Linear, BatchNorm1d / LayerNorm, a
Python loop over time; written here, eager as the reference runs without
torch.jit.script) against speechbrain_amd.nnet.RNN.LiGRU (arm b) with the same
weights and input, forward and forward + backward, under bf16 autocast and in
fp32.

    python scripts/ligru_ab.py --log profiles/ligru_ab.log [--rounds 3] [--steps 5] [--warmup 2]

Shapes:
  enc   the TIMIT CRDNN encoder RNN: 4 layers x 512, bidirectional, batchnorm, ReLU, batch 8, 300 frames,
        input 2560 (40 mels through the CRDNN's two CNN blocks: 10 bands x 256 channels)
  dec   the TIMIT transducer recipe's prediction network: 1 layer x 128, layernorm, unidirectional,
        batch 8, 60 tokens, input 39 (the one-hot width)

The driver runs no GPU work itself.  Every timed run is a child process of its
own (`--arm a|b --shape enc|dec`) under `timeout`, the arms alternating a, b,
a, b, ... on one box; the first child that fails ends the driver.  The log
records the ms per call of every run, each arm's median and run-to-run spread
(max - min).  Nothing here is compared against a target: only arm against arm
on one box.
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

SHAPES = {"enc": dict(L=4, H=512, bi=True, norm="batchnorm", I=2560, B=8, T=300),
          "dec": dict(L=1, H=128, bi=False, norm="layernorm", I=39, B=8, T=60)}
COMBOS = [("bf16", "fwd"), ("bf16", "fwdbwd"), ("fp32", "fwd"), ("fp32", "fwdbwd")]


def torch_ligru(torch, s):
    """RNN.py:961-1325 of the reference in plain torch modules, dropout 0, training mode."""
    class Layer(torch.nn.Module):
        def __init__(self, I, H, norm, bi):
            super().__init__()
            self.w = torch.nn.Linear(I, 2 * H, bias=False)
            self.u = torch.nn.Linear(H, 2 * H, bias=False)
            self.norm = torch.nn.BatchNorm1d(2 * H, momentum=0.05) if norm == "batchnorm" else torch.nn.LayerNorm(2 * H)
            self.register_buffer("h_init", torch.zeros(1, H))
            self.bi = bi

        def forward(self, x):
            if self.bi:
                x = torch.cat([x, x.flip(1)], dim=0)
            w = self.w(x)
            w = self.norm(w.reshape(w.shape[0] * w.shape[1], w.shape[2])).reshape(w.shape)
            ht, hiddens = self.h_init, []
            for k in range(w.shape[1]):
                at, zt = (w[:, k] + self.u(ht)).chunk(2, 1)
                zt = torch.sigmoid(zt)
                ht = zt * ht + (1 - zt) * torch.relu(at)
                hiddens.append(ht)
            h = torch.stack(hiddens, dim=1)
            if self.bi:
                hf, hb = h.chunk(2, dim=0)
                h = torch.cat([hf, hb.flip(1)], dim=2)
            return h

    D = 2 if s["bi"] else 1
    return torch.nn.Sequential(*[Layer(s["I"] if l == 0 else D * s["H"], s["H"], s["norm"], s["bi"])
                                 for l in range(s["L"])])


def child(args):
    """One arm at one shape: per combination warm up, time `steps` calls, print one JSON line."""
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    s = SHAPES[args.shape]
    torch.manual_seed(1234)
    stock = torch_ligru(torch, s)
    if args.arm == "b":
        from speechbrain_amd.nnet.RNN import LiGRU
        m = LiGRU(s["H"], (s["B"], s["T"], s["I"]), normalization=s["norm"], num_layers=s["L"], bidirectional=s["bi"])
        m.rnn.load_state_dict(stock.state_dict(), strict=False)      # the dropout pool stays the module's own (ones)
        m = m.to(dev)
        call = lambda x: m(x)[0]                    # noqa: E731
    else:
        m = stock.to(dev)
        call = m
    x = torch.randn(s["B"], s["T"], s["I"], device=dev, requires_grad=True)
    up = torch.randn(s["B"], s["T"], s["H"] * (2 if s["bi"] else 1), device=dev)
    out = {"arm": args.arm, "shape": args.shape}
    for prec, mode in COMBOS:
        def step():
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec == "bf16"):
                if mode == "fwd":
                    with torch.no_grad():
                        return call(x)
                y = call(x)
            y.backward(up.to(y.dtype))
            for p in m.parameters():
                p.grad = None
            x.grad = None
            return y
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        out[f"{prec}_{mode}"] = round(1000.0 * (time.perf_counter() - t0) / args.steps, 3)
    print("LIGRU_AB " + json.dumps(out), flush=True)


def run_child(arm, shape, args, log, limit=240):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--arm", arm, "--shape", shape,
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("LIGRU_AB ")), None)
    if r.returncode != 0 or line is None:
        log(f"arm {arm} {shape}: rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return None
    return json.loads(line[9:])


def driver(args):
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    fh = open(args.log, "w")

    def log(msg):
        print(msg, flush=True)
        fh.write(msg + "\n")
        fh.flush()

    log(f"ligru_ab: the reference's LiGRU restated in torch ops (a) against the LiGRU drop-in (b), ms per call, "
        f"{args.rounds} alternating rounds, {args.steps} timed calls after {args.warmup} warm-up calls per combination")
    for shape, s in SHAPES.items():
        log(f"shape {shape}: {s}")
        res = {"a": [], "b": []}
        for rnd in range(args.rounds):
            for arm in ("a", "b"):
                out = run_child(arm, shape, args, log)
                if out is None:
                    log("a run failed: stopping (nothing further is started)")
                    return 1
                res[arm].append(out)
                log(f"  round {rnd} arm {arm}: " + ", ".join(f"{p}_{m} {out[p + '_' + m]}" for p, m in COMBOS))
        for p, m in COMBOS:
            k = f"{p}_{m}"
            line = f"  {shape} {k}:"
            med = {}
            for arm in ("a", "b"):
                v = [r[k] for r in res[arm]]
                med[arm] = statistics.median(v)
                line += f" {arm} median {med[arm]:.3f} ms (spread {max(v) - min(v):.3f})"
            line += f"; b / a = {med['b'] / med['a']:.2f}"
            log(line)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("a", "b"))
    ap.add_argument("--shape", choices=tuple(SHAPES), default="enc")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "ligru_ab.log"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.arm:
        child(a)
    else:
        sys.exit(driver(a))
