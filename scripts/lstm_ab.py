"""A/B of the LSTM drop-in against the stock module: torch.nn.LSTM on the GPU
(arm a) against speechbrain_amd.nnet.RNN.LSTM (arm b) with the same weights
and input, forward and forward + backward, under bf16 autocast and in fp32.

    python scripts/lstm_ab.py --log profiles/lstm_ab.log [--rounds 3] [--steps 5] [--warmup 2]

Shapes (batch 8, 375 frames in both):
  enc   the LibriSpeech transducer recipe's encoder RNN: 4 layers x 1024, bidirectional, input 2560
  lm    RNNLM-like: 2 layers x 2048, unidirectional, input 128

The driver runs no GPU work itself.  Every timed run is a child process of its
own (`--arm a|b --shape enc|lm`) under `timeout`, the arms alternating a, b,
a, b, ... on one box; the first child that fails ends the driver.  A child
times the four (precision, pass) combinations one after the other; one the
stock module cannot run is recorded as such, not as a time.  Then one
rocprofv3 --kernel-trace --stats pass (kernels only, no counters) of arm b at
the encoder shape gives the split of its kernel time.  The log records the ms
per call of every run, each arm's median and run-to-run spread (max - min).
Nothing here is compared against a target: only arm against arm on one box.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"enc": dict(L=4, H=1024, bi=True, I=2560, B=8, T=375),
          "lm": dict(L=2, H=2048, bi=False, I=128, B=8, T=375)}
COMBOS = [("bf16", "fwd"), ("bf16", "fwdbwd"), ("fp32", "fwd"), ("fp32", "fwdbwd")]


def child(args):
    """One arm at one shape: per combination warm up, time `steps` calls, print one JSON line."""
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    s = SHAPES[args.shape]
    torch.manual_seed(1234)
    stock = torch.nn.LSTM(s["I"], s["H"], s["L"], batch_first=True, bidirectional=s["bi"])
    if args.arm == "b":
        from speechbrain_amd.nnet.RNN import LSTM
        m = LSTM(s["H"], input_size=s["I"], num_layers=s["L"], bidirectional=s["bi"])
        m.rnn.load_state_dict(stock.state_dict())
        m = m.to(dev)
        call = lambda x: m(x)[0]                    # noqa: E731
    else:
        m = stock.to(dev)
        call = lambda x: m(x)[0]                    # noqa: E731
    x = torch.randn(s["B"], s["T"], s["I"], device=dev, requires_grad=True)
    up = torch.randn(s["B"], s["T"], s["H"] * (2 if s["bi"] else 1), device=dev)
    out = {"arm": args.arm, "shape": args.shape}
    combos = [c for c in COMBOS if args.only in (None, "_".join(c))]
    for prec, mode in combos:
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
        try:
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            out[f"{prec}_{mode}"] = round(1000.0 * (time.perf_counter() - t0) / args.steps, 3)
        except (RuntimeError, NotImplementedError) as e:
            if "illegal memory access" in str(e) or "HIP error" in str(e):
                raise
            out[f"{prec}_{mode}"] = f"not run: {type(e).__name__}: {str(e)[:120]}"
    print("LSTM_AB " + json.dumps(out), flush=True)


def run_child(arm, shape, args, log, limit=300):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--arm", arm, "--shape", shape,
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("LSTM_AB ")), None)
    if r.returncode != 0 or line is None:
        log(f"arm {arm} {shape}: rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return None
    return json.loads(line[8:])


def trace(arm, shape, only, log, outdir):
    """One rocprofv3 kernel-trace pass: the kernels of one call, by total time."""
    d = os.path.join(outdir, f"lstm_ab_trace_{arm}_{shape}")
    os.makedirs(d, exist_ok=True)
    steps, warm = 1, 1
    cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run",
           "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--arm", arm, "--shape", shape,
           "--steps", str(steps), "--warmup", str(warm), "--only", only]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        log(f"trace arm {arm} {shape}: rc={r.returncode}\n{r.stderr[-3000:]}")
        return None
    rows = list(csv.DictReader(open(files[0])))
    n = steps + warm
    calls = sum(int(x["Calls"]) for x in rows)
    total = sum(float(x["TotalDurationNs"]) for x in rows)
    log(f"trace arm {arm} {shape} {only}: {calls / n:.0f} launches per call, {total / n / 1e6:.2f} ms of kernels "
        f"per call ({n} calls traced)")
    for x in sorted(rows, key=lambda x: -float(x["TotalDurationNs"]))[:12]:
        log(f"    {float(x['TotalDurationNs']) / n / 1e6:8.3f} ms/call {int(x['Calls']) / n:8.1f} launches/call "
            f"{float(x['TotalDurationNs']) / max(1, int(x['Calls'])) / 1e3:8.1f} us each  {x['Name'][:90]}")
    return True


def driver(args):
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    fh = open(args.log, "w")

    def log(msg):
        print(msg, flush=True)
        fh.write(msg + "\n")
        fh.flush()

    log(f"lstm_ab: torch.nn.LSTM (a) against the LSTM drop-in (b), ms per call, {args.rounds} alternating rounds, "
        f"{args.steps} timed calls after {args.warmup} warm-up calls per combination")
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
                if all(isinstance(t, float) for t in v):
                    med[arm] = statistics.median(v)
                    line += f" {arm} median {med[arm]:.3f} ms (spread {max(v) - min(v):.3f})"
                else:
                    line += f" {arm} {v[0]}"
            if len(med) == 2:
                line += f"; b / a = {med['b'] / med['a']:.2f}"
            log(line)
    if not args.no_trace:
        if trace("b", "enc", "bf16_fwdbwd", log, tempfile.mkdtemp(prefix="lstm_ab_")) is None:
            return 1
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("a", "b"))
    ap.add_argument("--shape", choices=tuple(SHAPES), default="enc")
    ap.add_argument("--only", default=None, help="child: one combination, e.g. bf16_fwdbwd")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "lstm_ab.log"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.arm:
        child(a)
    else:
        sys.exit(driver(a))
