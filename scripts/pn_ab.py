"""A/B of the config-4 training step's prediction network: the stock
F.one_hot -> torch.nn.GRU of bench_train.py (arm a) against the drop-ins
speechbrain_amd Embedding(consider_as_one_hot) -> GRU (arm b) with the same
weights.  Everything else is bench_train's, by import: build_modules,
brain_class, synthetic_batch, the Brain.fit_batch step; bench_train.py itself
keeps its stock GRU.

    python scripts/pn_ab.py --log profiles/<round>_pn_ab.log [--rounds 3] [--steps 10] [--warmup 3]

The driver runs no GPU work itself.  Every timed run is a child process of its
own (`--arm a|b`) under `timeout`, the arms alternating a, b, a, b, ... on one
box; the first child that fails ends the driver.  Then one rocprofv3
--kernel-trace --stats pass per arm (kernels only, no counters) gives the
launch count per step and the time in GRU kernels.  The log records ms per
step of every run, each arm's median, arm a's run-to-run spread (max - min)
and whether b beats a by more than that spread.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def child(args):
    """One arm: warm up, time `steps` fit_batch calls, print one JSON line."""
    import torch
    import bench_train as BT
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    mods, hp = BT.build_modules()
    Base = BT.brain_class(True)
    Brain = Base
    if args.arm == "b":
        from speechbrain_amd.core import Stage
        from speechbrain_amd.nnet.RNN import GRU
        from speechbrain_amd.nnet.embedding import Embedding
        stock = mods["dec"]
        dec = GRU(BT.J, input_size=BT.V - 1)
        dec.rnn.load_state_dict(stock.state_dict())
        mods["dec"] = dec
        mods["emb"] = Embedding(BT.V, consider_as_one_hot=True, blank_id=0)

        class Brain(Base):
            def compute_forward(self, batch, stage):
                wavs, wav_lens, tokens_bos, _, _ = batch
                with torch.no_grad():
                    feats = self.hparams["compute_features"](wavs)
                    feats = self.hparams["normalize"](feats, wav_lens, epoch=0)
                    if stage == Stage.TRAIN:
                        feats = self.hparams["augmentation"](feats)
                tn = self.modules.enc_lin(self.modules.enc(self.modules.CNN(feats), wav_lens))
                h, _ = self.modules.dec(self.modules.emb(tokens_bos))
                return tn, self.modules.dec_lin(h)

    hp = {k: v.to(dev) for k, v in hp.items()}
    brain = Brain(modules=mods, opt_class=lambda p: torch.optim.Adam(p, lr=1e-4), hparams=hp,
                  run_opts={"device": str(dev), "auto_mix_prec": "bf16", "max_grad_norm": 5.0})
    for m in brain.modules.values():
        m.train()
    batch = BT.synthetic_batch(args.batch, dev, 1234)
    torch.manual_seed(1234)
    losses = [brain.fit_batch(batch) for _ in range(args.warmup)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses.append(brain.fit_batch(batch))     # as bench_train: no host read inside the window
    torch.cuda.synchronize()
    ms = 1000.0 * (time.perf_counter() - t0) / args.steps
    losses = [float(x) for x in losses]
    print("PN_AB " + json.dumps({"arm": args.arm, "ms_per_step": round(ms, 3), "steps": args.steps,
                                 "warmup": args.warmup, "loss_first_last": [round(losses[0], 4),
                                                                            round(losses[-1], 4)]}), flush=True)


def run_child(arm, args, log, limit=300):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--arm", arm,
           "--steps", str(args.steps), "--warmup", str(args.warmup), "--batch", str(args.batch)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("PN_AB ")), None)
    if r.returncode != 0 or line is None:
        log(f"arm {arm}: rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return None
    return json.loads(line[6:])


def trace(arm, args, log, outdir):
    """One rocprofv3 kernel-trace pass of an arm: (launches per step, GRU-kernel ms per step, top GRU rows)."""
    d = os.path.join(outdir, f"pn_ab_trace_{arm}")
    os.makedirs(d, exist_ok=True)
    steps, warm = 2, 2
    cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run",
           "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--arm", arm,
           "--steps", str(steps), "--warmup", str(warm), "--batch", str(args.batch)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        log(f"trace arm {arm}: rc={r.returncode}\n{r.stderr[-3000:]}")
        return None
    rows = list(csv.DictReader(open(files[0])))
    n = steps + warm
    calls = sum(int(x["Calls"]) for x in rows)
    total = sum(float(x["TotalDurationNs"]) for x in rows)
    # arm a: MIOpen's / rocBLAS's kernels have no single name; arm b: gru_*_step_kernel, segsum, embed
    mine = [x for x in rows if any(k in x["Name"] for k in ("gru_fwd_step", "gru_bwd_step", "segsum_rows",
                                                            "embed_onehot"))]
    log(f"trace arm {arm}: {calls / n:.0f} launches per step, {total / n / 1e6:.2f} ms of kernels per step "
        f"({n} steps traced)")
    for x in sorted(rows, key=lambda x: -float(x["TotalDurationNs"]))[:25]:
        log(f"    {float(x['TotalDurationNs']) / n / 1e6:8.3f} ms/step {int(x['Calls']) / n:8.1f} calls/step  "
            f"{x['Name'][:110]}")
    if mine:
        log(f"  gru.hip / embedding.hip kernels: {sum(int(x['Calls']) for x in mine) / n:.0f} launches, "
            f"{sum(float(x['TotalDurationNs']) for x in mine) / n / 1e6:.3f} ms per step")
    return {"launches_per_step": calls / n, "kernel_ms_per_step": total / n / 1e6}


def driver(args):
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    fh = open(args.log, "w")

    def log(msg):
        print(msg, flush=True)
        fh.write(msg + "\n")
        fh.flush()

    log(f"pn_ab: config-4 fit_batch, B={args.batch}, bf16 autocast, {args.rounds} alternating rounds, "
        f"{args.steps} timed steps after {args.warmup} warm-up steps per run")
    res = {"a": [], "b": []}
    for rnd in range(args.rounds):
        for arm in ("a", "b"):
            out = run_child(arm, args, log)
            if out is None:
                log("a run failed: stopping (nothing further is started)")
                return 1
            res[arm].append(out["ms_per_step"])
            log(f"round {rnd} arm {arm}: {out['ms_per_step']:.3f} ms/step, loss {out['loss_first_last']}")
    med = {k: statistics.median(v) for k, v in res.items()}
    spread = max(res["a"]) - min(res["a"])
    log(f"arm a (F.one_hot -> torch.nn.GRU):      {res['a']} median {med['a']:.3f} ms/step, spread {spread:.3f}")
    log(f"arm b (Embedding -> GRU drop-ins, HIP): {res['b']} median {med['b']:.3f} ms/step, "
        f"spread {max(res['b']) - min(res['b']):.3f}")
    gain = med["a"] - med["b"]
    log(f"b - a = {-gain:+.3f} ms/step: " + ("b is faster than a by more than a's spread" if gain > spread else
                                             "NOT faster than a by more than a's run-to-run spread"))
    if not args.no_trace:
        for arm in ("a", "b"):
            if trace(arm, args, log, os.path.dirname(os.path.abspath(args.log))) is None:
                return 1
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("a", "b"))
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "pn_ab.log"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.arm:
        child(a)
    else:
        sys.exit(driver(a))
