"""A/B of the CRDNN lobe's CNN part: the fused conv + LayerNorm + pool kernels
(csrc/convln.hip, CRDNN.USE_FUSED_CNN = True, arm B) against the same modules
on im2col + MFMA GEMM + wide LayerNorm + LeakyReLU + the pooling wrapper
(USE_FUSED_CNN = False, arm A), as scripts/ligru_ab.py measures the LiGRU.

    python scripts/crdnn_ab.py [--log profiles/crdnn_ab.log]

Shape: the recipe's CNN — B 8, T 375, 40 mel bins, channels (128, 256),
pool (2, 2), dropout 0.15.  Runs: forward (no grad) and forward + backward,
under bf16 autocast and in fp32.  This driver launches no GPU work: every
timed run is a child process under `timeout`, the arms alternate, three
children per arm and run; reported are the medians, the run-to-run spread
(max - min of the three) and the peak allocated memory.  The gap of a run
counts for B when A - B exceeds the sum of the two spreads."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = [("fwd", "bf16"), ("fwd+bwd", "bf16"), ("fwd", "fp32"), ("fwd+bwd", "fp32")]


def child(arm, mode, prec, steps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    from speechbrain_amd.lobes.models.CRDNN import CRDNN
    CRDNN.USE_FUSED_CNN = arm == "B"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = CRDNN(input_shape=(8, 375, 40), rnn_layers=0, dnn_blocks=0).to(dev)
    net.train(mode != "fwd")
    x = torch.randn(8, 375, 40, device=dev)

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec == "bf16"):
            if mode == "fwd":
                with torch.no_grad():
                    net(x)
            else:
                net.zero_grad(set_to_none=True)
                net(x).float().square().mean().backward()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    print(json.dumps({"ms": t0.elapsed_time(t1) / steps, "peak_mb": torch.cuda.max_memory_allocated() / 2 ** 20}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "crdnn_ab.log"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", nargs=3)
    a = ap.parse_args()
    if a.child:
        return child(*a.child, a.steps, a.warmup)
    lines = ["CRDNN CNN part, B 8, T 375, F 40, channels (128, 256), pool (2, 2); A = ConvBlockFn + pooling wrapper, "
             f"B = csrc/convln.hip; medians of 3 children, {a.steps} steps after {a.warmup} warm-up"]
    wins = 0
    for mode, prec in RUNS:
        res = {"A": [], "B": []}
        for _ in range(3):
            for arm in ("A", "B"):
                cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
                       "--warmup", str(a.warmup), "--child", arm, mode, prec]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:
                    print(r.stdout[-2000:], r.stderr[-2000:])
                    sys.exit(f"child {arm} {mode} {prec} ended with {r.returncode}: no further run is started")
                res[arm].append(json.loads(r.stdout.strip().splitlines()[-1]))
        med = {k: statistics.median(v["ms"] for v in res[k]) for k in res}
        spr = {k: max(v["ms"] for v in res[k]) - min(v["ms"] for v in res[k]) for k in res}
        peak = {k: max(v["peak_mb"] for v in res[k]) for k in res}
        gap = med["A"] - med["B"]
        won = gap > spr["A"] + spr["B"]
        wins += won
        lines.append(f"{mode:8s} {prec}: A {med['A']:8.3f} ms (spread {spr['A']:.3f}, peak {peak['A']:7.0f} MB)  "
                     f"B {med['B']:8.3f} ms (spread {spr['B']:.3f}, peak {peak['B']:7.0f} MB)  "
                     f"gap A - B {gap:+.3f} ms: {'B' if won else 'not B'}")
    lines.append(f"USE_FUSED_CNN default: {'on' if wins == len(RUNS) else 'off'} ({wins} of {len(RUNS)} gaps for B)")
    text = "\n".join(lines)
    print(text)
    with open(a.log, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
