"""A/B of the ECAPA-TDNN eval forward: csrc/ecapa.hip (ECAPA_TDNN.USE_FUSED =
True, arm B) against the same modules on torch device ops (arm A), as
scripts/crdnn_ab.py measures the CRDNN.

    python scripts/ecapa_ab.py [--log profiles/ecapa_ab.log]

Shape: the recipes' model — input 80, channels [1024, 1024, 1024, 1024, 3072],
kernel sizes [5, 3, 3, 3, 1], dilations [1, 2, 3, 4, 1], N 32, L 300, ragged
lengths; eval forward under torch.no_grad(), bf16 autocast and fp32.  This
driver launches no GPU work: every timed run is a child process under
`timeout`, the arms alternate, three children per arm and run; reported are
the medians, the run-to-run spread (max - min of the three) and the peak
allocated memory.  B wins a run when A - B exceeds the sum of the spreads."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = ["bf16", "fp32"]


def child(arm, prec, steps, warmup):
    import torch
    sys.path.insert(0, ROOT)
    from speechbrain_amd.lobes.models.ECAPA_TDNN import ECAPA_TDNN
    ECAPA_TDNN.USE_FUSED = arm == "B"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = ECAPA_TDNN(80, channels=[1024, 1024, 1024, 1024, 3072], kernel_sizes=[5, 3, 3, 3, 1],
                     dilations=[1, 2, 3, 4, 1]).to(dev).eval()
    x = torch.randn(32, 300, 80, device=dev)
    lens = torch.linspace(1.0, 0.4, 32, device=dev)

    def step():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=prec == "bf16"):
            net(x, lens)

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
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "ecapa_ab.log"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(*a.child, a.steps, a.warmup)
    lines = ["ECAPA-TDNN eval forward, input 80, channels [1024 x 4, 3072], N 32, L 300, ragged lengths; A = torch "
             f"device ops, B = csrc/ecapa.hip; medians of 3 children, {a.steps} steps after {a.warmup} warm-up"]
    wins = 0
    for prec in RUNS:
        res = {"A": [], "B": []}
        for _ in range(3):
            for arm in ("A", "B"):
                cmd = ["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
                       "--warmup", str(a.warmup), "--child", arm, prec]
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:
                    print(r.stdout[-2000:], r.stderr[-2000:])
                    sys.exit(f"child {arm} {prec} ended with {r.returncode}: no further run is started")
                res[arm].append(json.loads(r.stdout.strip().splitlines()[-1]))
        med = {k: statistics.median(v["ms"] for v in res[k]) for k in res}
        spr = {k: max(v["ms"] for v in res[k]) - min(v["ms"] for v in res[k]) for k in res}
        peak = {k: max(v["peak_mb"] for v in res[k]) for k in res}
        gap = med["A"] - med["B"]
        won = gap > spr["A"] + spr["B"]
        wins += won
        lines.append(f"fwd {prec}: A {med['A']:8.3f} ms (spread {spr['A']:.3f}, peak {peak['A']:7.0f} MB)  "
                     f"B {med['B']:8.3f} ms (spread {spr['B']:.3f}, peak {peak['B']:7.0f} MB)  "
                     f"gap A - B {gap:+.3f} ms: {'B' if won else 'not B'}")
    lines.append(f"USE_FUSED default: {'on' if wins == len(RUNS) else 'off'} ({wins} of {len(RUNS)} gaps for B)")
    text = "\n".join(lines)
    print(text)
    with open(a.log, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
