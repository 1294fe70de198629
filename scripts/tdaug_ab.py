"""A/B of the time-domain augmentation drop-in: TimeDomainSpecAugment with the
recipe arguments (speeds 95 / 100 / 105, 0-3 notches, 0-5 zeroed chunks of
1000-2000 samples) on 32 x 15 s at 16 kHz, fp32.

    python scripts/tdaug_ab.py --log profiles/tdaug_ab.log [--rounds 3] [--steps 30] [--warmup 6]

Arms:
  a  the reference's algorithm in torch ops on the GPU, restated here: per
     polyphase phase a pad, a strided conv1d, a dilation by conv_transpose1d
     against an identity, a pad, a slice and an add; the notch filters chained
     by conv1d and applied by a 101-tap conv1d; a Python loop of slice
     assignments per utterance and chunk
  b  speechbrain_amd.lobes.augment.TimeDomainSpecAugment (one launch, sbk_tdaug)
  c  the same with fused = False (sbk_resample -> sbk_fir101 -> sbk_drop_chunks)

Every call of every arm starts from torch.manual_seed(call index), so the
arms make the same decisions call by call; the timed window covers all three
speeds.  The driver runs no GPU work itself.  Every timed run is a child
process of its own under `timeout`, the arms alternating a, b, c, a, ... on
one box; the first child that fails ends the driver.  A child reports the ms
per call (host clock around calls that end in a device synchronise) and the
one-read-one-write byte count of its calls, 4 (B T + B T_out) per call.  Then
one rocprofv3 --kernel-trace --stats pass (kernels only, no counters) of arms
b and c gives their kernel time per call, from which the fused launch's
share of the 8.0 TB/s HBM peak at that byte count follows.  The log records
every run, each arm's median and run-to-run spread (max - min).  Nothing here
is compared against a target: only arm against arm on one box.
"""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, T, RATE = 32, 240000, 16000
SPEEDS = [95, 100, 105]
HBM_PEAK = 8.0e12  # bytes / s, the part's specified peak


class TorchOpsArm:
    """Arm a.  Tables are made once per rate; a call draws on the host in the
    order rand, randint (speed); rand, randint, rand (notches); rand, randint
    (chunk counts), then per utterance randint lengths and randint starts."""

    def __init__(self, dev):
        import torch
        self.torch, self.dev = torch, dev
        self.tables = {}
        self.eye = torch.eye(1, device=dev).unsqueeze(2)

    def table(self, new):
        torch = self.torch
        if new not in self.tables:
            g = math.gcd(RATE, new)
            L, M = new // g, RATE // g
            cutoff = 0.99 * 0.5 * min(RATE, new)
            half = 6 / (2.0 * cutoff)
            t_out = torch.arange(0.0, L, device=self.dev) / new
            first = torch.ceil((t_out - half) * RATE)
            width = int((torch.floor((t_out + half) * RATE) - first + 1).max())
            idx = first[:, None] + torch.arange(width, device=self.dev)[None]
            dt = idx / RATE - t_out[:, None]
            w = torch.where(dt.abs() < half, 0.5 * (1 + torch.cos(2 * math.pi * cutoff / 6 * dt)), torch.zeros_like(dt))
            sinc = torch.where(dt == 0, torch.full_like(dt, 2 * cutoff),
                               torch.sin(2 * math.pi * cutoff * dt) / (math.pi * dt))
            self.tables[new] = (L, M, [int(f) for f in first.tolist()], (w * sinc / RATE))
        return self.tables[new]

    def n_out(self, new, n_in):
        ticks = RATE * new // math.gcd(RATE, new)
        span, per = n_in * (ticks // RATE), ticks // new
        last = span // per
        return last + (0 if last * per == span else 1)

    def resample(self, x, new):
        torch = self.torch
        F = torch.nn.functional
        L, M, first, w = self.table(new)
        x = x.unsqueeze(1)
        n_in, W = x.shape[-1], w.shape[1]
        total = self.n_out(new, n_in)
        y = torch.zeros(x.shape[0], 1, total, device=self.dev)
        for i in range(L):
            seg = x[..., first[i]:] if first[i] >= 0 else x
            stop = (total - 1) // L * M + W
            seg = F.pad(seg, (max(0, -first[i]), max(0, stop + 1 - (n_in - first[i]))))
            part = F.conv1d(seg, w[i].view(1, 1, -1), stride=M)
            part = F.conv_transpose1d(part, self.eye, stride=L)
            part = F.pad(part, (i, max(0, total - (i + part.shape[-1]))))
            y += part[..., :total]
        return y.squeeze(1)

    def notch(self, f, width=0.05):
        torch = self.torch
        pos = torch.arange(101) - 50

        def sinc(a):
            return torch.cat([torch.sin(a[:50]) / a[:50], torch.ones(1), torch.sin(a[51:]) / a[51:]])

        lo = sinc(3 * f * pos) * torch.blackman_window(101)
        lo = lo / lo.sum()
        hi = sinc(3 * (f + 2 * width) * pos) * torch.blackman_window(101)
        hi = hi / -hi.sum()
        hi[50] += 1
        return (lo + hi).view(1, 1, -1)

    def __call__(self, x, lens):
        torch = self.torch
        F = torch.nn.functional
        # speed
        if not torch.rand(1) > 1.0:
            new = RATE * SPEEDS[int(torch.randint(len(SPEEDS), (1,)))] // 100
            if new != RATE:
                x = self.resample(x, new)
        # notches
        y = x.clone()
        if not torch.rand(1) > 1.0:
            count = torch.randint(0, 4, (1,))
            freqs = torch.rand(count) * (1 - 1e-14) + 1e-14
            taps = torch.zeros(1, 1, 101, device=self.dev)
            taps[0, 0, 50] = 1
            for f in freqs:
                taps = F.conv1d(taps, self.notch(f).to(self.dev), padding=50)
            y = F.conv1d(y.unsqueeze(1), taps, padding=50).squeeze(1)
        # chunks
        lengths = (lens * y.shape[1]).long()
        z = y.clone()
        if not torch.rand(1) > 1.0:
            times = torch.randint(0, 6, (y.shape[0],))
            for b in range(y.shape[0]):
                if times[b] == 0:
                    continue
                ln = torch.randint(1000, 2001, (int(times[b]),))
                start = torch.randint(0, max(0, int(lengths[b]) - int(ln.max())) + 1, (int(times[b]),))
                for j in range(int(times[b])):
                    z[b, start[j]:start[j] + ln[j]] = 0.0
        return z


def child(args):
    """One arm: warm up, time `steps` calls, print one JSON line."""
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator().manual_seed(1234)
    x = (torch.rand(B, T, generator=gen) * 2 - 1).to(dev)
    lens = (0.5 + 0.5 * torch.rand(B, generator=gen)).to(dev)
    if args.arm == "a":
        m = TorchOpsArm(dev)
    else:
        from speechbrain_amd.lobes.augment import TimeDomainSpecAugment
        m = TimeDomainSpecAugment(speeds=SPEEDS)
        m.fused = args.arm == "b"
    with torch.no_grad():
        for i in range(args.warmup):
            torch.manual_seed(i)
            m(x, lens)
        torch.cuda.synchronize()
        nbytes = 0
        t0 = time.perf_counter()
        for i in range(args.steps):
            torch.manual_seed(i)
            y = m(x, lens)
            nbytes += 4 * (x.numel() + y.numel())
        torch.cuda.synchronize()
        ms = 1000.0 * (time.perf_counter() - t0) / args.steps
    print("TDAUG_AB " + json.dumps({"arm": args.arm, "ms": round(ms, 4), "mbytes": round(nbytes / args.steps / 1e6, 3),
                                    "checksum": float(y.double().abs().sum())}), flush=True)


def run_child(arm, args, log, limit=300):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--arm", arm,
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("TDAUG_AB ")), None)
    if r.returncode != 0 or line is None:
        log(f"arm {arm}: rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return None
    return json.loads(line[9:])


def trace(arm, args, log, outdir, mbytes):
    """One rocprofv3 kernel-trace pass: the arm's kernels per call, by total time."""
    d = os.path.join(outdir, f"tdaug_ab_trace_{arm}")
    os.makedirs(d, exist_ok=True)
    steps, warm = 12, 3
    cmd = ["timeout", "-k", "10", "420", "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "run",
           "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--arm", arm,
           "--steps", str(steps), "--warmup", str(warm)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        log(f"trace arm {arm}: rc={r.returncode}\n{r.stderr[-3000:]}")
        return None
    rows = list(csv.DictReader(open(files[0])))
    n = steps + warm
    ours = [x for x in rows if "tdaug" in x["Name"] or "resample" in x["Name"] or "fir101" in x["Name"]
            or "drop_chunks" in x["Name"]]
    total = sum(float(x["TotalDurationNs"]) for x in ours)
    log(f"trace arm {arm}: {sum(int(x['Calls']) for x in ours) / n:.2f} launches of the library's kernels per call, "
        f"{total / n / 1e3:.1f} us of them per call ({n} calls traced, the speeds of seeds 0..{n - 1})")
    for x in sorted(ours, key=lambda x: -float(x["TotalDurationNs"])):
        log(f"    {float(x['TotalDurationNs']) / n / 1e3:8.1f} us/call {int(x['Calls']) / n:6.2f} launches/call "
            f"{float(x['TotalDurationNs']) / max(1, int(x['Calls'])) / 1e3:8.1f} us each  {x['Name'][:80]}")
    if total > 0:
        log(f"    one read + one write is {mbytes:.1f} MB per call: {mbytes * 1e6 / (total / n * 1e-9) / 1e12:.2f} TB/s over "
            f"the kernel time, {100 * mbytes * 1e6 / (total / n * 1e-9) / HBM_PEAK:.0f} % of the {HBM_PEAK / 1e12:.1f} "
            "TB/s HBM peak (the byte count is the timed window's mean; the traced calls' speeds differ slightly)")
    return True


def driver(args):
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    fh = open(args.log, "w")

    def log(msg):
        print(msg, flush=True)
        fh.write(msg + "\n")
        fh.flush()

    log(f"tdaug_ab: TimeDomainSpecAugment(speeds={SPEEDS}) on {B} x {T} fp32 ({T / RATE:.0f} s at {RATE} Hz): torch ops "
        f"(a), the drop-in fused (b), the drop-in unfused (c); ms per call, {args.rounds} alternating rounds, "
        f"{args.steps} timed calls after {args.warmup} warm-up calls")
    res = {"a": [], "b": [], "c": []}
    for rnd in range(args.rounds):
        for arm in res:
            out = run_child(arm, args, log)
            if out is None:
                log("a run failed: stopping (nothing further is started)")
                return 1
            res[arm].append(out)
            log(f"  round {rnd} arm {arm}: {out['ms']} ms per call, {out['mbytes']} MB read once + written once per call, "
                f"checksum {out['checksum']:.6g}")
    med = {}
    for arm, runs in res.items():
        v = [r["ms"] for r in runs]
        med[arm] = statistics.median(v)
        log(f"  arm {arm}: median {med[arm]:.3f} ms per call (spread {max(v) - min(v):.3f}); one read + one write at "
            f"{HBM_PEAK / 1e12:.1f} TB/s would take {runs[0]['mbytes'] * 1e6 / HBM_PEAK * 1e3:.4f} ms: "
            f"{100 * runs[0]['mbytes'] * 1e6 / HBM_PEAK * 1e3 / med[arm]:.1f} % of it achieved end to end")
    log(f"  b / a = {med['b'] / med['a']:.3f}, c / a = {med['c'] / med['a']:.3f}, b / c = {med['b'] / med['c']:.3f}")
    if not args.no_trace:
        tmp = tempfile.mkdtemp(prefix="tdaug_ab_")
        for arm in ("b", "c"):
            if trace(arm, args, log, tmp, res[arm][0]["mbytes"]) is None:
                return 1
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("a", "b", "c"))
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "tdaug_ab.log"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--no-trace", action="store_true")
    a = ap.parse_args()
    if a.arm:
        child(a)
    else:
        sys.exit(driver(a))
