"""Time the CTC loss at the CTC/attention recipe's shape (B = 32, T = 376,
V = 5000, L <= 120): forward + backward of

  a  ctc_loss_from_logits (log-softmax fused into the loss)
  b  torch log_softmax, then ctc_loss on the log-probs
  c  torch's own on-device log_softmax + torch.nn.functional.ctc_loss

    python scripts/time_ctc.py [--out profiles/ctc_time.log]

Every variant runs in a process of its own (a failure of one cannot hide the
others), on the same seeded inputs.  Times are device events around a window
of >= 0.5 s of back-to-back iterations after warm-up, five windows, median
and range.  A further child runs variant a under `rocprofv3 --kernel-trace
--stats` and reads the mean time of each kernel; the gather and gradient
passes are set against the copy ceiling for their bytes, i.e. the bandwidth a
device-to-device copy of the (B, T, V) tensor reaches in the same process.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, T, V, L = 32, 376, 5000, 120


def inputs(dev):
    import torch
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, V, generator=g).to(dev)
    targets = torch.randint(1, V, (B, L), generator=g).to(dev)
    il = torch.randint(300, T + 1, (B,), generator=g)
    tl = torch.randint(60, L + 1, (B,), generator=g)
    il[0], tl[0] = T, L
    return x, targets, il, tl


def windows(step, n_windows=5):
    import torch
    for _ in range(10):
        step()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def run(n):
        ev[0].record()
        for _ in range(n):
            step()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / n   # ms per iteration

    n = max(20, int(500.0 / run(20)) + 1)
    ts = sorted(run(n) for _ in range(n_windows))
    return {"ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "iters_per_window": n}


def one(variant, iters):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_ctc.py needs a ROCm GPU; nothing is measured without one")
    from speechbrain_amd.nnet.losses import ctc_loss, ctc_loss_from_logits
    dev = torch.device("cuda:0")
    x, targets, il, tl = inputs(dev)
    x.requires_grad_()
    ilr, tlr = (il / T).float().to(dev), (tl / L).float().to(dev)
    il_d, tl_d = il.to(dev), tl.to(dev)

    def step():
        x.grad = None
        if variant == "a":
            loss = ctc_loss_from_logits(x, targets, ilr, tlr, 0, reduction="sum")
        elif variant == "b":
            loss = ctc_loss(x.log_softmax(-1), targets, ilr, tlr, 0, reduction="sum")
        else:
            loss = torch.nn.functional.ctc_loss(x.log_softmax(-1).transpose(0, 1), targets, il_d, tl_d, 0,
                                                reduction="sum", zero_infinity=True)
        loss.backward()
        return loss

    if iters:   # traced run: a fixed, small number of iterations
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        return
    res = {"variant": variant, "loss": float(step())}
    res.update(windows(step))
    if variant == "a":
        y = torch.empty_like(x)
        with torch.no_grad():
            cp = windows(lambda: y.copy_(x))
        res["copy_ms"] = cp["ms"]
        res["copy_GBps"] = 2 * x.numel() * 4 / cp["ms"] / 1e6
    print("RESULT " + json.dumps(res), flush=True)


def child(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), *args], capture_output=True, text=True,
                       timeout=timeout, cwd=ROOT)
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:]), r
    return None, r


def kernel_times():
    """Mean device time (µs) of each ctc kernel of variant a, from a traced run
    of its own."""
    tool = "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return None, "rocprofv3 not found"
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([tool, "--kernel-trace", "--stats", "-d", d, "-o", "ctc", "--output-format", "csv", "--",
                            sys.executable, os.path.abspath(__file__), "--one", "a", "--iters", "30"],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        out = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                name = row.get("Name", "")
                if "ctc_" in name and row.get("AverageNs"):
                    key = name.split("ctc_")[1].split("_kernel")[0]
                    out[key] = {"us": float(row["AverageNs"]) / 1e3, "calls": int(float(row.get("Calls", 0)))}
        if not out:
            return None, f"no kernel statistics (rc {r.returncode}): {r.stderr[-300:]}"
        return out, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=["a", "b", "c"])
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.iters)
    lines = [f"CTC forward + backward, B={B} T={T} V={V} L<={L}, fp32; ms per iteration, median of 5 windows [min, max]"]
    res = {}
    for v, what in (("a", "ctc_loss_from_logits"), ("b", "torch log_softmax + ctc_loss"),
                    ("c", "torch log_softmax + torch ctc_loss (device)")):
        res[v], r = child(["--one", v])
        if res[v] is None:
            lines.append(f"({v}) {what}: FAILED rc {r.returncode}: {r.stderr.strip()[-400:]}")
            if r.returncode not in (0, 1):
                # killed, aborted or faulted: start nothing more on the device
                lines.append("stopped: no further process is started after an abnormal exit")
                res = {}
                break
        else:
            m = res[v]
            lines.append(f"({v}) {what}: {m['ms']:.3f} ms [{m['min_ms']:.3f}, {m['max_ms']:.3f}], "
                         f"{m['iters_per_window']} iterations per window, loss {m['loss']:.3f}")
    if res.get("a") and res.get("c"):
        lines.append(f"(c) / (a) = {res['c']['ms'] / res['a']['ms']:.2f}")
    if res.get("a"):
        bw = res["a"]["copy_GBps"]
        lines.append(f"copy ceiling: device copy of the (B, T, V) tensor {res['a']['copy_ms']:.3f} ms = {bw:.0f} GB/s "
                     "(read + write)")
        kt, err = kernel_times()
        if kt is None:
            lines.append(f"kernel times: not measured ({err})")
        else:
            n = B * T * V * 4
            # gather: the logits read once (the second sweep of a 20 kB row is served by the cache);
            # gradient: logits read, gradient written
            for key, nbytes in (("gather", n), ("grad", 2 * n)):
                if key in kt:
                    floor_us = nbytes / bw / 1e3
                    lines.append(f"{key} kernel: {kt[key]['us']:.1f} us mean of {kt[key]['calls']} calls, "
                                 f"{nbytes / 1e6:.0f} MB, copy-ceiling time {floor_us:.1f} us, "
                                 f"fraction of ceiling {floor_us / kt[key]['us']:.2f}")
            if "lattice" in kt:
                lines.append(f"lattice kernel: {kt['lattice']['us']:.1f} us mean of {kt['lattice']['calls']} calls "
                             f"({2 * B} workgroups, {T} dependent steps)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
