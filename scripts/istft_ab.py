"""A/B of the ISTFT drop-in and the STFT gradient on 32 x 15 s at 16 kHz, fp32,
at (n_fft 400, hop 160) and (n_fft 512, hop 128), Hamming window, centred.

    python scripts/istft_ab.py --log profiles/istft_ab.log [--rounds 3] [--steps 20] [--warmup 5]

Arms:
  a  the reference's own sequence on the device: ISTFT.forward is permute ->
     torch.complex -> torch.istft, STFT.forward is torch.stft ->
     view_as_real -> transpose, gradients by autograd
  b  speechbrain_amd.processing.features.ISTFT / STFT (sbk_istft,
     sbk_istft_bwd, sbk_spectrum)

Cases: ISTFT forward, ISTFT forward + backward (gradient of the spectrum),
STFT forward + backward (gradient of the waveform).  The driver runs no GPU
work itself.  Every timed run is a child process of its own under `timeout`,
the arms alternating a, b, a, ... on one box; the first child that fails ends
the driver.  A child reports the ms per call of each case (host clock around
calls that end in a device synchronise).  The log records every run, each
arm's median and run-to-run spread (max - min), and for arm b's ISTFT forward
(one launch) the bytes it must move (spectrum read + waveform written) over
the call time as a share of the 8.0 TB/s HBM peak: an end-to-end figure, the
launch included, not a kernel trace.  Nothing here is compared against a
target: only arm against arm on one box.
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

B, S, RATE = 32, 240000, 16000
SETTINGS = {"400_160": (400, 25, 10, 160), "512_128": (512, 32, 8, 128)}  # n_fft, win ms, hop ms, hop
CASES = ("istft_fwd", "istft_fwdbwd", "stft_fwdbwd")
HBM_PEAK = 8.0e12  # bytes / s, the part's specified peak


def child(args):
    """One arm: per setting and case warm up, time `steps` calls; one JSON line."""
    import torch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    gen = torch.Generator().manual_seed(1234)
    wav = (torch.rand(B, S, generator=gen) * 2 - 1).to(dev)
    out = {}
    for name, (n_fft, win_ms, hop_ms, hop) in SETTINGS.items():
        window = torch.hamming_window(n_fft).to(dev)
        if args.arm == "a":
            def stft(x):
                return torch.view_as_real(torch.stft(x, n_fft, hop, n_fft, window, True, "constant", False, True,
                                                     return_complex=True)).transpose(2, 1)

            def istft(x):
                x = x.permute(0, 2, 1, 3)
                return torch.istft(torch.complex(x[..., 0], x[..., 1]), n_fft=n_fft, hop_length=hop, win_length=n_fft,
                                   window=window, center=True, onesided=True, length=S)
        else:
            from speechbrain_amd.processing.features import ISTFT, STFT
            stft = STFT(RATE, win_length=win_ms, hop_length=hop_ms, n_fft=n_fft)
            inv = ISTFT(RATE, n_fft=n_fft, win_length=win_ms, hop_length=hop_ms)

            def istft(x):
                return inv(x, S)
        with torch.no_grad():
            spec = stft(wav).contiguous()
        dy = torch.randn(B, S, generator=gen).to(dev)
        dspec = torch.randn(spec.shape, generator=gen).to(dev)

        def istft_fwd():
            with torch.no_grad():
                return istft(spec)

        def istft_fwdbwd():
            x = spec.detach().requires_grad_()
            istft(x).backward(dy)
            return x.grad

        def stft_fwdbwd():
            x = wav.detach().requires_grad_()
            stft(x).backward(dspec)
            return x.grad

        for case, fn in zip(CASES, (istft_fwd, istft_fwdbwd, stft_fwdbwd)):
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                r = fn()
            torch.cuda.synchronize()
            out[f"{name}_{case}"] = round(1000.0 * (time.perf_counter() - t0) / args.steps, 4)
            out[f"{name}_{case}_sum"] = float(r.double().abs().sum())
        out[f"{name}_mbytes"] = round(4 * (spec.numel() + B * S) / 1e6, 3)
    print("ISTFT_AB " + json.dumps({"arm": args.arm, **out}), flush=True)


def run_child(arm, args, log, limit=300):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--arm", arm,
           "--steps", str(args.steps), "--warmup", str(args.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("ISTFT_AB ")), None)
    if r.returncode != 0 or line is None:
        log(f"arm {arm}: rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
        return None
    return json.loads(line[9:])


def driver(args):
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    fh = open(args.log, "w")

    def log(msg):
        print(msg, flush=True)
        fh.write(msg + "\n")
        fh.flush()

    log(f"istft_ab: torch.istft / torch.stft with autograd on the device (a) against the ISTFT / STFT drop-ins (b) on "
        f"{B} x {S} fp32 ({S / RATE:.0f} s at {RATE} Hz); ms per call, {args.rounds} alternating rounds, {args.steps} "
        f"timed calls after {args.warmup} warm-up calls per case")
    res = {"a": [], "b": []}
    for rnd in range(args.rounds):
        for arm in res:
            out = run_child(arm, args, log)
            if out is None:
                log("a run failed: stopping (nothing further is started)")
                return 1
            res[arm].append(out)
            log(f"  round {rnd} arm {arm}: " + ", ".join(f"{k} {v}" for k, v in out.items()
                                                          if k != "arm" and not k.endswith(("_sum", "_mbytes"))))
    for name in SETTINGS:
        for case in CASES:
            k = f"{name}_{case}"
            va, vb = [r[k] for r in res["a"]], [r[k] for r in res["b"]]
            ma, mb = statistics.median(va), statistics.median(vb)
            log(f"  {k}: a median {ma:.3f} ms (spread {max(va) - min(va):.3f}) b median {mb:.3f} ms "
                f"(spread {max(vb) - min(vb):.3f}); b / a = {mb / ma:.2f}; checksum a {res['a'][0][k + '_sum']:.6g} "
                f"b {res['b'][0][k + '_sum']:.6g}")
        mb_fwd = statistics.median(r[f"{name}_istft_fwd"] for r in res["b"])
        mbytes = res["b"][0][f"{name}_mbytes"]
        log(f"  {name}: ISTFT forward reads the spectrum and writes the waveform once: {mbytes:.1f} MB, "
            f"{mbytes * 1e6 / HBM_PEAK * 1e3:.4f} ms at {HBM_PEAK / 1e12:.1f} TB/s: "
            f"{100 * mbytes * 1e6 / HBM_PEAK * 1e3 / mb_fwd:.1f} % of the HBM peak end to end (arm b, launch included)")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=("a", "b"))
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "istft_ab.log"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.arm:
        child(a)
    else:
        sys.exit(driver(a))
