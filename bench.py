"""Headline benchmark (BASELINE.json metric): audio-sec/sec of
Fbank → ConvolutionFrontEnd → Conformer encoder forward on synthetic 16 kHz
batches of 32 x 15 s per GPU (weak scaling: every rank encodes its own
batch; no collective on the data path).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--d-model 256] [--full] [--dump-outputs DIR]
    torchrun --nproc-per-node N bench.py --gpus N ...

One step = one pass of the hot path over one batch already resident in HBM:
fused Fbank kernel (+top_db clamp) → 2 fused ConvBlocks → src Linear →
12 Conformer layers → final LayerNorm, bf16 MFMA (torch.autocast bf16),
captured once into a HIP graph and replayed.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line.
--dump-outputs DIR also writes what the last timed step returned (the
encoder output a caller of the step receives) as DIR/<name>.npy, float32;
inputs and weights are seeded, so two builds can be compared array for array.

With --full also reported (rank 0, N=1 path of the contract):
  roofline      the dominant kernel (the FFN layer-chain kernel; the other
                fused encoder kernels are listed beside it): its launches of one step re-issued back to
                back from a HIP graph on the launch stream and timed with HIP
                events (average launch duration, as rocprofv3 reports it);
                achieved = algorithmic FLOPs / time; traffic = HBM bytes per
                launch from the committed rocprofv3 PMC passes.
  cpu_baseline  the from-scratch CPU restatement (oracle/, PyTorch CPU fp32)
                of the same path on a bounded sample, host threads stated.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SR = 16000
SECONDS = 15.0
BATCH = 32
PEAK_BF16_TFLOPS = 2500.0  # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3  # MI355X exact-f32 MFMA = the f32 vector rate (MI355X_MICROARCH.md)
_T0 = time.perf_counter()


def progress(msg):
    """One line per phase on stderr (stdout carries only the JSON line)."""
    print(f"[bench {time.perf_counter() - _T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


DUMP_BYTES = 60_000_000  # --dump-outputs writes at most this much array data in all (under 64 MB with the headers)


def dump_outputs(path, arrays):
    """--dump-outputs: each tensor of `arrays` ({name: tensor}) as
    path/<name>.npy in float32.  An output beyond its share of DUMP_BYTES is
    written as a fixed sample: its flattened elements at sorted indices drawn
    without replacement by numpy's default_rng(0) (the same indices every run)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    cap = DUMP_BYTES // (4 * max(1, len(arrays)))  # elements per array
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy()
        if a.size > cap:
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=cap, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))
        progress(f"wrote {name}.npy {a.shape} to {path}")


def build_model(d_model, dev, layers=12):
    from speechbrain_amd.lobes.features import Fbank
    from speechbrain_amd.lobes.models.convolution import ConvolutionFrontEnd
    from speechbrain_amd.lobes.models.transformer.TransformerASR import TransformerASR
    torch.manual_seed(0)
    fbank = Fbank(sample_rate=SR, n_fft=400, n_mels=80)
    cnn = ConvolutionFrontEnd(input_shape=(8, 10, 80), num_blocks=2, num_layers_per_block=1, out_channels=(64, 32),
                              kernel_sizes=(3, 3), strides=(2, 2), residuals=(False, False))
    tr = TransformerASR(tgt_vocab=5000, input_size=640, d_model=d_model, nhead=4, num_encoder_layers=layers,
                        num_decoder_layers=0, d_ffn=1024, dropout=0.1, encoder_module="conformer",
                        attention_type="RelPosMHAXL", normalize_before=True, causal=False)
    return fbank.to(dev).eval(), cnn.to(dev).eval(), tr.to(dev).eval()


def make_step(fbank, cnn, tr, wav, wav_len, precision="bf16"):
    """The timed step: Fbank (fused spectrum kernel; its top_db floor applied
    by the front-end as it loads the rows) → both ConvBlocks in one bf16
    kernel → TransformerASR.encode under bf16 autocast (fused FFN /
    conv-module / LDS-DMA attention kernels).  Also what
    tests/test_gpu_bench_parity.py runs against the fp32 oracle.  (The
    batch as 2 or 4 utterance groups on concurrent streams in one graph
    measured no faster in rounds 2 and 4: 1.339 / 1.355 vs 1.333 ms,
    profiles/r04i_bench_s*.log — the kernels already fill the chip.)"""
    if precision == "fp32":
        # the parity precision: no autocast, every GEMM / attention product on
        # the exact-f32 MFMA path (the 1e-4 parity of tests/test_gpu_encoder.py)
        def step():
            with torch.no_grad():
                feats, topdb = fbank.forward_deferred(wav)
                src = cnn.run(feats, torch.float32, topdb=topdb)
                return tr.encode(src, wav_len)
        return step

    def step():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            feats, topdb = fbank.forward_deferred(wav)
            src = cnn.run(feats, torch.bfloat16, topdb=topdb)
            return tr.encode(src, wav_len)
    return step


def encoder_flops(B, T_e, d, dff=1024, k=31, H=4, layers=12, T1=751, F1=40, T2=376, F2=20, c1=64, c2=32,
                  in_dim=640):
    """Algorithmic FLOPs of one step: per layer QKV 6d², out 2d²,
    FFN 2x4·d·dff, conv 4d²+2kd+2d², scores 2T·d + 2(2T-1)·d, AV 2T·d per token,
    linear_pos 2(2T-1)d² per layer; plus front-end convs and the src Linear."""
    per_tok = (6 * d * d + 2 * d * d + 2 * 4 * d * dff + 4 * d * d + 2 * k * d + 2 * d * d
               + 2 * T_e * d + 2 * (2 * T_e - 1) * d + 2 * T_e * d)
    enc = layers * (B * T_e * per_tok + 2 * (2 * T_e - 1) * d * d)
    front = B * (2 * T1 * F1 * c1 * 9 + 2 * T2 * F2 * c2 * 9 * c1) + B * T_e * 2 * in_dim * d
    return enc + front


def gemm_flops(M, N, K):
    return 2.0 * M * N * K


def _usable_cpus():
    try:
        return len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        return os.cpu_count() or 1


def pick_threads(probe):
    """The CPU baseline's thread count: SURVEY §8d times the reference CPU path
    on the host's cores (torch.set_num_threads(os.cpu_count())).  A GPU box's
    process may hold only a share of the machine (OMP_NUM_THREADS is set to
    it), where os.cpu_count() threads oversubscribe; so one short probe pass
    runs at each candidate — OMP_NUM_THREADS and 2x / 4x it (16 / 32 / 64 on
    the GPU box), the affinity mask, os.cpu_count(), those beyond 4x
    OMP_NUM_THREADS skipped — and the fastest is used.  Returns (threads,
    {threads: probe seconds})."""
    omp = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    cpus = os.cpu_count() or 1
    cands = {c for c in (omp, 2 * omp, 4 * omp, _usable_cpus(), cpus) if 1 <= c <= cpus}
    if omp >= 1:  # a share is set: far beyond it only oversubscribes (minutes per pass)
        cands = {c for c in cands if c <= 4 * omp}
    times = {}
    for c in sorted(cands):
        torch.set_num_threads(c)
        t0 = time.perf_counter()
        probe()  # warm-up at this thread count
        warm = time.perf_counter() - t0
        if times and warm > 4 * min(times.values()) + 2.0:
            # oversubscribed (the machine's cores, not this process's share):
            # a second pass would only spend minutes confirming it
            times[c] = round(warm, 4)
        else:
            t0 = time.perf_counter()
            probe()
            times[c] = round(time.perf_counter() - t0, 4)
        progress(f"thread probe: {c} threads {times[c]:.3f} s")
    best = min(times, key=times.get)
    torch.set_num_threads(best)
    return best, times


def cpu_baseline(d_model, n_utt=64, reps=3):
    """Oracle (PyTorch CPU fp32 restatement) on n_utt x 15 s, median of `reps`."""
    import oracle.conformer as OC
    fbank, cnn, tr = build_model(d_model, "cpu")
    sd_cnn = cnn.state_dict()
    sd_tr = tr.state_dict()
    g = torch.Generator().manual_seed(0)
    wav = 0.1 * torch.randn(n_utt, int(SR * SECONDS), generator=g)
    lens = torch.ones(n_utt)
    with torch.no_grad():
        threads, tried = pick_threads(lambda: OC.fbank_to_encoder(wav[:2], sd_cnn, sd_tr, 12, 4, n_mels=80,
                                                                  wav_len=lens[:2]))
    progress(f"cpu baseline: {threads} threads (probe {tried})")
    times = []
    with torch.no_grad():
        for r in range(reps + 1):
            t0 = time.perf_counter()
            OC.fbank_to_encoder(wav, sd_cnn, sd_tr, 12, 4, n_mels=80, wav_len=lens)
            progress(f"cpu baseline rep {r}: {time.perf_counter() - t0:.2f} s")
            if r:
                times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"value": round(n_utt * SECONDS / med, 2), "unit": "audio-sec/sec", "cores": threads, "kind": "port",
            "threads_probe_s": tried, "os_cpu_count": os.cpu_count(), "affinity_cpus": _usable_cpus(),
            "sample": f"{n_utt} utt x 15 s synthetic, fp32, median of {reps} after 1 warm-up; threads = fastest "
                      f"of {sorted(tried)} on a 2-utterance probe; CPU: {model}"}


class _LaunchProbe:
    """Wraps one speechbrain_amd._enc entry point and records every call of
    the timed precision (is_bf16: the selector, bf16 or fp32 operands) in one eager step (arguments kept alive) with its algorithmic FLOPs
    (`flops_of(*args, **kw)`).  `replay_time()` then captures exactly those
    calls, back to back, `reps` times into one HIP graph on the launch stream
    (torch's current stream, the one the ctypes kernels use) and times the
    replays with HIP events: the average launch duration of the kernel as it
    runs inside the step's graph, without per-launch event or host gaps — the
    quantity rocprofv3 --kernel-trace reports for it."""

    def __init__(self, name, flops_of, is_bf16, module=None):
        from speechbrain_amd import _enc
        self._enc = module if module is not None else _enc
        self.name = name
        self.orig = getattr(self._enc, name)
        self.flops_of = flops_of
        self.is_bf16 = is_bf16
        self.calls = []
        self.flops = 0.0

    def __enter__(self):
        probe = self

        def wrapped(*args, **kw):
            if probe.is_bf16(*args, **kw):
                probe.calls.append((args, kw))
                probe.flops += probe.flops_of(*args, **kw)
            return probe.orig(*args, **kw)
        setattr(self._enc, self.name, wrapped)  # callers resolve _enc.<name> at call time
        return self

    def __exit__(self, *exc):
        setattr(self._enc, self.name, self.orig)

    def replay_time(self, reps=10, rounds=3):
        """(ms per step's worth of launches, launches per step, FLOPs per step)."""
        if not self.calls:
            return 0.0, 0, 0.0

        def body():
            for a, k in self.calls:
                self.orig(*a, **k)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            body()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                body()
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(rounds):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (rounds * reps), len(self.calls), self.flops


def _ffn_flops(x, ln0, w1, *a, **k):
    return 4.0 * x.shape[0] * x.shape[1] * w1.shape[0]


def _ffn_proj_flops(x, ln0, w1, b1, act, slope, w2, b2, alpha, next_ln, wp, *a, **k):
    """FFN (2 GEMMs, 4·D·H per row) + the fused next-block projection (2·D·NP)."""
    return _ffn_flops(x, ln0, w1) + 2.0 * x.shape[0] * x.shape[1] * wp.shape[0]


def _ffn_chain_flops(x, a, b, act, slope, next_ln, wp, *r, **k):
    """Two FFN blocks (a, b) + the fused next-block projection."""
    M, D = x.shape
    return 4.0 * M * D * (a[1].shape[0] + b[1].shape[0]) + 2.0 * M * D * wp.shape[0]


def _conv_module_flops(x, B, T, ln0, w1p, b1p, wc, bc, causal, ln1, w2, b2, kpm=None, pre=None, **k):
    """pointwise 2d->(GLU) 4d², depthwise 2kd, pointwise 2d², + out_proj 2d² when fused (pre)."""
    M, D = x.shape
    return float(M) * (4 * D * D + 2 * wc.shape[0] * D + 2 * D * D + (2 * D * D if pre is not None else 0))


def _gemm_flops(a, w, *r, **k):
    return gemm_flops(a.shape[0], w.shape[0], a.shape[1])


def _attn_flops(qkv, pk, pbu, pbv, kpm, B, T, H, dh, *a, **k):
    """scores 2·T·d + 2·(2T−1)·d and P·V 2·T·d per query token."""
    return float(B) * T * H * dh * (8 * T - 2)


def load_traffic():
    """Per-launch HBM bytes of the profiled kernels (rocprofv3 PMC FETCH_SIZE x2
    (gfx950 correction) + WRITE_SIZE), committed under profiles/."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        with open(path) as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


def max_over_ranks(elapsed, world, device):
    """The slowest rank's wall time (the job finishes when it does)."""
    if world <= 1:
        return elapsed
    t = torch.tensor([elapsed], device=device, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def per_rank(elapsed, world, device):
    """Every rank's wall time, in rank order (reported beside the max)."""
    if world <= 1:
        return [elapsed]
    t = torch.tensor([elapsed], device=device, dtype=torch.float64)
    out = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(out, t)
    return [float(x.item()) for x in out]


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(script, argv, n):
    """`--gpus N` without a torchrun launcher: start N child processes of
    `script` (one per GPU, RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* set as torchrun
    would, rendezvous on 127.0.0.1) and return the first failing rank's exit code (0
    when every rank succeeds).  Called
    before this process touches the GPU, so the parent never initialises HIP;
    the children are started (not exec'd) and the parent waits for all."""
    import subprocess
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
        procs.append(subprocess.Popen([sys.executable, script, *argv], env=env))
    # poll every rank: the first one that fails ends the others (its peers
    # would otherwise block in a collective until the process-group timeout)
    codes = {}
    first_fail = None  # the exit code of the first rank that failed on its own
    while len(codes) < n:
        for r, p in enumerate(procs):
            if r not in codes and p.poll() is not None:
                codes[r] = p.returncode
                if p.returncode != 0:
                    if first_fail is None:
                        first_fail = p.returncode
                    for q in procs:
                        if q.poll() is None:
                            q.terminate()
                    for q in procs:
                        try:
                            q.wait(timeout=30)
                        except subprocess.TimeoutExpired:
                            q.kill()
                            q.wait()
                    for r2, q in enumerate(procs):
                        codes.setdefault(r2, q.returncode)
        time.sleep(0.05)
    # the peers this function terminated report -15: the failing rank's own
    # code is the one to return
    return first_fail if first_fail is not None else max(codes.values(), key=abs)


def rank_env(gpus):
    """(world, rank, local_rank) from the torchrun environment; the world size
    must equal --gpus (a launcher that started fewer ranks than asked for would
    otherwise report a silently wrong scaling point)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != gpus:
        raise SystemExit(f"--gpus {gpus} but WORLD_SIZE={world}: launch with torchrun --nproc-per-node {gpus} "
                         f"or without WORLD_SIZE set (bench.py then starts the ranks itself)")
    return world, int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))


def launch_plumbing(args):
    """`--plumbing`: the launcher + rendezvous + max-over-ranks timing on CPU
    (gloo), a fixed sleep per rank instead of the GPU step.  Used by the CPU
    test of the multi-rank contract."""
    world, rank, _ = rank_env(args.gpus)
    if os.environ.get("SBK_PLUMBING_FAIL_RANK") == str(rank):
        sys.exit(3)  # the launcher test's crashing rank: its peer must not wait for it
    if world > 1:
        dist.init_process_group("gloo")
        assert dist.get_world_size() == args.gpus
    t0 = time.perf_counter()
    time.sleep(0.05 * (1 + rank))
    mine = time.perf_counter() - t0
    elapsed = max_over_ranks(mine, world, torch.device("cpu"))
    ranks = per_rank(mine, world, torch.device("cpu"))
    if rank == 0:
        print(json.dumps({"metric": "plumbing", "n_gpus": world, "elapsed": elapsed, "rank_s": ranks,
                          "world_from_dist": dist.get_world_size() if world > 1 else 1}), flush=True)
    if world > 1:
        dist.destroy_process_group()


# ----------------------------------------------------------------- config 2
PEAK_HBM_GBS = 8000.0  # MI355X HBM3E (MI355X_MICROARCH.md)


def run_c2(args, world, rank, dev):
    """BASELINE config 2: the feature kernels on synthetic
    16 kHz B=32 x 15 s — Fbank(n_mels=80, deltas=True): the spectrum kernel,
    then one stencil kernel [x | Δ | ΔΔ] (240 dims) that applies the top_db
    floor as it loads — then SpecAugment with the recipe parameters
    (conformer_small.yaml:252-262; host draws from the CPU generator, seed
    1234+step, as the reference), in place.  HBM-bound: the roofline is GB/s
    of algorithmic bytes against 8 TB/s."""
    from speechbrain_amd import ops
    from speechbrain_amd.lobes.augment import SpecAugment
    from speechbrain_amd.lobes.features import Fbank
    fb = Fbank(sample_rate=SR, n_fft=400, n_mels=80, deltas=True).to(dev)
    sa = SpecAugment(time_warp=True, time_warp_window=5, time_warp_mode="bicubic", freq_mask=True,
                     freq_mask_width=(0, 30), n_freq_mask=2, time_mask=True, time_mask_width=(0, 40), n_time_mask=2,
                     replace_with_zero=False)
    g = torch.Generator().manual_seed(1234 + rank)
    wav = (0.1 * torch.randn(args.batch, int(SR * SECONDS), generator=g)).to(dev)
    it = [0]

    def step():
        # the draws come from the CPU generator (the reference's); seeding only
        # it (torch.manual_seed also seeds every GPU generator: ~57 us of host
        # time per step, more than a third of the step's kernels)
        torch.default_generator.manual_seed(1234 + it[0])
        it[0] += 1
        with torch.no_grad():
            return sa(fb(wav))  # Fbank(deltas=True): [fbank | Δ | ΔΔ], the top_db floor applied on load
    out = step()
    B, T, F3 = out.shape
    # a C2 step is ~0.1 ms: ten times the requested steps / warm-up, so the
    # timed region is not the first milliseconds of a cold clock (20 steps
    # timed 0.22 ms per step against 0.11 ms over 200, profiles/r04l_c2_host.log)
    steps, warmup = 10 * args.steps, 10 * args.warmup
    elapsed, rank_ms, last = time_steps(step, steps, warmup, world, dev)
    ms_per_step = 1000.0 * elapsed / steps
    value = world * args.batch * SECONDS * steps / elapsed
    if rank != 0:
        return
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"features": out if last is None else last})
    res = {
        "metric": "audio-sec/sec STFT+Filterbank+Deltas+SpecAugment (16kHz, B=32x15s)",
        "value": round(value, 1), "unit": "audio-sec/sec", "n_gpus": world, "steps": steps,
        "warmup": warmup, "ms_per_step": round(ms_per_step, 4), "rank_ms_per_step": rank_ms,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic (0.1·N(0,1) 16 kHz)",
        "config": {"workload": f"C2: Fbank(80) → Δ/ΔΔ (240) → SpecAugment(recipe, in place), B={args.batch}×15s "
                               f"per GPU, eager (host mask draws per step)",
                   "global_batch": world * args.batch, "seq_len": T, "parallelism": f"replicas{world}"},
    }
    if not args.full:
        print(json.dumps(res), flush=True)
        return
    # per-kernel: each op alone, back to back, HIP events on the launch stream.
    # SpecAugment's kernels are timed on one fixed host draw (the op itself):
    # the module's per-call host draws (five CPU randint calls, the mask
    # copies) take longer than its kernels, so timing the module would time
    # the host
    f80, (smax, topdb) = fb._deferred(wav)
    d240 = ops.deltas_floor(f80, 5, smax, topdb)
    S = wav.shape[1]
    torch.manual_seed(1234)
    c, w, fm, tm = sa.draws(B, T, F3)
    if c == w:
        c = w = -1
    fm_d, tm_d = fm.to(dev), tm.to(dev)

    def sa_kernels():  # the masked-cell count on the device (-1), as the module does
        torch.ops.sbk.specaugment_(d240, B, T, F3, c, w, fm_d, tm_d, True, -1, 0)
    kern = []
    traffic = load_traffic()
    for name, fn, nbytes, pmc in (
            ("spec_reg_kernel (Fbank, register FFT, top_db floor deferred)", lambda: fb._deferred(wav),
             4.0 * B * S + 4.0 * B * T * 80, ("spec_reg_kernel<2, false>",)),
            ("deltas4_concat_kernel (floor(x)|Δ|ΔΔ)", lambda: ops.deltas_floor(f80, 5, smax, topdb),
             4.0 * B * T * 80 + 4.0 * B * T * 240, ("deltas4_concat_kernel",)),
            ("specaugment (in place: roll4 warp + sums, fixup4 masked cells)", sa_kernels, 2 * 4.0 * B * T * 240,
             ("roll4_kernel<true, true, true>", "fixup4_kernel"))):
        # device time per call: `reps` calls captured in one HIP graph and
        # replayed (host dispatch excluded, kernels back to back)
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        reps = 20
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        try:
            gs = torch.cuda.Stream()
            gs.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(gs):
                fn()
            torch.cuda.current_stream().wait_stream(gs)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(reps):
                    fn()
            g.replay()
            torch.cuda.synchronize()
            e0.record()
            g.replay()
            e1.record()
        except RuntimeError as exc:  # not capturable: eager back-to-back calls
            progress(f"probe {name}: eager timing ({exc})")
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
        torch.cuda.synchronize()
        us = 1000.0 * e0.elapsed_time(e1) / reps
        tr = [traffic.get(k) for k in pmc]
        kern.append({"kernel": name, "us": round(us, 2), "algorithmic_bytes": int(nbytes),
                     "traffic": sum(tr) if all(v is not None for v in tr) else None,
                     "achieved": round(nbytes / (us * 1e-6) / 1e9, 1), "unit": "GB/s",
                     "frac": round(nbytes / (us * 1e-6) / 1e9 / PEAK_HBM_GBS, 4)})
    dom = max(kern, key=lambda k: k["us"])
    kernel_sum_us = sum(k["us"] for k in kern)
    res.update({
        "kernel_sum_us": round(kernel_sum_us, 2), "step_over_kernel_sum": round(1000.0 * ms_per_step / kernel_sum_us, 3),
        "roofline": {"bound": "hbm", "kernel": dom["kernel"], "achieved": dom["achieved"], "peak": PEAK_HBM_GBS,
                     "unit": "GB/s", "frac": dom["frac"], "traffic": dom["traffic"],
                     "avg_launch_us": dom["us"], "other_kernels": [k for k in kern if k is not dom]},
    })
    if not args.no_cpu_baseline and world == 1:
        res["cpu_baseline"] = cpu_baseline_c2(args.batch)
    print(json.dumps(res), flush=True)


def cpu_baseline_c2(batch, n_utt=4, reps=3):
    """Oracle (numpy/PyTorch CPU restatement) of the same C2 step on n_utt x 15 s."""
    import oracle.augment as OA
    import oracle.features as OF
    wav = 0.1 * torch.randn(n_utt, int(SR * SECONDS), generator=torch.Generator().manual_seed(0))
    threads, tried = pick_threads(lambda: OF.fbank(wav[:1], deltas_on=True, n_mels=80))
    times = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        d = OF.fbank(wav, deltas_on=True, n_mels=80)
        torch.manual_seed(1234)
        OA.spec_augment(d, time_warp_window=5, freq_mask_width=(0, 30), time_mask_width=(0, 40),
                        replace_with_zero=False)
        progress(f"cpu baseline rep {r}: {time.perf_counter() - t0:.2f} s")
        if r:
            times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    return {"value": round(n_utt * SECONDS / med, 2), "unit": "audio-sec/sec", "cores": threads, "kind": "port",
            "threads_probe_s": tried, "os_cpu_count": os.cpu_count(), "affinity_cpus": _usable_cpus(),
            "sample": f"{n_utt} utt x 15 s synthetic, fp32, median of {reps} after 1 warm-up; threads = fastest "
                      f"of {sorted(tried)} on a 1-utterance probe"}


# ----------------------------------------------------------------- config 5
C5_LAYERS, C5_D, C5_H, C5_FFN = 24, 1024, 16, 4096
PEAK_MXFP8_TFLOPS = 5000.0  # MI355X dense FP8 (block-scaled MFMA), MI355X_MICROARCH.md


def build_c5(dev, layers=C5_LAYERS):
    """BASELINE config 5: W2VLatentExtractor defaults (512 ch,
    k [11,3,...], s [5,2,...]) → EncoderWrapper(Linear 512→1024 + positional
    encoding) → TransformerEncoder(24L, d=1024, H=16, ffn 4096, GELU,
    pre-norm).  Random init (torch.manual_seed(0))."""
    from speechbrain_amd.lobes.models.transformer.Transformer import TransformerEncoder
    from speechbrain_amd.lobes.models.wav2vec import EncoderWrapper, W2VLatentExtractor
    torch.manual_seed(0)
    ext = W2VLatentExtractor()
    enc = TransformerEncoder(num_layers=layers, nhead=C5_H, d_ffn=C5_FFN, d_model=C5_D, dropout=0.0,
                             activation=torch.nn.GELU, normalize_before=True)
    wrap = EncoderWrapper(512, C5_D, enc, dropout_encoder_input=0.0)
    return ext.to(dev).eval(), wrap.to(dev).eval()


def c5_flops(B, S=240000, layers=C5_LAYERS, d=C5_D, dff=C5_FFN, C=512, ks=(11, 3, 3, 3, 3, 3, 3),
             ss=(5, 2, 2, 2, 2, 2, 2)):
    """Algorithmic FLOPs of one config-5 step: latent-extractor convs
    (2·T_i·C_out·C_in·k per utterance), the input projector, and per layer
    QKV 6d², out 2d², FFN 4·d·dff per token plus scores / P·V 4·T·d."""
    T, cin, fl = S, 1, 0.0
    for k, s in zip(ks, ss):
        T = (T - k) // s + 1
        fl += 2.0 * B * T * C * cin * k
        cin = C
    fl += 2.0 * B * T * C * d
    per_tok = 6 * d * d + 2 * d * d + 4 * d * dff + 4 * T * d
    return fl + layers * B * T * per_tok, T


def make_c5_step(ext, wrap, wav, wav_len, prec):
    import speechbrain_amd as sba

    def step():
        with torch.no_grad():
            if prec == "mxfp8":
                with sba.mxfp8():
                    lat, T = ext.run(wav, True, "mx")
                    return wrap.embed(lat, wav.shape[0], T, wav_len)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                lat, T = ext.run(wav, True, torch.bfloat16)
                return wrap.embed(lat, wav.shape[0], T, wav_len)
    return step


def cpu_baseline_c5(n_utt=1, reps=2):
    """Oracle (PyTorch CPU fp32 restatement, oracle/wav2vec.py) of config 5 on
    n_utt x 15 s, median of `reps` after a warm-up."""
    import oracle.wav2vec as OW
    ext, wrap = build_c5("cpu")
    sde, sdw = ext.state_dict(), wrap.state_dict()
    wav = 0.1 * torch.randn(n_utt, int(SR * SECONDS), generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        threads, tried = pick_threads(lambda: OW.wav2vec_encode(wav[:1, :32000], sde, sdw, 2, C5_H,
                                                                wav_lens=torch.ones(1)))
    times = []
    with torch.no_grad():
        for r in range(reps + 1):
            t0 = time.perf_counter()
            OW.wav2vec_encode(wav, sde, sdw, C5_LAYERS, C5_H, wav_lens=torch.ones(n_utt))
            progress(f"cpu baseline rep {r}: {time.perf_counter() - t0:.2f} s")
            if r:
                times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    return {"value": round(n_utt * SECONDS / med, 2), "unit": "audio-sec/sec", "cores": threads, "kind": "port",
            "threads_probe_s": tried, "os_cpu_count": os.cpu_count(), "affinity_cpus": _usable_cpus(),
            "sample": f"{n_utt} utt x 15 s synthetic, fp32, median of {reps} after 1 warm-up; threads = fastest "
                      f"of {sorted(tried)} on a 2 s / 2-layer probe"}


def _mha_flops(qkv, pk, pbu, pbv, kpm, B, T, H, dh, *a, **k):
    """Plain multi-head attention: scores 2·T·dh + P·V 2·T·dh per (query, head)
    (the zero positional band the rel-pos kernel also evaluates is not counted)."""
    return float(B) * T * H * dh * 4 * T


def _mx_flops(a, w, *r, **k):
    return 2.0 * a.q.shape[0] * w.q.shape[0] * a.q.shape[1]


def run_c5(args, world, rank, dev):
    prec = args.precision
    ext, wrap = build_c5(dev)
    g = torch.Generator().manual_seed(1234 + rank)
    wav = (0.1 * torch.randn(args.batch, int(SR * SECONDS), generator=g)).to(dev)
    wav_len = torch.ones(args.batch, device=dev)
    step = make_c5_step(ext, wrap, wav, wav_len, prec)
    out = step()
    T = out.shape[0] // args.batch
    run = capture(step, args.no_graph)
    elapsed, rank_ms, last = time_steps(run, args.steps, args.warmup, world, dev)
    ms_per_step = 1000.0 * elapsed / args.steps
    value = world * args.batch * SECONDS * args.steps / elapsed
    if rank != 0:
        return
    if args.dump_outputs:  # a graph replay returns nothing: its output is the captured tensor
        dump_outputs(args.dump_outputs, {"encoder_out": last if last is not None else
                                         (out if args.no_graph else capture.out)})
    res = {
        "metric": "audio-sec/sec wav2vec2 CNN frontend + 24L TransformerEncoder fwd (16kHz, B=32x15s)",
        "value": round(value, 1), "unit": "audio-sec/sec", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "rank_ms_per_step": rank_ms,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "mxfp8" if prec == "mxfp8" else "bf16", "data": "synthetic (0.1·N(0,1) 16 kHz, random-init weights)",
        "config": {"workload": f"C5: W2VLatentExtractor(512ch, 7 conv) → Linear 512→1024 → TransformerEncoder "
                               f"{C5_LAYERS}L d={C5_D} H={C5_H} ffn={C5_FFN} GELU pre-norm, B={args.batch}×15s per GPU"
                               + (" (GEMMs MXFP8 e4m3 + E8M0 block scales, attention bf16)" if prec == "mxfp8"
                                  else " (bf16)"),
                   "global_batch": world * args.batch, "seq_len": T, "parallelism": f"replicas{world}",
                   "hip_graph": not args.no_graph},
    }
    if not args.full:
        print(json.dumps(res), flush=True)
        return
    total, _ = c5_flops(args.batch)
    from speechbrain_amd import _enc, _w2v
    probes = [_LaunchProbe("mx_gemm", _mx_flops, lambda *a, **k: True, module=_w2v),
              _LaunchProbe("relpos_attention", _mha_flops, lambda qkv, *a, **k: qkv.dtype == torch.bfloat16)]
    if prec != "mxfp8":
        probes = [_LaunchProbe("gemm", _gemm_flops, lambda a, w, *r, **k: a.dtype == torch.bfloat16),
                  probes[1]]
    for p in probes:
        p.__enter__()
    try:
        step()
    finally:
        for p in probes:
            p.__exit__()
    kern = {}
    for p in probes:
        ms, n, fl = p.replay_time()
        if n:
            kern[p.name] = {"kernel": p.name, "launches_per_step": n, "avg_launch_us": round(1000.0 * ms / n, 3),
                            "achieved": round(fl / (ms * 1e-3) / 1e12, 2), "step_share_ms": round(ms, 4)}
    dom = max(kern.values(), key=lambda k: k["step_share_ms"])
    peak = PEAK_MXFP8_TFLOPS if (prec == "mxfp8" and dom["kernel"] == "mx_gemm") else PEAK_BF16_TFLOPS
    traffic = load_traffic()
    res.update({
        "roofline": {"bound": "mfma", "kernel": dom["kernel"], "achieved": dom["achieved"], "peak": peak,
                     "unit": "TFLOP/s", "frac": round(dom["achieved"] / peak, 4),
                     "traffic": traffic.get(dom["kernel"]), "launches_per_step": dom["launches_per_step"],
                     "avg_launch_us": dom["avg_launch_us"], "step_algorithmic_tflop": round(total / 1e12, 4),
                     "step_tflops_achieved": round(total / (ms_per_step * 1e-3) / 1e12, 2),
                     "other_kernels": [k for k in kern.values() if k is not dom]},
    })
    if not args.no_cpu_baseline and world == 1:
        res["cpu_baseline"] = cpu_baseline_c5()
    print(json.dumps(res), flush=True)


def capture(step, no_graph):
    """The step captured once into a HIP graph (replayed), or eager."""
    if no_graph:
        return step
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        capture.out = step()  # the tensor every replay writes its result into
    torch.cuda.synchronize()
    capture.graphs.append(graph)  # keep the graph (and its memory pool) alive
    return graph.replay


capture.graphs = []
capture.out = None


def time_steps(run, steps, warmup, world, dev):
    """W untimed runs, then exactly K timed, bracketed by barrier + synchronize;
    returns (max-over-ranks seconds, per-rank ms per step, what the last
    timed run returned: None for a graph replay)."""
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    last = None
    t0 = time.perf_counter()
    for _ in range(steps):
        last = run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    mine = time.perf_counter() - t0
    return (max_over_ranks(mine, world, dev), [round(1000.0 * t / steps, 4) for t in per_rank(mine, world, dev)],
            last)


def roofline_c3(args, step, fp32, T_e, ms_per_step):
    """--full, config 3: the roofline entry of the JSON line (None when no
    kernel of the timed precision was launched)."""
    total_flops = encoder_flops(args.batch, T_e, args.d_model)
    # per-kernel timing: the dominant kernels' launches of one step,
    # replayed back to back from a HIP graph and timed with HIP events
    # the calls of the timed precision (bf16 operands, or fp32 ones on the parity path)
    sel_dt = torch.float32 if fp32 else torch.bfloat16
    bf = lambda t: t.dtype == sel_dt  # noqa: E731
    probes = [_LaunchProbe("ffn_chain", _ffn_chain_flops, lambda x, a, *r, **k: bf(a[1])),
              _LaunchProbe("ffn_proj", _ffn_proj_flops, lambda x, ln0, w1, *a, **k: bf(w1)),
              _LaunchProbe("ffn", _ffn_flops, lambda x, ln0, w1, *a, **k: bf(w1)),
              _LaunchProbe("conv_module", _conv_module_flops, lambda x, B, T, ln0, w1p, *a, **k: bf(w1p)),
              _LaunchProbe("gemm", _gemm_flops, lambda a, w, *r, **k: bf(a)),
              _LaunchProbe("relpos_attention", _attn_flops, lambda qkv, *a, **k: bf(qkv))]
    for p in probes:
        p.__enter__()
    try:
        step()
    finally:
        for p in probes:
            p.__exit__()
    kern = {}
    labels = (("ffn_kernel<256, 1, true, true> (FFN2 + FFN1 + in_proj layer chain)",
               "ffn_kernel<256, 1, true, true>"),
              ("ffn_kernel<256, 1, true, false> (FFN1 + in_proj, layer 0)", "ffn_kernel<256, 1, true, false>"),
              ("ffn_kernel<256, 1, false, false> (final FFN2 + final LayerNorm)",
               "ffn_kernel<256, 1, false, false>"),
              ("conv_module_kernel<true> (out_proj + residual + conv module)", "conv_module_kernel<true>"),
              ("gemm_kernel<float> (exact-f32 projections, all tiles)" if fp32 else
               "gemm_kernel<bf16> (projections, all tiles)",
               "gemm_kernel<float" if fp32 else "gemm_kernel<unsigned short, 64, 64, 64, 2>"),
              ("relpos_flash_kernel<float> (rel-pos attention, exact f32)" if fp32 else
               "relpos_flash_dma_kernel (rel-pos attention)",
               "relpos_flash_kernel<float" if fp32 else "relpos_flash_dma_kernel"))
    for p, (label, pmc_key) in zip(probes, labels):
        ms, n, fl = p.replay_time()
        if n:
            kern[p.name] = {"kernel": label, "pmc_key": pmc_key, "launches_per_step": n,
                            "avg_launch_us": round(1000.0 * ms / n, 3),
                            "achieved": round(fl / (ms * 1e-3) / 1e12, 2),
                            "step_share_ms": round(ms, 4)}
    progress("per-kernel launch timing done")
    if not kern:
        return None
    dom = max(kern.values(), key=lambda k: k["step_share_ms"])
    traffic = load_traffic()
    peak = PEAK_F32_TFLOPS if fp32 else PEAK_BF16_TFLOPS
    return {
        "bound": "mfma", "kernel": dom["kernel"], "achieved": dom["achieved"], "peak": peak,
        "unit": "TFLOP/s", "frac": round(dom["achieved"] / peak, 4),
        "traffic": None if fp32 else traffic.get(dom["pmc_key"]),
        "traffic_source": "profiles/pmc_traffic.json (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE per launch)",
        "launches_per_step": dom["launches_per_step"], "avg_launch_us": dom["avg_launch_us"],
        "step_algorithmic_tflop": round(total_flops / 1e12, 4),
        "step_tflops_achieved": round(total_flops / (ms_per_step * 1e-3) / 1e12, 2),
        "other_kernels": [k for k in kern.values() if k is not dom]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--d-model", type=int, default=256)
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baseline out")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the per-kernel roofline figures (launches re-issued "
                         "from a HIP graph) and the same-run CPU baseline, and add them to the JSON line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32, at most 60 MB in all: "
                         "a fixed seeded sample of a larger output)")
    ap.add_argument("--config", choices=["c2", "c3", "c5"], default="c3",
                    help="c3: Fbank→Conformer (the BASELINE metric, default); c2: feature kernels "
                         "(Fbank, Δ/ΔΔ, SpecAugment); c5: wav2vec2 + 24L TransformerEncoder")
    ap.add_argument("--precision", choices=["mxfp8", "bf16", "fp32"], default=None,
                    help="c3: bf16 (default, the BASELINE config) or fp32 (the 1e-4 parity path); "
                         "c5: mxfp8 (default) or bf16")
    ap.add_argument("--plumbing", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.precision is None:
        args.precision = "mxfp8" if args.config == "c5" else "bf16"
    if (args.config == "c5" and args.precision == "fp32") or (args.config == "c3" and args.precision == "mxfp8"):
        ap.error(f"--precision {args.precision} is not offered for --config {args.config}")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus))
    if args.plumbing:
        return launch_plumbing(args)

    world, rank, local = rank_env(args.gpus)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)
        assert dist.get_world_size() == args.gpus
    if args.config in ("c2", "c5"):
        (run_c2 if args.config == "c2" else run_c5)(args, world, rank, dev)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    fbank, cnn, tr = build_model(args.d_model, dev)
    g = torch.Generator().manual_seed(1234 + rank)
    wav = (0.1 * torch.randn(args.batch, int(SR * SECONDS), generator=g)).to(dev)
    wav_len = torch.ones(args.batch, device=dev)

    fp32 = args.precision == "fp32"
    step = make_step(fbank, cnn, tr, wav, wav_len, args.precision)
    progress("model built")

    out = step()
    T_e = out.shape[1]
    torch.cuda.synchronize()
    graph = None
    if not args.no_graph:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = step()
        torch.cuda.synchronize()
        progress("graph captured")

    run = graph.replay if graph is not None else step
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    last = None
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = run()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    mine = time.perf_counter() - t0
    elapsed = max_over_ranks(mine, world, dev)
    rank_ms = [round(1000.0 * t / args.steps, 4) for t in per_rank(mine, world, dev)]
    ms_per_step = 1000.0 * elapsed / args.steps
    progress(f"timed {args.steps} steps: {ms_per_step:.3f} ms/step")
    audio = world * args.batch * SECONDS * args.steps
    value = audio / elapsed

    if rank == 0:
        if args.dump_outputs:  # a graph replay returns nothing: its output is the captured tensor
            dump_outputs(args.dump_outputs, {"encoder_out": out if (graph is not None or last is None) else last})
        res = {
            "metric": "audio-sec/sec Fbank→Conformer fwd (16kHz, B=32×15s) at 1/2/4/8 GPU",
            "value": round(value, 1),
            "unit": "audio-sec/sec",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "rank_ms_per_step": rank_ms,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "fp32" if fp32 else "bf16",
            "data": "synthetic (0.1·N(0,1) 16 kHz, random-init weights)",
            "config": {"workload": f"Fbank(80)→ConvFrontEnd(64,32)→Conformer 12L d={args.d_model} H=4 ffn=1024 "
                                   f"k=31 encode, B={args.batch}×15s per GPU" +
                                   (" (fp32: exact-f32 MFMA, the parity path)" if fp32 else ""),
                       "global_batch": world * args.batch, "seq_len": T_e, "parallelism": f"replicas{world}",
                       "hip_graph": graph is not None},
        }
        if args.full:
            res["roofline"] = roofline_c3(args, step, fp32, T_e, ms_per_step)
            if not args.no_cpu_baseline and world == 1:
                res["cpu_baseline"] = cpu_baseline(args.d_model)
        print(json.dumps(res), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
