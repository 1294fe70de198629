"""Restatement of the time-domain augmentation arithmetic in numpy, float64
by default: the polyphase sum of Resample, DropFreq's correlation, DropChunk's
segment fill and amplitude, and their chain.  Run with dtype=np.float32 it
gives E32, the error of the same arithmetic in the kernels' precision, from
which the tests' bound max(1e-6, 8 E32) comes.

Each function takes a `fault` that models one wrong kernel; `mismatch` (the
check the GPU tests apply to kernel outputs) has to reject every one of them
(tests/test_tdaug_cpu.py).
"""
import numpy as np

TAPS = 101
PAD = TAPS // 2


def resample(x, first, w, M, T_out, dtype=np.float64, fault=None, span=None):
    """x (B, T) or (B, T, C): y[k L + i] = sum_j w[i][j] x[first[i] + k M + j],
    x zero outside [0, T), j ascending.
    fault: 'phase' (weights of the next phase), 'sign' (first index negated),
    'truncate' (windows that pass the end of the input give zero).
    span (lo, hi): the output positions lo..hi-1 instead of 0..T_out-1, the
    same formula continued past the ends (floor division)."""
    x = np.asarray(x)
    xs = x[:, :, None] if x.ndim == 2 else x
    B, T, C = xs.shape
    first = np.asarray(first).astype(np.int64)
    w = np.asarray(w, dtype)
    L, W = w.shape
    n = np.arange(T_out) if span is None else np.arange(*span)
    i, k = n % L, n // L
    base = (-first[i] if fault == "sign" else first[i]) + k * M
    wi = (i + 1) % L if fault == "phase" else i
    y = np.zeros((B, len(n), C), dtype)
    for j in range(W):
        t = base + j
        ok = (t >= 0) & (t < T)
        xv = np.where(ok[None, :, None], xs[:, np.clip(t, 0, T - 1), :].astype(dtype), dtype(0))
        y = y + w[wi, j][None, :, None] * xv
    if fault == "truncate":
        y[:, base + W - 1 >= T, :] = 0
    return y[:, :, 0] if x.ndim == 2 else y


def fir101(x, taps, dtype=np.float64, fault=None):
    """x (B, T): y[t] = sum_k taps[k] x[t + k - 50], zero padding, k ascending.
    fault: 'flip' (a convolution instead of the correlation)."""
    x = np.asarray(x, dtype)
    taps = np.asarray(taps, dtype)
    if fault == "flip":
        taps = taps[::-1]
    B, T = x.shape
    xp = np.zeros((B, T + 2 * PAD), dtype)
    xp[:, PAD:PAD + T] = x
    y = np.zeros((B, T), dtype)
    for k in range(TAPS):
        y = y + taps[k] * xp[:, k:k + T]
    return y


def amplitude(x, lengths, dtype=np.float64):
    """sum_t |x[b, t]| over all T, over the absolute length of the row."""
    return np.abs(np.asarray(x, dtype)).sum(1) / np.asarray(lengths, dtype)


def drop_chunks(x, segs, noise=None, noff=None, lengths=None, noise_factor=0.0, dtype=np.float64, fault=None):
    """x (B, T) or (B, T, C) with the [start, end) segments of segs (B, S, 2)
    zeroed, or filled with 2 nm u - nm, nm = 2 amp_b noise_factor, u =
    noise[noff[b][j] + t - start]; later segments overwrite earlier ones.
    `segs` may pass T only with fault='noclip', which models a kernel that
    does not clip an end at T: it writes on into the next row."""
    x = np.asarray(x)
    y = np.array(x, dtype)
    B, T = y.shape[:2]
    flat = y.reshape(B * T, -1)
    amp = amplitude(x, lengths, dtype) if noise is not None else None
    for b in range(B):
        for j, (s, e) in enumerate(np.asarray(segs)[b]):
            if fault != "noclip":
                assert 0 <= s <= T and e <= T, "segments are clipped at T by the caller"
            if e <= s:
                continue
            if noise is None:
                flat[b * T + s:b * T + e] = 0
            else:
                nm = dtype(2) * amp[b] * dtype(noise_factor)
                u = np.asarray(noise, dtype)[noff[b][j]:noff[b][j] + e - s]
                flat[b * T + s:b * T + e, 0] = dtype(2) * nm * u - nm
    return y


def chain(x, table=None, taps=None, segs=None, dtype=np.float64, fault=None):
    """resample -> fir101 -> drop_chunks (zero fill) of x (B, T); a stage
    whose argument is None is dropped.  table: (first, w, M, T_out).
    fault: 'halo' models a fused kernel that fills the filter's halo past
    the ends of the resampled signal with extrapolated resample values
    instead of zeros."""
    y = np.asarray(x, dtype)
    if table is not None:
        first, w, M, T_out = table
        if fault == "halo" and taps is not None:
            ext = resample(y, first, w, M, T_out, dtype, span=(-PAD, T_out + PAD))
            f = np.asarray(taps, dtype)
            y = np.zeros((y.shape[0], T_out), dtype)
            for k in range(TAPS):
                y = y + f[k] * ext[:, k:k + T_out]
            taps = None
        else:
            y = resample(y, first, w, M, T_out, dtype)
    if taps is not None:
        y = fir101(y, taps, dtype)
    if segs is not None:
        y = drop_chunks(y, segs, dtype=dtype)
    return y


def bound(ref64, ref32):
    """max(1e-6, 8 E32), E32 the float32 restatement's distance from the
    float64 one."""
    e32 = float(np.abs(np.asarray(ref32, np.float64) - np.asarray(ref64, np.float64)).max()) if np.size(ref64) else 0.0
    return max(1e-6, 8 * e32)


def mismatch(got, ref64, ref32):
    """None when `got` has the reference's shape, is finite and lies within
    bound(ref64, ref32) of it; otherwise a description of the failure."""
    got = np.asarray(got)
    if got.shape != np.shape(ref64):
        return f"shape {got.shape} != {np.shape(ref64)}"
    if not np.isfinite(got).all():
        return "non-finite output"
    if got.size == 0:
        return None
    err = np.abs(got.astype(np.float64) - ref64)
    b = bound(ref64, ref32)
    if err.max() > b:
        at = np.unravel_index(err.argmax(), err.shape)
        return f"max |err| {err.max():.3e} > {b:.3e} at {tuple(int(a) for a in at)}"
    return None


def flat_draws(module):
    """A drop-in's last_draws as the flat float64 sequence the fixture keeps:
    every value in the order the reference's forward draws them."""
    name = type(module).__name__
    d = module.last_draws
    parts = []

    def put(v):
        parts.append(np.asarray(v, np.float64).reshape(-1))

    if name == "TimeDomainSpecAugment":
        return np.concatenate([flat_draws(m) for m in (module.speed_perturb, module.drop_freq, module.drop_chunk)])
    put(d[0])
    if d[1] is not None:
        put(d[1])
        if name == "DropFreq":
            put(d[2])
        if name == "DropChunk":
            for c, nz in zip(d[2], d[3]):
                if c is not None:
                    put(c[0])
                    put(c[1])
                    for v in nz:
                        put(v)
    return np.concatenate(parts)
