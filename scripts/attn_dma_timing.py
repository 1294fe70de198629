"""Per-launch time of the two LDS-DMA attention kernels at the encoder's shape
(B = 32, T = 376, H = 4, dh = 64, bf16), for one build of libsbk.so (GPU box,
not the product).

    [SBK_PROBE_LIB=other/libsbk.so] python scripts/attn_dma_timing.py LABEL

Per row 10 warm-up launches, then 9 repeats of 50 launches between device
events; prints us per launch as median, min and max of the 9.  Run one
process per library and alternate them in one job."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import speechbrain_amd._lib as _L  # noqa: E402
if os.environ.get("SBK_PROBE_LIB"):
    _L.LIB_PATH = os.path.abspath(os.environ["SBK_PROBE_LIB"])
from speechbrain_amd import _enc  # noqa: E402

B, T, H, DH = 32, 376, 4, 64


def main(label):
    dev = torch.device("cuda")
    d = H * DH
    g = torch.Generator().manual_seed(0)
    qkv = torch.randn(B * T, 3 * d, generator=g).to(torch.bfloat16).to(dev)
    pk = torch.randn(2 * T - 1, d, generator=g).to(torch.bfloat16).to(dev)
    u, v = torch.randn(d, generator=g).to(dev), torch.randn(d, generator=g).to(dev)
    kpm = torch.zeros(B, T, dtype=torch.uint8, device=dev)
    rows = (("dma_band B32", lambda: _enc.relpos_attention(qkv, pk, u, v, kpm, B, T, H, DH, 1 / 16.0)),
            ("dma_plain B32", lambda: _enc.mha_attention(qkv, kpm, B, T, H, DH, 1 / 8.0)))
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, fn in rows:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(9):
            s.record()
            for _ in range(50):
                fn()
            e.record()
            torch.cuda.synchronize()
            us.append(s.elapsed_time(e) / 50 * 1e3)
        print(f"{label:8s} {name:24s} median {statistics.median(us):8.2f} us  min {min(us):8.2f}  max {max(us):8.2f}",
              flush=True)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "tree")
