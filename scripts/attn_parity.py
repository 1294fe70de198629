"""Bit identity of the self-attention kernels (csrc/attention.hip) between two
builds of libsbk.so (GPU box, not the product).

    [SBK_PROBE_LIB=other/libsbk.so] python scripts/attn_parity.py dump OUT.npz
    python scripts/attn_parity.py compare A.npz B.npz

`dump` launches, in the order of tests/test_gpu_selfattn_paths.CASES and from
that module's seeded inputs, every case of the ten kernel ids at T = 1, 63,
64, 65, 129, 200 and 577 (additive masks, "misq" and "pkld4" layouts
included), the T = 2113 and 4096 cases of the two LDS-DMA ids, and both DMA
ids at the encoder's shape B = 32, T = 376, H = 4, dh = 64; out and probs go
into one .npz as raw integers.  The kernels use no atomics, so `compare`
expects every array bit-identical; it prints one line per differing array
and the totals."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import speechbrain_amd._lib as _L  # noqa: E402
if os.environ.get("SBK_PROBE_LIB"):
    _L.LIB_PATH = os.path.abspath(os.environ["SBK_PROBE_LIB"])
from gemm_parity import _raw, compare  # noqa: E402

TS = (1, 63, 64, 65, 129, 200, 577)
TS_DMA = (2113, 4096)


def dump(path):
    import test_gpu_selfattn_paths as S
    dev = torch.device("cuda")
    out = {}
    cases = [c for c in S.CASES.values() if c.T in TS or (c.kern.startswith("dma") and c.T in TS_DMA)]
    for kern, api in (("dma_band", "relpos"), ("dma_plain", "mha")):  # the encoder's shape
        cases.append(SimpleNamespace(id=f"{kern}-encoder-T376-B32H4", kern=kern, dt="bf16", dh=64, probs=False,
                                     lay="aligned", B=32, H=4, T=376, fam="ord", kpm="none", am=None, d=256, api=api))
    for c in cases:
        assert S._dispatch(c)[0] == c.kern, c.id
        n = S._inputs(c)
        o, p = S._launch(c, n, S._operands(c, n, dev))
        out[f"{c.kern}/{c.id}/out"] = _raw(o)
        if c.probs:
            out[f"{c.kern}/{c.id}/probs"] = _raw(p)
    torch.cuda.synchronize()
    assert {k.split("/")[0] for k in out} == set(S.KERNELS)
    np.savez(path, **out)
    print(f"{len(out)} arrays from {_L.LIB_PATH} -> {path}")


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
