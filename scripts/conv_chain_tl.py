"""s_memtime timeline of the fused layer kernel (sbk_conv_ffn_chain: conv
module of layer i, FFN2 + norm2 of layer i, FFN1 + norm1 + in_proj of layer
i+1) for every wave of workgroup 128 (a full tile) and of workgroup 127 (the
last tile of an utterance, 40 live rows: the projection tail stores at the
block ends and after the loop), at the headline shape (B = 32, T = 376,
H = 1024, kernel size 31).  Probe build with -DSBK_PROBE_TL; never the product.
usage: scripts/probe_build.sh speechbrain_amd/csrc/ffn.hip TL, then
       SBK_PROBE_LIB=<the TL probe library it wrote> python scripts/conv_chain_tl.py"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import speechbrain_amd._lib as _L  # noqa: E402
_L.LIB_PATH = os.path.abspath(os.environ["SBK_PROBE_LIB"])
from speechbrain_amd import _enc  # noqa: E402
from speechbrain_amd.lobes.models.transformer.Conformer import ConvolutionModule  # noqa: E402
from speechbrain_amd.nnet.activations import Swish  # noqa: E402
from speechbrain_amd.nnet.attention import PositionalwiseFeedForward  # noqa: E402

dev = torch.device("cuda")
D, H, B, T, K = 256, 1024, 32, 376, 31
torch.manual_seed(0)
cm = ConvolutionModule(D, K, causal=False).to(dev).eval()
fa = PositionalwiseFeedForward(H, input_size=D, activation=Swish).to(dev).eval()
fb = PositionalwiseFeedForward(H, input_size=D, activation=Swish).to(dev).eval()
lns = [(torch.randn(D, device=dev) * 0.5 + 1, torch.randn(D, device=dev) * 0.1, 1e-5) for _ in range(4)]
x = (torch.randn(B * T, D, device=dev) * 2 + 0.3).contiguous()
o = torch.randn(B * T, D, device=dev).to(torch.bfloat16)
wo = _enc.cast_bf16(torch.randn(D, D, device=dev) / 16)
bo = torch.randn(D, device=dev) * 0.1
wp = _enc.cast_bf16(torch.randn(3 * D, D, device=dev) / 16)
a, b = fa.chain_block(lns[0], 0.5, post_ln=lns[1]), fb.chain_block(lns[2], 0.5)
with torch.no_grad():
    for _ in range(5):
        _enc.conv_ffn_chain(x, B, T, (o, wo, bo), cm.fused_params(), None, a, b, "swish", 0.0, lns[3], wp)
torch.cuda.synchronize()
buf = (ctypes.c_ulonglong * (16 * 256))()
lib = ctypes.CDLL(_L.LIB_PATH)
assert lib.sbk_probe_ffn_tl(buf) == 0
tl = np.array(buf, dtype=np.int64).reshape(16, 256)
# marks in program order: conv stage 210 .. 218 (its start split by 219 .. 222, its middle phases by 223 .. 229), chain 1, A steps, 197 .. 198, B steps, 194 .. 196
names = [("start", 0), ("cs in", 210), ("o landed", 219), ("staged", 211), ("wo k0 landed", 220), ("last mfma", 221),
         ("x landed", 222), ("xres reloc", 227), ("out_proj+sums", 212), ("xchg bar 1", 228), ("xchg bar 2", 229),
         ("LN0", 213), ("ph1 gemm", 214), ("b1 landed", 223), ("GLU", 215), ("taps landed", 224), ("window", 225),
         ("ph2a", 216), ("2b params", 226), ("ph2b", 217), ("ph3", 218), ("A LN0 (loop)", 1), ("A steps", 3 + 2 * 31),
         ("seam in", 197), ("seam z", 200), ("postLN", 201), ("LN0b", 202), ("Xn bar", 203), ("frags", 198),
         ("B steps", 3 + 2 * 63), ("epi in", 194), ("epi z", 195), ("nextLN", 204), ("Zo/Xn bar", 205),
         ("proj", 206), ("end", 196)]
print("s_memtime ticks (as the committed chain timelines), wave by wave; each column: mark time / delta to the previous")
for wg, rows in ((128, tl[:8]), (127, tl[8:])):
    # each workgroup against its own first mark (the two run on different XCDs)
    rel = rows - rows[:, 0].min()
    print(f"workgroup {wg} ({'full tile' if wg == 128 else 'last tile of utterance 15, 40 live rows'}):")
    for w in range(8):
        r = rel[w]
        prev, cells = r[0], []
        for nm, i in names:
            cells.append(f"{nm} {r[i]}/{r[i] - prev}")
            prev = r[i]
        print(f"w{w}: " + " | ".join(cells))
    med = np.median(rel, axis=0).astype(np.int64)
    prev = med[0]
    print(f"median over the waves of workgroup {wg}:")
    for nm, i in names:
        print(f"  {nm:16s} at {med[i]:7d}  +{med[i] - prev}")
        prev = med[i]
    print(f"  end of the last wave {rel[:, 196].max()}, waves 0-3 proj {np.median(rel[:4, 206] - rel[:4, 205]):.0f}, "
          f"waves 4-7 proj {np.median(rel[4:, 206] - rel[4:, 205]):.0f}")
