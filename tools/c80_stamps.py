#!/usr/bin/env python3
"""Phase stamps of the 80-channel conv kernel at the shape of DRN-L's RCAB chain in the C3 forward (8 x 64 x 64 px, bf16 input,
ReLU, no residual): the stamped instance of the kernel through srad_op_conv80_h with bit 16 of rmode, synchronously; the library
prints the per-phase medians of the fifth and sixth launch to stderr.
    python tools/c80_stamps.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from srad_amd import _lib as L
from srad_amd import ops

STAMPS = 1 << 16
B, H, W = 8, 64, 64

torch.manual_seed(1)
x = torch.randn(B * H * W, 80, device="cuda").to(torch.bfloat16)
w = torch.randn(80, 80, 3, 3, device="cuda") / 27.0
b = torch.randn(80, device="cuda")
for _ in range(6):
    y = ops.conv80_bf16(x, w, b, B=B, H=H, W=W, act=L.ACT_RELU, rmode=STAMPS)
torch.cuda.synchronize()
print("done", tuple(y.shape))
