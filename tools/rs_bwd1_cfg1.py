"""resample2d d_input1 at BASELINE configs[0] ([1,64,128,128], ks 4, flow ~ U[-3,3)) and at [8,64,512,512]: the tap-lane kernel (option
rs_bwd1_variant 0 = default, 5 = 16-row tiles) against round 2's plane / tile kernels (1 = plane where it fits, 2 = tile);
HIP-event time of the backward launches."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ffwm_amd import _lib, ops
lib = _lib.load()
g = torch.Generator().manual_seed(0)
dev = "cuda"
for shape in ((1, 64, 128, 128), (8, 64, 512, 512)):
    B, C, H, W = shape
    in1 = torch.rand(*shape, generator=g).to(dev)
    in2 = torch.cat((torch.rand(B, 2, H, W, generator=g) * 6 - 3, torch.full((B, 1, H, W), 2.0)), 1).to(dev)
    go = torch.rand(*shape, generator=g).to(dev)
    g1 = torch.zeros_like(in1)
    for variant in (0, 5, 1, 2):
        lib.ffwm_set_option(b"rs_bwd1_variant", variant)
        for _ in range(2):
            ops.resample2d_backward(in1, in2, go, 4, 1, g1, None)
        torch.cuda.synchronize()
        _lib.prof_reset(); _lib.prof_enable(True)
        for _ in range(5):
            ops.resample2d_backward(in1, in2, go, 4, 1, g1, None)
        torch.cuda.synchronize(); _lib.prof_enable(False)
        rows = _lib.prof_collect()
        print(shape, "variant", variant, {k: round(v["avg_ms"] * 1e3, 1) for k, v in rows.items()})
    lib.ffwm_set_option(b"rs_bwd1_variant", 0)
