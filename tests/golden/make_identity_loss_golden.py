"""Generates tests/golden/reference_identity_loss.pt by running the REFERENCE's own IdentityLoss (models/losses.py:76-112, imported
from /root/reference, CPU, float64) around a small stand-in identity network, with crop=False and crop=True.  Runs only in the build
container; the fixture (tensors only: the losses and d loss / d out; the inputs are re-derived from tests/golden/fill.py) is what travels.

    python tests/golden/make_identity_loss_golden.py

The stand-in is `StandIn` of tests/identity_train_bounds.py, restated here so that the fixture does not depend on the module under
test: a seeded linear map (8 x 8 average pooling, then a [24, 256] matrix) that returns (None, fc, pool).  The inputs `out` and `gt`
[2, 3, 128, 128] are float32 values (identity_train_bounds.loss_inputs, from tests/golden/fill.py) held in float64, so that a float32 run starts from the same numbers.  The reference treats the three channels alike, so d loss / d out
is the same plane in each of them: channel 0 is stored, with the largest difference of the other two from it (a committed file stays
under 1 MiB).
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REF)
np.int = int                                   # base_networks.py:366 uses the removed alias
tv = types.ModuleType("torchvision")           # losses.py:3 imports torchvision.models (never used here)
tv.models = types.ModuleType("torchvision.models")
sys.modules["torchvision"] = tv
sys.modules["torchvision.models"] = tv.models

import identity_train_bounds as tb  # noqa: E402
from models import losses  # noqa: E402


class StandIn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(29)
        self.register_buffer("w", (torch.rand(24, 256, generator=gen, dtype=torch.float64) * 2.0 - 1.0) / 16.0)

    def forward(self, x):
        f = (F.avg_pool2d(x, 8).reshape(x.shape[0], 1, -1) * self.w.unsqueeze(0)).sum(-1)          # (products and a plain sum: no BLAS call)
        return None, f[:, :16], f[:, 16:]


torch.set_num_threads(8)
img_out, img_gt = tb.loss_inputs()
out = {}
for crop in (False, True):
    x = img_out.clone().requires_grad_(True)
    loss = losses.IdentityLoss(StandIn(), crop=crop)(x, img_gt)
    loss.backward()
    key = "crop" if crop else "plain"
    out["loss_" + key] = loss.detach().clone()
    out["grad_" + key] = x.grad[:, :1].clone()
    out["grad_spread_" + key] = (x.grad - x.grad[:, :1]).abs().max()
    print(key, float(loss), float(x.grad.abs().max()))

path = os.path.join(HERE, "reference_identity_loss.pt")
torch.save(out, path)
print("wrote reference_identity_loss.pt  %.1f KiB" % (os.path.getsize(path) / 1024.0))
