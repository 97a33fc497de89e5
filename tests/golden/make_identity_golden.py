"""Generates tests/golden/reference_identity.pt by running the REFERENCE's own Python modules (imported from /root/reference, CPU):
the centre-face crop of --crop, the LightCNN-29 feature of the cropped input and the by-pose rank-1 meter.  Runs only in the build
container; the fixture (data: inputs are re-derived from tests/golden/fill.py and from seeds, outputs are stored) is what travels.

    python tests/golden/make_identity_golden.py
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
sys.modules.setdefault("cv2", types.ModuleType("cv2"))          # util/util.py imports it for its image helpers (never used here)

import fill  # noqa: E402
import identity_bounds as ib  # noqa: E402
from models import base_networks, losses  # noqa: E402
from lightcnn import light_cnn  # noqa: E402
from util import util  # noqa: E402

torch.set_num_threads(8)
out = {}

with torch.no_grad():
    lc = fill.fill_module(light_cnn.LightCNN_29Layers()).eval()
    iden = losses.IdentityLoss(lc, crop=True)
    img = fill.image(2, 3, 128, 128, "ident_img")
    # FFWMModel.test (models/ffwm_model.py:196-201): gray first, then the crop
    gray = torch.mean(img, dim=(1,), keepdim=True)
    grid = iden.build_grid(2, 98).type_as(gray)
    cropped = F.interpolate(base_networks.WarpNet()(gray, grid), (128, 128), mode="bilinear")
    _, fc, _ = lc(cropped)
    out["cropped"] = cropped
    out["fc_cropped"] = fc

    # AverageMeter (util/util.py:141-181) on the synthetic probes / gallery of tests/identity_bounds.py
    names, keys, probe, gallery = ib.meter_case()
    meter = util.AverageMeter()
    meter.update(probe, names, gallery, keys, topk=1)
    out["meter"] = {"stat_dict": meter.stat_dict, "str": str(meter), "names": names, "keys": keys}

path = os.path.join(HERE, "reference_identity.pt")
torch.save(out, path)
print("wrote reference_identity.pt  %.1f KiB" % (os.path.getsize(path) / 1024.0))
