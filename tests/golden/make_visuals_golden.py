"""Writes tests/golden/visuals_ref.npz: the inputs of tests/visual_cases.py and the bytes the REFERENCE's own util/util.py
(tensor2im, tensor2mask, tensor2flow) and util/flow_util.py (flow2img) produce from them on the CPU, with the numpy version that did.

    python tests/golden/make_visuals_golden.py <path to a checkout of the reference>

Runs only where the reference exists (its modules are loaded by path; nothing of its text is copied).  util.py imports cv2 at module
level, which tensor2im / tensor2mask / tensor2flow never touch: an EMPTY stand-in module named cv2 is put into sys.modules so that the
import succeeds.  tensor2att needs the real cv2 (applyColorMap) and is not recorded.

Keys: in/<kind>/<case> the input (up to 4096 elements; a larger one is seeded, and sha256/<kind>/<case> of its bytes is kept instead),
ref/<kind>/<case> uint8 [B, H, W, 3] the reference's output image by image (idx = 0 .. B - 1).
The reference casts with astype(uint8), which is undefined outside [0, 256): what it gave on this numpy build is recorded as it came
out, and the tests compare those cells for information only (tests/test_visuals_cpu.py)."""
import hashlib
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # the repository root
import visual_cases as cases  # noqa: E402

if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "util", "flow_util.py")):
    sys.exit(__doc__)
sys.path.insert(0, sys.argv[1])
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
from util import util as ref_util  # noqa: E402

out = {"numpy_version": np.array(np.__version__), "torch_version": np.array(torch.__version__)}


def record(kind, name, array, fn):
    t = torch.from_numpy(array)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # the reference divides 0 / 0 and casts NaN on purpose-built cases
        with np.errstate(all="ignore"):
            imgs = [np.ascontiguousarray(fn(t.clone(), idx=i)) for i in range(array.shape[0])]
    if array.size <= 4096:
        out["in/%s/%s" % (kind, name)] = array
    else:
        out["sha256/%s/%s" % (kind, name)] = np.array(hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest())
    out["ref/%s/%s" % (kind, name)] = np.stack(imgs).astype(np.uint8)


for name, x in cases.image_cases().items():
    record("image", name, x, ref_util.tensor2im)
    record("mask", name, x, ref_util.tensor2mask)
for name, f in cases.flow_cases().items():
    record("flow", name, f, ref_util.tensor2flow)

path = os.path.join(HERE, "visuals_ref.npz")
np.savez_compressed(path, **out)
print("wrote %s: %d arrays, %d bytes, numpy %s" % (path, len(out), os.path.getsize(path), np.__version__))
