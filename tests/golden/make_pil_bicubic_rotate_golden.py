"""Writes tests/golden/pil_bicubic_rotate.npz: what PIL's Image.rotate(angle, resample=BICUBIC) followed (where the case says so) by
transpose(FLIP_LEFT_RIGHT) gives for identity_data_cases.golden_cases(), recorded with PIL 12.2.0.  The file holds, per case,
`in/<key>` (the image), `out/<key>` (PIL's bytes), and `angles` / `flips` in the order of `keys`, so the tests that read it need no PIL.

    python tests/golden/make_pil_bicubic_rotate_golden.py
"""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import identity_data_cases as ic  # noqa: E402


def pil_item(img, angle, flip):
    out = Image.fromarray(img).rotate(angle, resample=Image.BICUBIC, expand=False)
    if flip:
        out = out.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(out, dtype=np.uint8)


if __name__ == "__main__":
    import PIL
    arrays, keys, angles, flips = {}, [], [], []
    for key, img, angle, flip in ic.golden_cases():
        arrays["in/" + key], arrays["out/" + key] = img, pil_item(img, angle, flip)
        keys.append(key)
        angles.append(angle)
        flips.append(flip)
    arrays.update(keys=np.array(keys), angles=np.array(angles, dtype=np.float64), flips=np.array(flips), pil_version=np.array(PIL.__version__))
    path = os.path.join(HERE, "pil_bicubic_rotate.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(keys), "cases, PIL", PIL.__version__)
