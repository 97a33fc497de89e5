"""Generates tests/golden/cv2_warp_affine.npz: what OpenCV's own warpAffine gives for the inputs of the rotation of --aug, so that
tests/test_face_aug_cpu.py can hold ffwm_amd.data.warp_affine_linear against cv2's bytes and not only against its restatement.

    python tests/golden/make_face_aug_golden.py          # where `import cv2` works

It has NOT been run for this repository: no OpenCV was at hand when the rotation was written.  Until the file exists the CPU test that
reads it is skipped, and "equal to cv2's bytes" rests on the restatement of the classic warpAffine path (OpenCV 2.4 to 4.10).

Recorded for the s16 case of tests/face_data_cases.py, the calls of the reference's aug_transform (data/face_dataset.py:113-117) on the
float32 images and masks that --preload holds: for every angle of np.random.randint(-5, 5) and every file, unflipped,
    mat = cv2.getRotationMatrix2D((w // 2, h // 2), angle, 1);  cv2.warpAffine(img, mat, (w, h))
  images uint8 [N, 16, 16, 3], masks uint8 [N, 16, 16], angles int64 [10],
  warped_images float32 [10, N, 16, 16, 3], warped_masks float32 [10, N, 16, 16]          (about 200 KiB)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import face_data_cases as fc  # noqa: E402


def main():
    import cv2
    c = fc.case("s16")
    images, masks = c["images"], c["masks"]
    h, w = images.shape[1:3]
    angles = np.arange(-5, 5, dtype=np.int64)
    warped_images, warped_masks = [], []
    for ang in angles.tolist():
        mat = cv2.getRotationMatrix2D((w // 2, h // 2), int(ang), 1)
        warped_images.append(np.stack([cv2.warpAffine(im.copy().astype("float32"), mat, (w, h)) for im in images]))
        warped_masks.append(np.stack([cv2.warpAffine(m[:, :, np.newaxis].copy().astype("float32"), mat, (w, h)) for m in masks]))
    out = os.path.join(HERE, "cv2_warp_affine.npz")
    np.savez(out, images=images, masks=masks, angles=angles, warped_images=np.stack(warped_images).astype(np.float32),
             warped_masks=np.stack(warped_masks).astype(np.float32), cv2_version=np.array(cv2.__version__))
    print("wrote %s with OpenCV %s" % (out, cv2.__version__))


if __name__ == "__main__":
    main()
