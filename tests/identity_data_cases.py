"""The images, angles and flips of the identity-data tests, from numpy's frozen RandomState: tests/golden/make_pil_bicubic_rotate_golden.py
feeds them to PIL once and records what it gives, tests/test_identity_data_cpu.py and tests/test_gpu_identity_data.py feed them to
ffwm_amd.data.

    cases()          140 of them: 5 sizes x 4 image kinds x 7 angles -> [(key, image uint8 [H, W, 3], angle, flip)]
    golden_cases()   the ones recorded in tests/golden/pil_bicubic_rotate.npz: every case of the four small sizes and two of 128 x 128
    synthetic(...)   names and images of a small set for the store / loader / kernel tests
"""
import numpy as np

SIZES = [(128, 128), (37, 53), (5, 4), (1, 1), (2, 9)]          # (H, W)
KINDS = ("random", "binary", "ramp_x", "ramp_y")
FIXED_ANGLES = [0.0, 5.0, -5.0, 1e-9]
GOLDEN_128 = ("128x128_random_2", "128x128_random_5")          # -5 degrees, and a drawn angle


def image(kind, H, W, rs):
    if kind == "random":
        return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    if kind == "binary":
        return (rs.randint(0, 2, (H, W, 3)) * 255).astype(np.uint8)
    ramp = np.arange(W)[None, :, None] * 255 // max(W - 1, 1) if kind == "ramp_x" else np.arange(H)[:, None, None] * 255 // max(H - 1, 1)
    return np.broadcast_to(ramp + np.array([0, 1, 2])[None, None, :], (H, W, 3)).clip(0, 255).astype(np.uint8)


def cases():
    out = []
    for si, (H, W) in enumerate(SIZES):
        for ki, kind in enumerate(KINDS):
            rs = np.random.RandomState(100 * si + ki)
            img = image(kind, H, W, rs)
            angles = FIXED_ANGLES + list(rs.uniform(-5.0, 5.0, 3))
            for ai, angle in enumerate(angles):
                out.append(("%dx%d_%s_%d" % (H, W, kind, ai), img, float(angle), bool((si + ki + ai) % 2)))
    return out


def golden_cases():
    return [c for c in cases() if not c[0].startswith("128x128") or c[0] in GOLDEN_128]


def synthetic(N, H, W, seed):
    """N images of two files per identity ('001_01_01_051_06.png', '001_01_01_110_06.png', '002_...'), image 0 with every byte value
    when it has room for them."""
    rs = np.random.RandomState(seed)
    names = ["%03d_01_01_%s_06.png" % (i // 2 + 1, "051" if i % 2 == 0 else "%03d" % (110 + 10 * (i // 2 % 9))) for i in range(N)]
    images = rs.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    if H * W * 3 >= 256:
        images[0] = rs.permutation(np.arange(H * W * 3) % 256).astype(np.uint8).reshape(H, W, 3)
    return names, images
