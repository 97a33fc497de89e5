"""The shared cases of the result-image tests (tests/test_visuals_cpu.py, tests/test_gpu_visuals.py) and of the fixture generator
(tests/golden/make_visuals_golden.py): seeded numpy float32 arrays [B, C, H, W], the smallest at which the kernel of
csrc/visuals.hip can still go wrong -- odd sizes whose pixel count is no multiple of the 4 pixels a thread owns, images that a
thread's four pixels straddle, planes larger than the one workgroup that reduces a flow image's maximum and than the workgroup of the
colouring pass, and the values at which the stated arithmetic has a seam."""
import collections

import numpy as np

from ffwm_amd import visuals as V


def _rng(seed):
    return np.random.RandomState(seed)


def identity_grid(B, H, W):
    """The sampling grid tensor2flow maps to zero motion: (f + 1) * (H / 2) = x and y -- both scaled with H, as the reference does."""
    x = np.arange(W, dtype=np.float32) * np.float32(2.0 / H) - np.float32(1)
    y = np.arange(H, dtype=np.float32) * np.float32(2.0 / H) - np.float32(1)
    g = np.stack([np.broadcast_to(x[None, :], (H, W)), np.broadcast_to(y[:, None], (H, W))])
    return np.ascontiguousarray(np.broadcast_to(g[None], (B, 2, H, W))).astype(np.float32)


def image_cases():
    """name -> (array, kinds it is rendered as).  Values in [0, 1) unless the name says otherwise."""
    c = collections.OrderedDict()
    c["rgb_2x3x5x7"] = _rng(1).rand(2, 3, 5, 7).astype(np.float32)          # 70 pixels: 70 % 4 == 2, planes of 35
    c["gray_2x1x5x7"] = _rng(2).rand(2, 1, 5, 7).astype(np.float32)
    s = _rng(3).rand(1, 3, 4, 4).astype(np.float32)
    special = [0.0, 1.0, 1.0 - 2.0 ** -24, 0.5, -0.25, 1.5, 300.0, np.nan, np.inf, -np.inf, 2.0 ** 24, -(2.0 ** 24), 255.5 / 255.0, -0.0]
    s.reshape(3, 16)[0, :len(special)] = special
    s.reshape(3, 16)[1, :len(special)] = special[::-1]
    s.reshape(3, 16)[2, 2:2 + len(special)] = special
    c["special_1x3x4x4"] = s
    g = _rng(4).rand(1, 1, 4, 4).astype(np.float32)
    g.reshape(16)[:len(special)] = special
    c["special_1x1x4x4"] = g
    return c


def mixed_table():
    """Three items of different sizes for ONE call: fake_F32 beside fake_F128, and an odd-sized 1-channel mask."""
    return [("fake_F32", V.IMAGE, _rng(5).rand(1, 3, 32, 32).astype(np.float32)),
            ("fake_F128", V.IMAGE, _rng(6).rand(1, 3, 128, 128).astype(np.float32)),
            ("mask_S", V.MASK, _rng(7).rand(2, 1, 5, 7).astype(np.float32))]


def flow_cases():
    c = collections.OrderedDict()
    c["uniform_16"] = (_rng(10).rand(1, 2, 16, 16) * 2 - 1).astype(np.float32)
    two = identity_grid(2, 8, 8)
    d = (_rng(11).rand(2, 8, 8) * 2 - 1).astype(np.float32)
    two[0] += d * np.float32(0.5)
    two[1] += d * np.float32(0.05)               # image 1 moves 10 times less: its own maximum must normalise it
    c["two_scales_2x8"] = two
    c["identity_8"] = identity_grid(1, 8, 8)     # no motion: maxrad 0, 0 / 0, black
    sx = identity_grid(1, 16, 16)
    sx[0, 0] += np.float32(3 * 2.0 / 16)
    c["shift_x3_16"] = sx                        # atan2 on the axis
    sy = identity_grid(1, 16, 16)
    sy[0, 1] += np.float32(3 * 2.0 / 16)
    c["shift_y3_16"] = sy
    n = c["uniform_16"].copy()
    n[0, 0, 5, 9] = np.nan
    c["one_nan_16"] = n
    i = c["uniform_16"].copy()
    i[0, 0, 2, 3] = np.inf
    i[0, 1, 11, 4] = -np.inf
    c["two_inf_16"] = i
    b = c["uniform_16"].copy()
    b[0, 0, 0, :4] = 50.0
    b[0, 1, 7, 3:9] = -50.0
    b[0, 0, 15, 15] = -50.0
    c["clamped_50_16"] = b
    c["uniform_128"] = (_rng(12).rand(1, 2, 128, 128) * 2 - 1).astype(np.float32)
    c["uniform_20"] = (_rng(13).rand(1, 2, 20, 20) * 2 - 1).astype(np.float32)       # 400 cells: less than one pass of the reduction
    # 1089 cells, an odd count: the scalar route of the workgroup that reduces an image's maximum, more than one pass of its threads
    side = 33
    assert side * side > V.FLOW_REDUCTION_BLOCK and (side * side) % 4
    c["uniform_33"] = (_rng(16).rand(1, 2, side, side) * 2 - 1).astype(np.float32)
    c["nonsquare_8x12"] = (_rng(14).rand(1, 2, 8, 12) * 2 - 1).astype(np.float32)
    c["odd_2x5x7"] = (_rng(15).rand(2, 2, 5, 7) * 2 - 1).astype(np.float32)      # planes of 35: a thread's four pixels straddle two images
    # 16384 cells: several float4 passes of that workgroup, several workgroups of the colouring pass
    assert 128 * 128 > V.FLOW_REDUCTION_PASS and 128 * 128 > V.PIXELS_PER_BLOCK
    return c


def palette_case():
    return _rng(20).rand(2, 1, 5, 7).astype(np.float32), _rng(21).randint(0, 256, size=(256, 3)).astype(np.uint8)


def undecided(flow, idx):
    """(image, undecided mask [H, W], largest level difference between the two perturbed images): a pixel is undecided when moving
    arctan2's result by +4 or by -4 ulp changes one of its bytes."""
    base = V.tensor2flow(flow, idx)
    up, down = V.tensor2flow(flow, idx, atan2_ulps=4), V.tensor2flow(flow, idx, atan2_ulps=-4)
    und = (up != base).any(axis=2) | (down != base).any(axis=2)
    spread = int(np.abs(up.astype(np.int32) - down.astype(np.int32)).max())
    return base, und, spread
