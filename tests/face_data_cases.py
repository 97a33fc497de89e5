"""The small face sets of the data tests, from numpy's frozen RandomState: tests/golden/make_face_dataset_golden.py feeds them to the
reference's FaceDataset, tests/test_face_data_cpu.py and tests/test_gpu_face_data.py feed them to ffwm_amd.data.FaceStore.

    case(name) -> {"images" uint8 [N, H, W, 3], "masks" uint8 [N, H, W], "names", "lm_dicts", "load_size"}

  s16    16 x 16, five files (P = 5), 9 landmarks chosen by hand: non-integral, negative, beyond 127 and beyond the image; lm_S float64,
         lm_F float32; image 0 holds every byte value, mask 0 too
  s128   128 x 128, four files, 580 landmarks in [-10, 140): lm_S float32, lm_F int64
  synthetic(...) any size, for the kernel tests (integral float landmarks)
"""
import numpy as np

FILES = {
    "s16": ["001_01_01_041_06.png", "001_01_01_051_06.png", "002_01_01_190_06.png", "002_01_01_051_06.png", "001_01_01_190_06.png"],
    "s128": ["003_01_01_051_06.png", "003_01_01_080_06.png", "004_02_01_051_07.png", "004_02_01_130_07.png"],
}
HAND = np.array([[-3.7, 0.5], [0.5, 15.99], [126.5, 16.0], [127.0, -0.3], [127.49, 7.2], [130.2, 200.9], [111.01, 3.999], [63.5, 1e6],
                 [-1e6, 12.0]])


def key(name):
    return name[:-7]


def s2f(name):
    ss = name.split("_")
    return "_".join((ss[0], ss[1], ss[2], "051", ss[4]))


def case(name):
    side, seed, L = {"s16": (16, 11, 9), "s128": (128, 12, 580)}[name]
    rs = np.random.RandomState(seed)
    names = list(FILES[name])
    N = len(names)
    images = rs.randint(0, 256, (N, side, side, 3)).astype(np.uint8)
    masks = rs.randint(0, 256, (N, side, side)).astype(np.uint8)
    every = np.arange(side * side * 3) % 256
    images[0] = rs.permutation(every).astype(np.uint8).reshape(side, side, 3)
    masks[0] = rs.permutation(np.arange(side * side) % 256).astype(np.uint8).reshape(side, side)
    lm_S, lm_F, gate = {}, {}, {}
    for n in names:
        if name == "s16":
            lm_S[key(n)] = HAND[rs.permutation(L)].astype(np.float64)
            lm_F[key(n)] = (HAND[rs.permutation(L)] + 0.25).astype(np.float32)
        else:
            lm_S[key(n)] = (rs.rand(L, 2) * 150.0 - 10.0).astype(np.float32)
            lm_F[key(n)] = rs.randint(-10, 140, (L, 2)).astype(np.int64)
        gate[key(n)] = (rs.rand(L) > 0.3).astype(np.float64)
    return {"images": images, "masks": masks, "names": names, "lm_dicts": {"lm_S": lm_S, "lm_F": lm_F, "gate": gate}, "load_size": side}


def synthetic(n_ids, H, W, L, seed, load_size=128):
    """2 n_ids files (a profile and its frontal file per identity, P = 2 n_ids pairs), landmarks integral floats in [-4, 132)."""
    rs = np.random.RandomState(seed)
    names = []
    for i in range(n_ids):
        names += ["%03d_01_01_051_06.png" % (i + 1), "%03d_01_01_%03d_06.png" % (i + 1, 10 * (i % 9) + 110)]
    N = len(names)
    images = rs.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    masks = rs.randint(0, 256, (N, H, W)).astype(np.uint8)
    lm_S, lm_F, gate = {}, {}, {}
    for n in names:
        lm_S[key(n)] = rs.randint(-4, 132, (L, 2)).astype(np.float64)
        lm_F[key(n)] = rs.randint(-4, 132, (L, 2)).astype(np.float64) + 0.5
        gate[key(n)] = (rs.rand(L) > 0.2).astype(np.float32)
    return {"images": images, "masks": masks, "names": names, "lm_dicts": {"lm_S": lm_S, "lm_F": lm_F, "gate": gate}, "load_size": load_size}
