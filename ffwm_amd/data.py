"""The reference's input pipeline (data/face_dataset.py with --preload, data/__init__.py's DataLoader) with the set kept ON THE DEVICE.

    store = FaceStore.from_directory(dataroot, "multipie", isval=False).to("cuda:0")
    for batch in FaceLoader(store, batch_size=8, shuffle=True, seed=0):
        trainer.step(batch)

FaceStore holds what `--preload` holds -- every image [N, H, W, 3] and mask [N, H, W] as bytes, the pair table, the landmark and gate
tables -- as tensors; FaceStore.to(device) uploads them once.  FaceLoader draws an epoch's permutation on the host, uploads it once,
and assembles every batch with ONE launch of ops.face_batch on a slice of it: no per-item host work, no host-to-device copy, no
synchronisation.  On a CPU store the same batch comes from host_batch (the reference's own arithmetic, item by item), which is also
what the tests hold the kernel against.

What the reference does and this module reproduces (face_dataset.py:37-90, 132-174):
  * index i in [0, 2 P): i >= P is the flipped copy of pair i % P -- images and masks reversed along W, landmark x -> 127 - x (127
    whatever the image size), the subtraction made in the landmarks' own dtype BEFORE .long() truncates toward zero; then the clamp to
    [0, load_size - 1].  Both versions of every landmark row are worked out once, on the host, by those very numpy / torch calls;
  * images and masks are byte / 255 in float32 (Tensor.div: a true division);
  * landmark and gate rows are looked up by file[:-7]; lm_S, lm_F and gate are three dicts of landmarks.npy;
  * multipie pairs are (file, s2f(file)), other modes (file, file); a test item is img_S, img_F, input_path, unflipped;
  * the gallery is gallery_list.npy or the first *051_06.png per file[:3], each entry the channel mean of byte / 255.
Not reproduced: reading without --preload, sharding over ranks.  The reference walks os.listdir() order (arbitrary) and shuffles the
files before it picks a gallery; from_directory sorts the names, so "first" means first by name.

The random rotation of --aug (face_dataset.py:73-75, 110-130) is here as a STATED algorithm, asked for with `rotation=`:

    store = FaceStore.from_directory(dataroot, "multipie", rotation=True).to("cuda:0")
    for batch in FaceLoader(store, 8, seed=0, rotation=True):          # angles from np.random.randint(-5, 5)'s range

Its image half is cv2.warpAffine with bilinear interpolation, which is integer arithmetic from end to end: rotation_tables restates
getRotationMatrix2D, warpAffine's inversion and its four fixed-point tables (10 fractional bits, rounded to 1 / 32 pixel), and
warp_affine_linear the weighted sum of the four taps (5-bit fractions; the weights sum to 1024; a tap outside the image is 0).  On
the --preload path the images are float32, so the result sum / 1024 is exact in float32 whatever the order of the sums, and the
host restatement and the kernel (ffwm_face_batch_aug) agree bit for bit.  This is the classic warpAffine path of OpenCV 2.4 to 4.10
as its source states it; NO OpenCV WAS AVAILABLE TO CONFIRM that cv2's bytes are these bytes (tests/golden/make_face_aug_golden.py
records cv2's output where cv2 exists, and the CPU test compares against that file when it is there).  That is why aug=True, which
means "the reference's bytes, certified", still raises, and the argument is called rotation.  The landmark half is the reference's
four numpy lines in float32, step by step, as numpy 1.x's value-based casting evaluates them (rotate_landmarks).  Only img_S, mask_S
(binarised: > 0 -> 1, even at angle 0) and lm_S change; the flip comes first, then the rotation.  The reference draws its angles
from numpy's global state inside its loader workers, so ITS sequence of draws cannot be reproduced; the distribution is the same.

The input pipeline of LightCNN fine-tuning (lightcnn/dataset.py with --preload, finetune.py:98-106, 145-148) is here too:

    store = IdentityStore.from_directory(dataroot, isval=False).to("cuda:0")
    for epoch in range(epochs):
        loss, prec1, prec5 = trainer.train_epoch(IdentityLoader(store, 64, crop=True, seed=0), epoch)

IdentityStore holds the images as bytes and the class of every image (int(name[:3]) - 1); IdentityLoader draws an epoch's permutation,
rotation angles and flips on the host, uploads them once, and assembles every batch {"img", "target"} with ONE launch of
ops.identity_batch (csrc/identity_batch.hip) on slices of them.  What the reference does per training item and this module reproduces
(dataset.py:19-24, 57-67): ToPILImage, RandomRotation(5, BICUBIC), RandomHorizontalFlip, ToTensor, torch.mean over the channels,
and with --crop the slice [:, 28:-2, 15:-15] resized bilinearly to 128 x 128; a test item is byte / 255, the mean and the same crop.
The rotation is PIL's Image.rotate: rotation_matrix and rotate_bicubic restate it in float64 (numpy; the run time needs no PIL), and
tests/golden/pil_bicubic_rotate.npz records what PIL 12.2 gives for the same inputs -- the bytes are equal.  The reference draws its
angles and flips from Python's global `random` inside its loader workers, so ITS sequence of draws cannot be reproduced; the
distributions are the same.
"""
import collections
import math
import os

import numpy as np
import torch

TRAIN_KEYS = ("img_S", "img_F", "mask_S", "mask_F", "lm_F", "lm_S", "gate")
TEST_KEYS = ("img_S", "img_F")
_TABLES = ("images", "masks", "pairs", "pair_lm", "lm", "lm_flip", "gate")
_RAW_TABLES = ("lm_raw", "lm_raw_flip")          # only in a store built with rotation=True


def s2f(file):
    """The frontal file of a MultiPIE file: the fourth `_`-separated field of the name becomes 051 (face_dataset.py:10-17)."""
    name = os.path.split(file)[1]
    ss = name.split("_")
    return "{}_{}_{}_{}_{}".format(ss[0], ss[1], ss[2], "051", ss[4])


def _refuse_aug(aug):
    if aug:
        raise NotImplementedError(
            "the random rotation of --aug is not implemented: its image half is cv2.warpAffine, and without OpenCV there is nothing to "
            "check a kernel against (rotation=True gives the stated fixed-point algorithm, which no OpenCV has confirmed)")


# ---------------------------------------------------------------------- the rotation of --aug, stated (see the module's text)
MAX_ANGLES = 64                    # angle slots of one table set (ffwm_face_batch_aug's A)
_ROTATIONS_KEPT = 8                # table sets a store keeps for FaceStore.rotation(lo, hi)
RotationTables = collections.namedtuple("RotationTables", "adelta bdelta X0 Y0 matrix")


def rotation_tables(angle, W, H):
    """The four integer tables (int64: adelta, bdelta [W]; X0, Y0 [H]) of warpAffine(img, getRotationMatrix2D((W // 2, H // 2), angle,
    1), (W, H)) and the inverted matrix [M0 .. M5] they come from, in Python floats and in OpenCV's order of operations.  These are
    the only floating-point operations of the image half.  rint is round half to even, as cvRound."""
    a = angle * math.pi / 180.0
    alpha, beta = math.cos(a), math.sin(a)
    cx, cy = W // 2, H // 2
    M = [alpha, beta, (1 - alpha) * cx - beta * cy, -beta, alpha, beta * cx + (1 - alpha) * cy]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1, b2 = -M[0] * M[2] - M[1] * M[5], -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    as_int = lambda v: np.rint(v).astype(np.int64)          # noqa: E731
    return RotationTables(as_int(M[0] * x * 1024), as_int(M[3] * x * 1024), as_int((M[1] * y + M[2]) * 1024) + 16,
                          as_int((M[4] * y + M[5]) * 1024) + 16, M)


def warp_affine_linear(array, tables):
    """The integer sums S (int64, the shape of `array`) of warpAffine's bilinear path over an integer array [H, W] or [H, W, C] with a
    constant border of 0: X = (X0[y] + adelta[x]) >> 5, Y likewise; taps at (Y >> 5, X >> 5) and its right / lower neighbours under
    the weights (32 - fx)(32 - fy), fx (32 - fy), (32 - fx) fy, fx fy of fx = X & 31, fy = Y & 31.  The float32 result is S / 1024."""
    array = np.asarray(array)
    H, W = array.shape[:2]
    if tables.adelta.shape != (W,) or tables.X0.shape != (H,):
        raise ValueError("the tables are for %d x %d, the array is %d x %d" % (tables.X0.shape[0], tables.adelta.shape[0], H, W))
    src = array.astype(np.int64)
    X = (tables.X0[:, None] + tables.adelta[None, :]) >> 5
    Y = (tables.Y0[:, None] + tables.bdelta[None, :]) >> 5
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    S = np.zeros(array.shape, dtype=np.int64)
    for dy, dx, w in ((0, 0, (32 - fx) * (32 - fy)), (0, 1, fx * (32 - fy)), (1, 0, (32 - fx) * fy), (1, 1, fx * fy)):
        ty, tx = sy + dy, sx + dx
        w = np.where((ty >= 0) & (ty < H) & (tx >= 0) & (tx < W), w, 0)
        tap = src[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)]
        S += tap * (w[..., None] if array.ndim == 3 else w)
    return S


def rotate_landmarks(lm32, angle, load_size, truncate=True):
    """aug_transform's landmark half (face_dataset.py:122-129) on a float32 row [L, 2] (the row after the flip, .astype('float32')):
    about (load_size // 2, load_size // 2) by -angle, clipped to [0, load_size]; then, with `truncate`, what get_train_item makes of
    it: .long() and the clamp to [0, load_size - 1] -> int64.  Every step is an explicit np.float32 operation with cos and sin
    rounded to float32 first: that is what the reference's lines give under numpy 1.x's value-based casting (a float32 array times
    a float64 SCALAR stays float32), which the reference ran under; numpy 2 would promote to float64, so the installed numpy's
    promotion is not relied on."""
    lm32 = np.asarray(lm32)
    if lm32.dtype != np.float32 or lm32.ndim != 2 or lm32.shape[1] != 2:
        raise ValueError("rotate_landmarks takes a float32 [L, 2] row")
    arc = -angle * np.pi / 180.0
    c, s, h = np.float32(np.cos(arc)), np.float32(np.sin(arc)), np.float32(load_size // 2)
    with np.errstate(over="ignore"):
        x0, y0 = lm32[:, 0] - h, lm32[:, 1] - h
        out = np.stack(((x0 * c - y0 * s) + h, (x0 * s + y0 * c) + h), axis=1)
    assert out.dtype == np.float32
    out = np.minimum(np.maximum(out, np.float32(0)), np.float32(load_size))
    if not truncate:
        return out
    return torch.clamp(torch.from_numpy(out).long(), 0, load_size - 1).numpy()


def _landmark_rows(arr, load_size):
    """One entry of lm_dicts['lm_S' / 'lm_F'] -> (plain, flipped) int32 [L, 2], by the reference's own calls (face_dataset.py:66-67, 82-85)."""
    arr = np.asarray(arr).copy()
    if arr.ndim != 2 or arr.shape[1] != 2:
        raise ValueError("a landmark entry must be [L, 2], got %s" % (arr.shape,))
    flipped = np.hstack((127 - arr[:, 0:1], arr[:, 1:2]))
    return tuple(torch.clamp(torch.from_numpy(np.ascontiguousarray(a)).long(), 0, load_size - 1).to(torch.int32) for a in (arr, flipped))


def _landmark_raw(arr):
    """The same entry -> (plain, flipped) float32 [L, 2] as aug_transform receives them: the flip in the row's own dtype (face_dataset.py:66),
    then .astype('float32') (:122)."""
    arr = np.asarray(arr).copy()
    flipped = np.hstack((127 - arr[:, 0:1], arr[:, 1:2]))
    with np.errstate(over="ignore"):
        rows = tuple(torch.from_numpy(np.ascontiguousarray(a.astype("float32"))) for a in (arr, flipped))
    if not all(bool(torch.isfinite(r).all()) for r in rows):
        raise ValueError("a landmark that is not finite in float32 cannot be rotated")
    return rows


class FaceBatch(dict):
    """A batch: a dict of exactly the tensors trainer.synthetic_batch makes (what FFWMTrainer / FlowNetTrainer .step and .capture take
    -- capture clones every value, so the dict holds tensors only), with the rest as attributes:
      .input_path    the file of S per sample (the reference's batch["input_path"]), from the host copy of the permutation
      .batch_weight  the samples in this batch: the w of train_ffwm.py's sum_loss
      .invalid       int32 [B] on the device, 1 where an index was out of range (never, from a FaceLoader)"""

    def __init__(self, tensors, input_path, batch_weight, invalid=None):
        dict.__init__(self, tensors)
        self.input_path, self.batch_weight, self.invalid = input_path, batch_weight, invalid


class FaceRotation(object):
    """The tables of the integer angles [lo, hi) for W x H images, on one device, as ffwm_face_batch_aug reads them: xtab int32
    [A, 2, W] (adelta, bdelta), ytab int32 [A, 2, H] (X0, Y0), cs float32 [A, 2] (cos and sin of -angle, rounded to float32 as
    rotate_landmarks rounds them); A = hi - lo <= MAX_ANGLES.  Angle `a` has slot a - lo."""

    def __init__(self, lo, hi, W, H, load_size, device="cpu"):
        lo, hi = int(lo), int(hi)
        if not 1 <= hi - lo <= MAX_ANGLES:
            raise ValueError("a rotation range holds 1 to %d whole angles, got [%d, %d)" % (MAX_ANGLES, lo, hi))
        self.lo, self.hi, self.W, self.H, self.load_size, self.device = lo, hi, int(W), int(H), int(load_size), torch.device(device)
        tabs = [rotation_tables(a, W, H) for a in range(lo, hi)]
        arcs = [-a * np.pi / 180.0 for a in range(lo, hi)]
        as_i32 = lambda rows: torch.from_numpy(np.stack(rows).astype(np.int32))          # noqa: E731 (|entry| < 2^25 up to 8192 px)
        self.xtab = as_i32([np.stack((t.adelta, t.bdelta)) for t in tabs]).to(self.device)
        self.ytab = as_i32([np.stack((t.X0, t.Y0)) for t in tabs]).to(self.device)
        self.cs = torch.from_numpy(np.array([[np.cos(a), np.sin(a)] for a in arcs]).astype(np.float32)).to(self.device)

    def slots(self, angles):
        """angles (whole degrees, a list or a tensor on the host) -> int32 slots on the host."""
        angles = torch.as_tensor(angles).to(torch.int64)
        if angles.numel() and not (int(angles.min()) >= self.lo and int(angles.max()) < self.hi):
            raise ValueError("an angle outside [%d, %d)" % (self.lo, self.hi))
        return (angles - self.lo).to(torch.int32)


class FaceStore(object):
    """The preloaded set as tensors on one device (see the module's text).  Build it with from_arrays / from_directory / load."""

    def __init__(self, tensors, names, isval, datamode, load_size, gallery_names, host=None):
        self.t = tensors                      # images, masks, pairs, pair_lm, lm, lm_flip, gate (None where the mode has none)
        self._rotations = {}                  # (lo, hi) -> FaceRotation on this store's device
        self.names = list(names)
        self.isval, self.datamode, self.load_size = bool(isval), datamode, int(load_size)
        self.gallery_names = list(gallery_names) if gallery_names is not None else None
        self.host = host if host is not None else self          # the CPU store behind a device store: host_item, names, the gallery's rows
        self.device = tensors["images"].device

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_arrays(cls, images, masks, names, lm_dicts=None, datamode="multipie", isval=False, load_size=128, gallery_list=None,
                    aug=False, rotation=False):
        """images uint8 [N, H, W, 3] (RGB) and masks uint8 [N, H, W] or [N, H, W, 1] (None for a test set) in the order of `names`
        (the reference's self.files); lm_dicts = {"lm_S": {key: [L, 2]}, "lm_F": {...}, "gate": {key: [L]}} (landmarks.npy) for a
        training set.  gallery_list: the names of gallery_list.npy, or None for the reference's rule (multipie test sets only).
        rotation: a training store also keeps lm_raw / lm_raw_flip float32 [K, L, 2], the plain and the flipped landmark rows before
        .long(), row for row beside lm / lm_flip: what the rotation of --aug starts from (a landmark that is not finite is refused)."""
        _refuse_aug(aug)
        if rotation and isval:
            raise ValueError("only a training set is rotated")
        images = torch.as_tensor(np.asarray(images) if not torch.is_tensor(images) else images)
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
            raise ValueError("images must be uint8 [N, H, W, 3], got %s %s" % (images.dtype, tuple(images.shape)))
        images = images.contiguous().cpu()
        N, H, W, _ = images.shape
        names = [str(n) for n in names]
        if len(names) != N or len(set(names)) != N:
            raise ValueError("need one distinct name per image (%d names, %d images)" % (len(names), N))
        row = {n: i for i, n in enumerate(names)}
        if datamode == "multipie":
            missing = [n for n in names if s2f(n) not in row]
            if missing:
                raise KeyError("no frontal file %s for %s (%d such files)" % (s2f(missing[0]), missing[0], len(missing)))
            pairs = [(i, row[s2f(n)]) for i, n in enumerate(names)]
        else:
            pairs = [(i, i) for i in range(N)]
        t = dict.fromkeys(_TABLES)
        t["images"] = images
        t["pairs"] = torch.tensor(pairs, dtype=torch.int32).view(-1, 2)
        if not isval:
            if masks is None or lm_dicts is None:
                raise ValueError("a training set needs masks and lm_dicts")
            masks = torch.as_tensor(np.asarray(masks) if not torch.is_tensor(masks) else masks)
            if masks.dim() == 4 and masks.shape[3] == 1:
                masks = masks[..., 0]
            if masks.dtype != torch.uint8 or tuple(masks.shape) != (N, H, W):
                raise ValueError("masks must be uint8 [%d, %d, %d], got %s %s" % (N, H, W, masks.dtype, tuple(masks.shape)))
            t["masks"] = masks.contiguous().cpu()
            lm_rows, gate_rows, plain, flipped, gates, pair_lm, raw = {}, {}, [], [], [], [], []
            for s, f in pairs:
                ks = []
                for which, key in (("lm_S", names[s][:-7]), ("lm_F", names[f][:-7])):
                    if (which, key) not in lm_rows:
                        a, b = _landmark_rows(lm_dicts[which][key], load_size)
                        lm_rows[(which, key)] = len(plain)
                        plain.append(a)
                        flipped.append(b)
                        if rotation:
                            raw.append(_landmark_raw(lm_dicts[which][key]))
                    ks.append(lm_rows[(which, key)])
                key = names[s][:-7]
                if key not in gate_rows:
                    gate_rows[key] = len(gates)
                    gates.append(torch.from_numpy(np.asarray(lm_dicts["gate"][key]).copy().astype("float32")).reshape(-1))
                pair_lm.append(ks + [gate_rows[key]])
            L = plain[0].shape[0]
            if any(a.shape[0] != L for a in plain) or any(g.shape[0] != L for g in gates):
                raise ValueError("every landmark and gate entry must have the same number of landmarks (the default collate needs it too)")
            t["lm"], t["lm_flip"], t["gate"] = torch.stack(plain), torch.stack(flipped), torch.stack(gates)
            t["pair_lm"] = torch.tensor(pair_lm, dtype=torch.int32).view(-1, 3)
            if rotation:
                t["lm_raw"], t["lm_raw_flip"] = torch.stack([r[0] for r in raw]), torch.stack([r[1] for r in raw])
        gallery = None
        if isval and datamode == "multipie":
            if gallery_list is not None:
                gallery = [str(g) for g in gallery_list]
            else:
                first = {}
                for k in names:
                    if k[:3] not in first and k.strip().endswith("051_06.png"):
                        first[k[:3]] = k
                gallery = list(first.values())
            missing = [g for g in gallery if g not in row]
            if missing:
                raise KeyError("gallery file %s is not among the images" % missing[0])
        return cls(t, names, isval, datamode, load_size, gallery)

    @classmethod
    def from_directory(cls, dataroot, datamode="multipie", isval=False, load_size=128, threads=8, aug=False, rotation=False):
        """<dataroot>/<datamode>/{train,test}/ (multipie) or <dataroot>/<datamode>/ (other modes) with images/, masks/ and landmarks.npy
        for a training set, images/ and an optional gallery_list.npy for a test set -- read once, with PIL on `threads` threads.
        8-bit RGB images and single-channel 8-bit masks are taken byte for byte; anything else is refused (a mask stored with colour
        channels would need the grey conversion of cv2.imread(path, 0), which cannot be reproduced without OpenCV)."""
        _refuse_aug(aug)
        from concurrent.futures import ThreadPoolExecutor
        from PIL import Image
        base = os.path.join(dataroot, datamode)
        if datamode == "multipie":
            base = os.path.join(base, "test" if isval else "train")
        names = sorted(os.listdir(os.path.join(base, "images")))

        def read(args):
            folder, name, mode = args
            with Image.open(os.path.join(base, folder, name)) as im:
                if im.mode != mode:
                    raise ValueError("%s/%s is stored as PIL mode %r; only 8-bit %s files are read (byte for byte)" % (
                        folder, name, im.mode, "RGB" if mode == "RGB" else "single-channel"))
                return np.asarray(im, dtype=np.uint8)

        def read_all(folder, mode):
            with ThreadPoolExecutor(max_workers=max(1, int(threads))) as ex:
                arrs = list(ex.map(read, [(folder, n, mode) for n in names]))
            if any(a.shape != arrs[0].shape for a in arrs):
                raise ValueError("the files of %s/ differ in size" % folder)
            return np.stack(arrs)

        images = read_all("images", "RGB")
        masks = lm_dicts = gallery_list = None
        if not isval:
            masks = read_all("masks", "L")
            lm_dicts = np.load(os.path.join(base, "landmarks.npy"), allow_pickle=True).item()
        elif os.path.exists(os.path.join(base, "gallery_list.npy")):
            gallery_list = [str(g) for g in np.load(os.path.join(base, "gallery_list.npy"))]
        return cls.from_arrays(images, masks, names, lm_dicts, datamode, isval, load_size, gallery_list, rotation=rotation)

    def save(self, path):
        """The store as one uncompressed .npz (the tables as they are: load() needs no landmarks.npy and converts nothing again; the
        raw landmark tables of rotation=True go with it when the store has them)."""
        h = self.host
        arrays = {k: v.numpy() for k, v in h.t.items() if v is not None}
        arrays["names"] = np.array(h.names)
        arrays["gallery_names"] = np.array(h.gallery_names if h.gallery_names is not None else [], dtype=str)
        arrays["meta"] = np.array([str(int(h.isval)), h.datamode, str(h.load_size), str(int(h.gallery_names is not None))])
        np.savez(path, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            t = {k: (torch.from_numpy(z[k]) if k in z.files else None) for k in _TABLES}
            t.update({k: torch.from_numpy(z[k]) for k in _RAW_TABLES if k in z.files})          # (a file without them cannot rotate)
            meta = [str(m) for m in z["meta"]]
            gallery = [str(g) for g in z["gallery_names"]] if meta[3] == "1" else None
            return cls(t, [str(n) for n in z["names"]], meta[0] == "1", meta[1], int(meta[2]), gallery)

    def to(self, device):
        """The store with its tensors on `device` (uploaded once); the CPU store stays behind it as .host."""
        device = torch.device(device)
        if device == self.device:
            return self
        if device.type == "cpu":
            return self.host
        h = self.host
        return FaceStore({k: (v.to(device) if v is not None else None) for k, v in h.t.items()}, h.names, h.isval, h.datamode,
                         h.load_size, h.gallery_names, host=h)

    # ------------------------------------------------------------------ the reference's dataset
    @property
    def pairs(self):
        """[(path_S, path_F)] as the reference's self.pairs."""
        return [(self.names[s], self.names[f]) for s, f in self.host.t["pairs"].tolist()]

    @property
    def n_pairs(self):
        return self.t["pairs"].shape[0]

    def __len__(self):
        return self.n_pairs if self.isval else 2 * self.n_pairs

    def nbytes(self):
        return sum(v.numel() * v.element_size() for v in self.t.values() if v is not None)

    @property
    def can_rotate(self):
        """A training store built with rotation=True (or loaded from the file of one)."""
        return not self.isval and self.t.get("lm_raw") is not None and self.t.get("lm_raw_flip") is not None

    def _need_rotation(self):
        if not self.can_rotate:
            raise ValueError("the rotation needs a training store built with rotation=True (the raw landmark tables lm_raw / lm_raw_flip)")

    def rotation(self, lo, hi):
        """The FaceRotation of the angles [lo, hi) on this store's device, built and uploaded on first use.  The store keeps the
        last _ROTATIONS_KEPT ranges it was asked for (a loader holds its own): callers that ask for ever new ranges, as
        batch(angle=...) may, do not pile up tables on the device."""
        self._need_rotation()
        if (lo, hi) not in self._rotations:
            _, H, W, _ = self.t["images"].shape
            while len(self._rotations) >= _ROTATIONS_KEPT:
                del self._rotations[next(iter(self._rotations))]          # (the oldest: a dict keeps insertion order)
            self._rotations[(lo, hi)] = FaceRotation(lo, hi, W, H, self.load_size, self.device)
        return self._rotations[(lo, hi)]

    def host_item(self, index, angle=None):
        """Item `index` on the CPU, step by step as get_test_item / get_train_item compute it (face_dataset.py:37-90); with an integer
        `angle` (degrees) the item after aug_transform (:73-75, 110-130) as the module's text states it: img_S, mask_S and lm_S change."""
        h = self.host
        P = h.n_pairs
        if not 0 <= index < len(h):
            raise IndexError("item %d of %d" % (index, len(h)))
        if angle is not None:
            h._need_rotation()
            if angle != int(angle):
                raise ValueError("the reference rotates by whole degrees (np.random.randint), got %r" % (angle,))
            angle = int(angle)
        _index = index % P if index >= P else index
        s, f = h.t["pairs"][_index].tolist()
        images = h.t["images"].numpy()
        img_S, img_F = images[s].copy().astype("float32"), images[f].copy().astype("float32")
        if h.isval:
            return {"img_S": torch.from_numpy(img_S.transpose((2, 0, 1)).astype("float32")).div(255),
                    "img_F": torch.from_numpy(img_F.transpose((2, 0, 1)).astype("float32")).div(255), "input_path": h.names[s]}
        masks = h.t["masks"].numpy()
        mask_S, mask_F = masks[s][:, :, np.newaxis].copy().astype("float32"), masks[f][:, :, np.newaxis].copy().astype("float32")
        rs, rf, rg = h.t["pair_lm"][_index].tolist()
        table, raw = h.t["lm"], h.t.get("lm_raw")
        if index >= P:
            table, raw = h.t["lm_flip"], h.t.get("lm_raw_flip")
            img_S, img_F, mask_S, mask_F = img_S[:, ::-1, :], img_F[:, ::-1, :], mask_S[:, ::-1, :], mask_F[:, ::-1, :]
        lm_S = table[rs].long()
        if angle is not None:
            H, W, _ = img_S.shape
            tables = rotation_tables(angle, W, H)
            img_S = (warp_affine_linear(img_S.astype(np.int64), tables) / 1024.0).astype("float32")          # (S / 1024 is exact)
            mask_S = warp_affine_linear(mask_S.astype(np.int64), tables)
            mask_S = np.where(mask_S > 0, np.float32(255), np.float32(0))                                     # mask_aug[mask_aug > 0] = 255
            lm_S = torch.from_numpy(rotate_landmarks(raw[rs].numpy(), angle, h.load_size))
        item = {k: torch.from_numpy(v.transpose((2, 0, 1)).astype("float32")).div(255)
                for k, v in (("img_S", img_S), ("img_F", img_F), ("mask_S", mask_S), ("mask_F", mask_F))}
        item.update({"input_path": h.names[s], "lm_S": lm_S, "lm_F": table[rf].long(), "gate": h.t["gate"][rg].clone().unsqueeze(1)})
        return item

    def host_batch(self, indices, angles=None):
        """The default collate of host_item over `indices` (with one integer angle per item, or none): {key: [B, ...]} plus
        "input_path" as a list -- what one step of the reference's DataLoader hands out."""
        if angles is not None and len(angles) != len(indices):
            raise ValueError("need one angle per index")
        items = [self.host_item(int(i), None if angles is None else angles[j]) for j, i in enumerate(indices)]
        batch = {k: torch.stack([it[k] for it in items]) for k in items[0] if k != "input_path"}
        batch["input_path"] = [it["input_path"] for it in items]
        return batch

    def batch(self, index, out=None, angle=None):
        """-> the tensors of the batch of `index` (int32 [B] on the store's device; a list on a CPU store) plus "invalid": one launch of
        ops.face_batch on a device store, host_batch on a CPU store.  `out`: destinations written in place.  angle: one integer
        angle per sample ON THE HOST (a list or a CPU tensor): the rotated batch -- on a device store through the tables of
        rotation(min, max + 1) and an upload of the slots (batch_rotated is the form without host work)."""
        as_list = lambda v: v.tolist() if torch.is_tensor(v) else list(v)          # noqa: E731
        if angle is not None:
            angle = as_list(angle)
            if any(a != int(a) for a in angle):
                raise ValueError("the reference rotates by whole degrees (np.random.randint)")
        if self.device.type == "cuda":
            from . import ops
            t = self.t
            if angle is not None:
                rot = self.rotation(int(min(angle)), int(max(angle)) + 1)
                return self.batch_rotated(index, rot.slots(angle).to(self.device), rot, out=out)
            if self.isval:
                return ops.face_batch(t["images"], t["pairs"], index, out=out)
            return ops.face_batch(t["images"], t["pairs"], index, t["masks"], t["pair_lm"], t["lm"], t["lm_flip"], t["gate"], out=out)
        idx = as_list(index)
        res = self.host_batch(idx, angle)
        del res["input_path"]
        res["invalid"] = torch.zeros(len(idx), dtype=torch.int32)
        if out is not None:
            for k, v in res.items():
                if out.get(k) is not None:
                    res[k] = out[k].copy_(v)
        return res

    def batch_rotated(self, index, slot, rotation, out=None):
        """The rotated batch of `index` under the angle slots `slot` (int32 [B], angle - rotation.lo), both on the store's device,
        in ONE launch of ops.face_batch_aug: no host work, no copy, no synchronisation (a captured launch follows both vectors).  A
        slot outside [0, hi - lo) gives zeros and invalid[b] = 1, as an index out of range does.  On a CPU store: host_batch."""
        self._need_rotation()
        if rotation.device != self.device or (rotation.H, rotation.W) != tuple(self.t["images"].shape[1:3]) \
                or rotation.load_size != self.load_size:
            raise ValueError("the rotation tables belong to another device, image size or load_size")
        if self.device.type != "cuda":
            slots = slot.tolist() if torch.is_tensor(slot) else list(slot)
            return self.batch(index, out=out, angle=[rotation.lo + int(s) for s in slots])
        from . import ops
        t = self.t
        return ops.face_batch_aug(t["images"], t["pairs"], index, t["masks"], t["pair_lm"], t["lm"], t["lm_flip"], t["gate"], t["lm_raw"],
                                  t["lm_raw_flip"], slot, rotation.xtab, rotation.ytab, rotation.cs, rotation.load_size, out=out)

    # ------------------------------------------------------------------ the gallery
    def gallery_rows(self):
        if self.gallery_names is None:
            raise ValueError("only a multipie test set has a gallery")
        row = {n: i for i, n in enumerate(self.names)}
        return [row[g] for g in self.gallery_names]

    def host_gallery(self):
        """-> (ids, planes [G, 1, H, W]) as get_gallery builds gallery_dict (face_dataset.py:153-168): id = name[:3] (a later entry of
        one id replaces an earlier one, as in the dict), plane = torch.mean over the channels of byte / 255."""
        images = self.host.t["images"].numpy()
        planes = {}
        for g, r in zip(self.gallery_names, self.gallery_rows()):
            gallery = torch.from_numpy(images[r].copy().astype("float32").transpose((2, 0, 1)).astype("float32")).div(255)
            planes[g[:3]] = torch.mean(gallery, (0, ), keepdim=True)
        return list(planes), torch.stack(list(planes.values()))

    def gallery(self):
        """-> (ids, planes [G, 1, H, W] on the store's device): one launch on a device store (FaceIdentifier.set_gallery takes the planes)."""
        if self.device.type != "cuda":
            return self.host_gallery()
        from . import _lib, ops
        rows = {}
        for g, r in zip(self.gallery_names, self.gallery_rows()):
            rows[g[:3]] = r
        N, H, W, _ = self.t["images"].shape
        index = torch.tensor(list(rows.values()), dtype=torch.int32).to(self.device)
        out = torch.empty((len(rows), 1, H, W), dtype=torch.float32, device=self.device)
        if len(rows):
            with ops._on_device(out) as stream:
                _lib.check(_lib.load().ffwm_face_gallery(self.t["images"].data_ptr(), index.data_ptr(), out.data_ptr(), N, H, W, len(rows),
                                                         stream), "ffwm_face_gallery")
        return list(rows), out


class FaceLoader(object):
    """The reference's DataLoader over a FaceStore (data/__init__.py:77-87: shuffle=True for training, sequential for a test set,
    drop_last=False): iterating yields one FaceBatch per step.

    The permutation of epoch e is torch.randperm under a generator seeded with seed + e, drawn on the host and uploaded once per epoch;
    a step is one launch on a slice of it.  `out`: a dict of preallocated tensors [batch_size, ...] (a trainer's static inputs, say)
    that every full batch is written into -- the trainers' `b[k] is v` test then skips their copy; without it the loader alternates
    between two buffer sets of its own, so a batch stays intact while the next one is assembled, and is overwritten by the one after.
    A short last batch is written into the leading rows of its buffers.

    rotation: True for the reference's --aug, np.random.randint(-5, 5), or (lo, hi) for the half-open range of whole angles of
    np.random.randint(lo, hi), hi - lo <= 64; the store must have been built with rotation=True.  Epoch e then draws, under the ONE
    generator seeded with seed + e, first the permutation (the very call a loader without rotation makes, so the item order is the
    same) and then torch.randint(lo, hi, (n,)): one angle per position of the epoch.  The tables of the range go to the device
    once per loader, the epoch's angle slots once per epoch beside the index; a step is one launch of ffwm_face_batch_aug on
    slices of both.  The reference draws from numpy's global state inside its workers, so its own sequence of angles cannot be
    reproduced; the distribution is the same."""

    def __init__(self, store, batch_size, shuffle=None, drop_last=False, seed=0, out=None, aug=False, rotation=None):
        _refuse_aug(aug)
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        self.store, self.batch_size, self.drop_last, self.seed = store, int(batch_size), bool(drop_last), int(seed)
        self.shuffle = (not store.isval) if shuffle is None else bool(shuffle)
        self.epoch = 0
        self.out = out
        self._sets = [dict(out)] if out is not None else None          # (a copy: the loader adds its `invalid` buffer to it)
        self.rotation = None
        if rotation is not None and rotation is not False:
            lo, hi = (-5, 5) if rotation is True else (int(rotation[0]), int(rotation[1]))
            if not 1 <= hi - lo <= MAX_ANGLES:
                raise ValueError("rotation=(lo, hi) is the range of np.random.randint(lo, hi) with 1 <= hi - lo <= %d" % MAX_ANGLES)
            self.rotation = store.rotation(lo, hi)          # (ValueError for a test store or one without the raw tables)

    def __len__(self):
        n, B = len(self.store), self.batch_size
        return n // B if self.drop_last else (n + B - 1) // B

    def draws(self, epoch):
        """-> (permutation int32 [n], angles int64 [n] or None without rotation) of `epoch`, on the host: position i of the epoch
        shows item permutation[i] rotated by angles[i] degrees."""
        n = len(self.store)
        g = torch.Generator().manual_seed(self.seed + epoch)
        perm = torch.randperm(n, generator=g).to(torch.int32) if self.shuffle else torch.arange(n, dtype=torch.int32)
        if self.rotation is None:
            return perm, None
        return perm, torch.randint(self.rotation.lo, self.rotation.hi, (n,), generator=g)

    def permutation(self, epoch):
        """The item order of `epoch` as an int32 tensor on the host."""
        return self.draws(epoch)[0]

    def _destinations(self, step, b):
        if self.store.device.type != "cuda":
            return self.out if (self.out is None or b == self.batch_size) else {k: v[:b] for k, v in self.out.items()}
        if self._sets is None:
            self._sets = [{}, {}]
        dst = self._sets[step % len(self._sets)]
        return dst if b == self.batch_size else {k: v[:b] for k, v in dst.items()}

    def __iter__(self):
        store, B = self.store, self.batch_size
        rot = self.rotation
        perm, angles = self.draws(self.epoch)
        self.epoch += 1
        index = perm.to(store.device)          # the one upload of the epoch (two with rotation: the angle slots)
        slot = rot.slots(angles).to(store.device) if rot is not None else None
        order = perm.tolist()
        names = store.host.names
        rows_S = store.host.t["pairs"][:, 0].tolist()
        P, n = store.n_pairs, len(store)
        for step in range(len(self)):
            lo, hi = step * B, min(n, step * B + B)
            dst = self._destinations(step, hi - lo)
            res = store.batch(index[lo:hi], out=dst) if rot is None else store.batch_rotated(index[lo:hi], slot[lo:hi], rot, out=dst)
            if store.device.type == "cuda" and hi - lo == B:
                self._sets[step % len(self._sets)].update(res)          # buffers the first full batch allocated are kept
            invalid = res.pop("invalid")
            yield FaceBatch(res, [names[rows_S[i % P]] for i in order[lo:hi]], hi - lo, invalid)


# ====================================================================== LightCNN fine-tuning: lightcnn/dataset.py
CROP_ROWS, CROP_COLS = slice(28, -2), slice(15, -15)          # dataset.py:64


def rotation_matrix(angle, w, h):
    """The inverse-map matrix [m0 .. m5] of Image.rotate(angle) (degrees, counter-clockwise, about the centre, expand=False) for a
    w x h image, in Python floats with the math module, as PIL builds it."""
    a = -math.radians(angle % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def _cubic(v1, v2, v3, v4, d):
    """The a = -1 cubic through four taps at fraction d, in PIL's operation order."""
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def rotate_bicubic(image, matrix):
    """Image.transform(size, AFFINE, matrix, BICUBIC) of a uint8 [H, W, 3] array, restated in float64 (numpy rounds every product
    and sum on its own: nothing is contracted): xin = m0 (x + .5) + m1 (y + .5) + m2, yin likewise; outside [0, W) x [0, H) the
    pixel is 0; else the cubic over 4 x 4 index-clamped taps around (xin - .5, yin - .5), rows first, clipped to [0, 255] and
    TRUNCATED to a byte.  Image.rotate(angle, BICUBIC) is this under rotation_matrix(angle, W, H)."""
    image = np.asarray(image)
    H, W, _ = image.shape
    m = [float(v) for v in matrix]
    xs, ys = (np.arange(W, dtype=np.float64) + 0.5)[None, :], (np.arange(H, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        xin = m[0] * xs + m[1] * ys + m[2]
        yin = m[3] * xs + m[4] * ys + m[5]
        inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)          # made before any conversion to an integer
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    fx, fy = np.floor(xin), np.floor(yin)
    dx, dy = (xin - fx)[..., None], (yin - fy)[..., None]
    x0, y0 = fx.astype(np.int64) - 1, fy.astype(np.int64) - 1
    xi = [np.clip(x0 + k, 0, W - 1) for k in range(4)]
    yi = [np.clip(y0 + k, 0, H - 1) for k in range(4)]
    src = image.astype(np.float64)
    rows = [_cubic(src[yi[j], xi[0]], src[yi[j], xi[1]], src[yi[j], xi[2]], src[yi[j], xi[3]], dx) for j in range(4)]
    v = _cubic(rows[0], rows[1], rows[2], rows[3], dy)
    out = np.where(v <= 0.0, 0.0, np.where(v >= 255.0, 255.0, v)).astype(np.uint8)
    out[~inside] = 0
    return out


def _identity_targets(names):
    """finetune.py:146-148 (LightCNNTrainer.targets_from_names): the class of an image is the number its name begins with, from 1."""
    try:
        return torch.tensor([int(os.path.basename(n)[:3]) - 1 for n in names], dtype=torch.int64)
    except ValueError:
        raise ValueError("every file name must begin with its three-digit identity (finetune.py:147 reads int(name[:3]))")


class IdentityBatch(dict):
    """A batch of LightCNN fine-tuning: {"img": [B, 1, H, W] or [B, 1, 128, 128], "target": int64 [B]} -- what LightCNNTrainer.step
    and .capture take -- with .input_path, .batch_weight and .invalid as FaceBatch has them."""

    def __init__(self, tensors, input_path, batch_weight, invalid=None):
        dict.__init__(self, tensors)
        self.input_path, self.batch_weight, self.invalid = input_path, batch_weight, invalid


class IdentityStore(object):
    """The preloaded set of lightcnn/dataset.py's ImgDataset as tensors on one device: images uint8 [N, H, W, 3], targets int64 [N]
    (see the module's text).  Build it with from_arrays / from_directory / from_face_store / load."""

    def __init__(self, tensors, names, isval, gallery_names, host=None):
        self.t = tensors                      # images, targets
        self.names = list(names)
        self.isval = bool(isval)
        self.gallery_names = list(gallery_names) if gallery_names is not None else None
        self.host = host if host is not None else self
        self.device = tensors["images"].device

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_arrays(cls, images, names, isval=False, gallery_list=None):
        """images uint8 [N, H, W, 3] (RGB) in the order of `names`.  gallery_list: the names of gallery_list.npy, or None for the
        reference's rule (the first *051_06.png per name[:3]); a training set has no gallery."""
        images = torch.as_tensor(np.asarray(images) if not torch.is_tensor(images) else images)
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
            raise ValueError("images must be uint8 [N, H, W, 3], got %s %s" % (images.dtype, tuple(images.shape)))
        return cls._from_tensor(images.contiguous().cpu(), names, isval, gallery_list)

    @classmethod
    def _from_tensor(cls, images, names, isval, gallery_list):
        names = [str(n) for n in names]
        if len(names) != images.shape[0] or len(set(names)) != len(names):
            raise ValueError("need one distinct name per image (%d names, %d images)" % (len(names), images.shape[0]))
        gallery = None
        if isval:
            if gallery_list is not None:
                gallery = [str(g) for g in gallery_list]
            else:
                first = {}
                for k in names:
                    if k[:3] not in first and k.strip().endswith("051_06.png"):
                        first[k[:3]] = k
                gallery = list(first.values())
            known = set(names)
            missing = [g for g in gallery if g not in known]
            if missing:
                raise KeyError("gallery file %s is not among the images" % missing[0])
        return cls({"images": images, "targets": _identity_targets(names)}, names, isval, gallery)

    @classmethod
    def from_directory(cls, dataroot, isval=False, threads=8):
        """<dataroot>/{train,test}/images (and an optional gallery_list.npy beside a test set's images/), read once with PIL on
        `threads` threads, the names sorted.  8-bit RGB files are taken byte for byte; anything else is refused."""
        from concurrent.futures import ThreadPoolExecutor
        from PIL import Image
        base = os.path.join(dataroot, "test" if isval else "train")
        names = sorted(os.listdir(os.path.join(base, "images")))

        def read(name):
            with Image.open(os.path.join(base, "images", name)) as im:
                if im.mode != "RGB":
                    raise ValueError("images/%s is stored as PIL mode %r; only 8-bit RGB files are read (byte for byte)" % (name, im.mode))
                return np.asarray(im, dtype=np.uint8)

        with ThreadPoolExecutor(max_workers=max(1, int(threads))) as ex:
            arrs = list(ex.map(read, names))
        if any(a.shape != arrs[0].shape for a in arrs):
            raise ValueError("the files of images/ differ in size")
        gallery_list = None
        if isval and os.path.exists(os.path.join(base, "gallery_list.npy")):
            gallery_list = [str(g) for g in np.load(os.path.join(base, "gallery_list.npy"))]
        return cls.from_arrays(np.stack(arrs), names, isval, gallery_list)

    @classmethod
    def from_face_store(cls, store):
        """The images of a FaceStore as an IdentityStore on the same device: the image tensors are SHARED, nothing is copied."""
        h = store.host
        host = cls._from_tensor(h.t["images"], h.names, h.isval, h.gallery_names if h.isval else None)
        if store.device.type == "cpu":
            return host
        return cls({"images": store.t["images"], "targets": host.t["targets"].to(store.device)}, host.names, host.isval,
                   host.gallery_names, host=host)

    def save(self, path):
        """The store as one uncompressed .npz."""
        h = self.host
        np.savez(path, images=h.t["images"].numpy(), targets=h.t["targets"].numpy(), names=np.array(h.names),
                 gallery_names=np.array(h.gallery_names if h.gallery_names is not None else [], dtype=str),
                 meta=np.array([str(int(h.isval)), str(int(h.gallery_names is not None))]))

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            meta = [str(m) for m in z["meta"]]
            gallery = [str(g) for g in z["gallery_names"]] if meta[1] == "1" else None
            return cls({"images": torch.from_numpy(z["images"]), "targets": torch.from_numpy(z["targets"])},
                       [str(n) for n in z["names"]], meta[0] == "1", gallery)

    def to(self, device):
        """The store with its tensors on `device` (uploaded once); the CPU store stays behind it as .host."""
        device = torch.device(device)
        if device == self.device:
            return self
        if device.type == "cpu":
            return self.host
        h = self.host
        return IdentityStore({k: v.to(device) for k, v in h.t.items()}, h.names, h.isval, h.gallery_names, host=h)

    def __len__(self):
        return self.t["images"].shape[0]

    def nbytes(self):
        return sum(v.numel() * v.element_size() for v in self.t.values())

    # ------------------------------------------------------------------ the reference's dataset
    def host_item(self, index, angle=None, flip=False, crop=False, matrix=None):
        """Item `index` on the CPU as get_train_item / get_test_item and postprocess compute it (dataset.py:33-67): `angle` (degrees)
        or `matrix` (rotation_matrix's six numbers; it wins over `angle`) and `flip` are the draws of RandomRotation and
        RandomHorizontalFlip; with neither, the test item.  -> {"img": [1, H, W] or [1, 128, 128], "input_path", "target"}."""
        h = self.host
        if not 0 <= index < len(h):
            raise IndexError("item %d of %d" % (index, len(h)))
        img = h.t["images"][index].numpy()
        H, W, _ = img.shape
        if matrix is None and angle is not None:
            matrix = rotation_matrix(float(angle), W, H)
        if matrix is not None:
            img = rotate_bicubic(img, matrix)                  # RandomRotation(5, resample=Image.BICUBIC, expand=False)
        if flip:
            img = img[:, ::-1, :]                              # RandomHorizontalFlip
        img = torch.from_numpy(img.transpose((2, 0, 1)).copy()).float().div(255)          # ToTensor / .float().div(255)
        img = torch.mean(img, dim=(0, ), keepdim=True)
        if crop:
            img = img[:, CROP_ROWS, CROP_COLS]
            img = torch.nn.functional.interpolate(img.unsqueeze(0), (128, 128), mode="bilinear")
            img = img[0]
        return {"img": img, "input_path": h.names[index], "target": h.t["targets"][index].clone()}

    def host_batch(self, indices, angles=None, flips=None, crop=False, matrices=None):
        """The default collate of host_item over `indices` (with one angle or matrix and one flip per item, or none: test items):
        {"img": [B, ...], "target": int64 [B], "input_path": list}."""
        items = [self.host_item(int(i), None if angles is None else float(angles[j]), False if flips is None else bool(flips[j]), crop,
                                None if matrices is None else [float(v) for v in matrices[j]]) for j, i in enumerate(indices)]
        return {"img": torch.stack([it["img"] for it in items]), "target": torch.stack([it["target"] for it in items]),
                "input_path": [it["input_path"] for it in items]}

    def batch(self, index, matrix=None, flip=None, crop=False, out=None):
        """-> {"img", "target", "invalid"} of the batch of `index` (int32 [B]) under `matrix` (float64 [B, 6]) and `flip` (uint8 [B]),
        all on the store's device (lists will do on a CPU store); both None: test items.  One launch of ops.identity_batch on a
        device store, host_batch on a CPU store.  `out`: destinations written in place."""
        if self.device.type == "cuda":
            from . import ops
            return ops.identity_batch(self.t["images"], self.t["targets"], index, matrix, flip, crop=crop, out=out)
        as_list = lambda v: v.tolist() if torch.is_tensor(v) else (None if v is None else list(v))          # noqa: E731
        idx = as_list(index)
        res = self.host_batch(idx, None, as_list(flip), crop, as_list(matrix))
        del res["input_path"]
        res["invalid"] = torch.zeros(len(idx), dtype=torch.int32)
        if out is not None:
            for k, v in res.items():
                if out.get(k) is not None:
                    res[k] = out[k].copy_(v)
        return res

    # ------------------------------------------------------------------ the gallery (as FaceStore has it)
    def gallery_rows(self):
        if self.gallery_names is None:
            raise ValueError("only a test set has a gallery")
        row = {n: i for i, n in enumerate(self.names)}
        return [row[g] for g in self.gallery_names]

    host_gallery = FaceStore.host_gallery
    gallery = FaceStore.gallery


class IdentityLoader(object):
    """The reference's DataLoader over an IdentityStore (finetune.py:98-106: shuffle=True for training, sequential for validation,
    drop_last=False): iterating yields one IdentityBatch per step.

    Epoch e draws, under ONE generator seeded with seed + e and in this order, the permutation (torch.randperm), the angles (float64,
    uniform in [-degrees, degrees]: RandomRotation(degrees)) and the flips (probability 0.5), one angle and one flip per position of
    the epoch.  The reference draws both from Python's global `random` inside its loader workers, so its own sequence cannot be
    reproduced; the distributions are the same.  The matrices are built on the host (rotation_matrix); index, matrices and flips are
    uploaded once per epoch and a step is one launch on slices of them.  A validation store yields un-augmented batches.  `out` and
    the two alternating buffer sets work as FaceLoader's do; a short last batch is written into the leading rows of its buffers."""

    def __init__(self, store, batch_size, crop=False, shuffle=None, drop_last=False, seed=0, out=None, degrees=5.0):
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        if not degrees >= 0:
            raise ValueError("degrees must not be negative")
        self.store, self.batch_size, self.crop, self.drop_last = store, int(batch_size), bool(crop), bool(drop_last)
        self.seed, self.degrees = int(seed), float(degrees)
        self.shuffle = (not store.isval) if shuffle is None else bool(shuffle)
        self.augment = not store.isval
        self.epoch = 0
        self.out = out
        self._sets = [dict(out)] if out is not None else None

    def __len__(self):
        n, B = len(self.store), self.batch_size
        return n // B if self.drop_last else (n + B - 1) // B

    def draws(self, epoch):
        """-> (permutation int32 [n], angles float64 [n], flips uint8 [n]) of `epoch`, on the host; position i of the epoch shows item
        permutation[i] rotated by angles[i] and mirrored where flips[i] (a validation store: angles and flips are None)."""
        n = len(self.store)
        g = torch.Generator().manual_seed(self.seed + epoch)
        perm = torch.randperm(n, generator=g).to(torch.int32) if self.shuffle else torch.arange(n, dtype=torch.int32)
        if not self.augment:
            return perm, None, None
        angles = (torch.rand(n, dtype=torch.float64, generator=g) * 2.0 - 1.0) * self.degrees
        flips = (torch.rand(n, generator=g) < 0.5).to(torch.uint8)
        return perm, angles, flips

    def permutation(self, epoch):
        return self.draws(epoch)[0]

    def matrices(self, angles):
        """float64 [n, 6]: rotation_matrix of every angle for the store's image size."""
        _, H, W, _ = self.store.t["images"].shape
        return torch.tensor([rotation_matrix(a, W, H) for a in angles.tolist()], dtype=torch.float64).view(-1, 6)

    def _destinations(self, step, b):
        if self.store.device.type != "cuda":
            return self.out if (self.out is None or b == self.batch_size) else {k: v[:b] for k, v in self.out.items()}
        if self._sets is None:
            self._sets = [{}, {}]
        dst = self._sets[step % len(self._sets)]
        return dst if b == self.batch_size else {k: v[:b] for k, v in dst.items()}

    def __iter__(self):
        store, B = self.store, self.batch_size
        perm, angles, flips = self.draws(self.epoch)
        self.epoch += 1
        index = perm.to(store.device)          # the uploads of the epoch
        matrix = self.matrices(angles).to(store.device) if self.augment else None
        flip = flips.to(store.device) if self.augment else None
        order = perm.tolist()
        names = store.host.names
        n = len(store)
        for step in range(len(self)):
            lo, hi = step * B, min(n, step * B + B)
            dst = self._destinations(step, hi - lo)
            res = store.batch(index[lo:hi], matrix[lo:hi] if self.augment else None, flip[lo:hi] if self.augment else None,
                              self.crop, out=dst)
            if store.device.type == "cuda" and hi - lo == B:
                self._sets[step % len(self._sets)].update(res)          # buffers the first full batch allocated are kept
            invalid = res.pop("invalid")
            yield IdentityBatch(res, [names[i] for i in order[lo:hi]], hi - lo, invalid)
