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
Not reproduced: the rotation of --aug (its image half is cv2.warpAffine, which cannot be checked without OpenCV: aug=True raises),
lightcnn/dataset.py's transform, reading without --preload, sharding over ranks.  The reference walks os.listdir() order (arbitrary)
and shuffles the files before it picks a gallery; from_directory sorts the names, so "first" means first by name.
"""
import os

import numpy as np
import torch

TRAIN_KEYS = ("img_S", "img_F", "mask_S", "mask_F", "lm_F", "lm_S", "gate")
TEST_KEYS = ("img_S", "img_F")
_TABLES = ("images", "masks", "pairs", "pair_lm", "lm", "lm_flip", "gate")


def s2f(file):
    """The frontal file of a MultiPIE file: the fourth `_`-separated field of the name becomes 051 (face_dataset.py:10-17)."""
    name = os.path.split(file)[1]
    ss = name.split("_")
    return "{}_{}_{}_{}_{}".format(ss[0], ss[1], ss[2], "051", ss[4])


def _refuse_aug(aug):
    if aug:
        raise NotImplementedError(
            "the random rotation of --aug is not implemented: its image half is cv2.warpAffine, and without OpenCV there is nothing to "
            "check a kernel against")


def _landmark_rows(arr, load_size):
    """One entry of lm_dicts['lm_S' / 'lm_F'] -> (plain, flipped) int32 [L, 2], by the reference's own calls (face_dataset.py:66-67, 82-85)."""
    arr = np.asarray(arr).copy()
    if arr.ndim != 2 or arr.shape[1] != 2:
        raise ValueError("a landmark entry must be [L, 2], got %s" % (arr.shape,))
    flipped = np.hstack((127 - arr[:, 0:1], arr[:, 1:2]))
    return tuple(torch.clamp(torch.from_numpy(np.ascontiguousarray(a)).long(), 0, load_size - 1).to(torch.int32) for a in (arr, flipped))


class FaceBatch(dict):
    """A batch: a dict of exactly the tensors trainer.synthetic_batch makes (what FFWMTrainer / FlowNetTrainer .step and .capture take
    -- capture clones every value, so the dict holds tensors only), with the rest as attributes:
      .input_path    the file of S per sample (the reference's batch["input_path"]), from the host copy of the permutation
      .batch_weight  the samples in this batch: the w of train_ffwm.py's sum_loss
      .invalid       int32 [B] on the device, 1 where an index was out of range (never, from a FaceLoader)"""

    def __init__(self, tensors, input_path, batch_weight, invalid=None):
        dict.__init__(self, tensors)
        self.input_path, self.batch_weight, self.invalid = input_path, batch_weight, invalid


class FaceStore(object):
    """The preloaded set as tensors on one device (see the module's text).  Build it with from_arrays / from_directory / load."""

    def __init__(self, tensors, names, isval, datamode, load_size, gallery_names, host=None):
        self.t = tensors                      # images, masks, pairs, pair_lm, lm, lm_flip, gate (None where the mode has none)
        self.names = list(names)
        self.isval, self.datamode, self.load_size = bool(isval), datamode, int(load_size)
        self.gallery_names = list(gallery_names) if gallery_names is not None else None
        self.host = host if host is not None else self          # the CPU store behind a device store: host_item, names, the gallery's rows
        self.device = tensors["images"].device

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_arrays(cls, images, masks, names, lm_dicts=None, datamode="multipie", isval=False, load_size=128, gallery_list=None,
                    aug=False):
        """images uint8 [N, H, W, 3] (RGB) and masks uint8 [N, H, W] or [N, H, W, 1] (None for a test set) in the order of `names`
        (the reference's self.files); lm_dicts = {"lm_S": {key: [L, 2]}, "lm_F": {...}, "gate": {key: [L]}} (landmarks.npy) for a
        training set.  gallery_list: the names of gallery_list.npy, or None for the reference's rule (multipie test sets only)."""
        _refuse_aug(aug)
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
            lm_rows, gate_rows, plain, flipped, gates, pair_lm = {}, {}, [], [], [], []
            for s, f in pairs:
                ks = []
                for which, key in (("lm_S", names[s][:-7]), ("lm_F", names[f][:-7])):
                    if (which, key) not in lm_rows:
                        a, b = _landmark_rows(lm_dicts[which][key], load_size)
                        lm_rows[(which, key)] = len(plain)
                        plain.append(a)
                        flipped.append(b)
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
    def from_directory(cls, dataroot, datamode="multipie", isval=False, load_size=128, threads=8, aug=False):
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
        return cls.from_arrays(images, masks, names, lm_dicts, datamode, isval, load_size, gallery_list)

    def save(self, path):
        """The store as one uncompressed .npz (the tables as they are: load() needs no landmarks.npy and converts nothing again)."""
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

    def host_item(self, index):
        """Item `index` on the CPU, step by step as get_test_item / get_train_item compute it (face_dataset.py:37-90)."""
        h = self.host
        P = h.n_pairs
        if not 0 <= index < len(h):
            raise IndexError("item %d of %d" % (index, len(h)))
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
        table = h.t["lm"]
        if index >= P:
            table = h.t["lm_flip"]
            img_S, img_F, mask_S, mask_F = img_S[:, ::-1, :], img_F[:, ::-1, :], mask_S[:, ::-1, :], mask_F[:, ::-1, :]
        item = {k: torch.from_numpy(v.transpose((2, 0, 1)).astype("float32")).div(255)
                for k, v in (("img_S", img_S), ("img_F", img_F), ("mask_S", mask_S), ("mask_F", mask_F))}
        item.update({"input_path": h.names[s], "lm_S": table[rs].long(), "lm_F": table[rf].long(), "gate": h.t["gate"][rg].clone().unsqueeze(1)})
        return item

    def host_batch(self, indices):
        """The default collate of host_item over `indices`: {key: [B, ...]} plus "input_path" as a list -- what one step of the
        reference's DataLoader hands out."""
        items = [self.host_item(int(i)) for i in indices]
        batch = {k: torch.stack([it[k] for it in items]) for k in items[0] if k != "input_path"}
        batch["input_path"] = [it["input_path"] for it in items]
        return batch

    def batch(self, index, out=None):
        """-> the tensors of the batch of `index` (int32 [B] on the store's device; a list on a CPU store) plus "invalid": one launch of
        ops.face_batch on a device store, host_batch on a CPU store.  `out`: destinations written in place."""
        if self.device.type == "cuda":
            from . import ops
            t = self.t
            if self.isval:
                return ops.face_batch(t["images"], t["pairs"], index, out=out)
            return ops.face_batch(t["images"], t["pairs"], index, t["masks"], t["pair_lm"], t["lm"], t["lm_flip"], t["gate"], out=out)
        idx = index.tolist() if torch.is_tensor(index) else list(index)
        res = self.host_batch(idx)
        del res["input_path"]
        res["invalid"] = torch.zeros(len(idx), dtype=torch.int32)
        if out is not None:
            for k, v in res.items():
                if out.get(k) is not None:
                    res[k] = out[k].copy_(v)
        return res

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
    A short last batch is written into the leading rows of its buffers."""

    def __init__(self, store, batch_size, shuffle=None, drop_last=False, seed=0, out=None, aug=False):
        _refuse_aug(aug)
        if batch_size < 1:
            raise ValueError("batch_size must be positive")
        self.store, self.batch_size, self.drop_last, self.seed = store, int(batch_size), bool(drop_last), int(seed)
        self.shuffle = (not store.isval) if shuffle is None else bool(shuffle)
        self.epoch = 0
        self.out = out
        self._sets = [dict(out)] if out is not None else None          # (a copy: the loader adds its `invalid` buffer to it)

    def __len__(self):
        n, B = len(self.store), self.batch_size
        return n // B if self.drop_last else (n + B - 1) // B

    def permutation(self, epoch):
        """The item order of `epoch` as an int32 tensor on the host."""
        n = len(self.store)
        if not self.shuffle:
            return torch.arange(n, dtype=torch.int32)
        return torch.randperm(n, generator=torch.Generator().manual_seed(self.seed + epoch)).to(torch.int32)

    def _destinations(self, step, b):
        if self.store.device.type != "cuda":
            return self.out if (self.out is None or b == self.batch_size) else {k: v[:b] for k, v in self.out.items()}
        if self._sets is None:
            self._sets = [{}, {}]
        dst = self._sets[step % len(self._sets)]
        return dst if b == self.batch_size else {k: v[:b] for k, v in dst.items()}

    def __iter__(self):
        store, B = self.store, self.batch_size
        perm = self.permutation(self.epoch)
        self.epoch += 1
        index = perm.to(store.device)          # the one upload of the epoch
        order = perm.tolist()
        names = store.host.names
        rows_S = store.host.t["pairs"][:, 0].tolist()
        P, n = store.n_pairs, len(store)
        for step in range(len(self)):
            lo, hi = step * B, min(n, step * B + B)
            dst = self._destinations(step, hi - lo)
            res = store.batch(index[lo:hi], out=dst)
            if store.device.type == "cuda" and hi - lo == B:
                self._sets[step % len(self._sets)].update(res)          # buffers the first full batch allocated are kept
            invalid = res.pop("invalid")
            yield FaceBatch(res, [names[rows_S[i % P]] for i in order[lo:hi]], hi - lo, invalid)
