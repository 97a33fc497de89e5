"""Generates tests/golden/face_dataset.pt by running the REFERENCE's own FaceDataset (data/face_dataset.py, imported from
/root/reference) on the small sets of tests/face_data_cases.py.  Runs only in the build container; the fixture is what travels.

    python tests/golden/make_face_dataset_golden.py

The reference's module imports cv2 (only its non-preload readers and --aug use it) and, through data/base_dataset.py, torchvision:
both are stubbed with empty modules.  FaceDataset.__init__ would list a directory, so it is bypassed (__new__) and the fields it sets
are filled directly: preload = True, image_dict / mask_dict ([H, W, 3] / [H, W, 1] uint8 per file, as read_images leaves them), pairs
as get_pairs builds them for multipie, lm_dicts as landmarks.npy holds them.  Recorded for s16: get_train_item for every index in
[0, 2 P), torch's default_collate of a list of them (flipped, unflipped and one repeated), and with isval = True get_test_item for
every index and a collate of three; for s128 (128 x 128: each float plane counts) one unflipped and one flipped training item, their
collate, and the collate of one test item.

A float image is stored as the byte it came from (every output value is table[byte], checked here) plus the reference's own table of
byte / 255 -- read off its outputs, image 0 of s16 holds every byte value -- so the file stays small.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.modules["cv2"] = types.ModuleType("cv2")
if "torchvision" not in sys.modules:
    try:
        import torchvision  # noqa: F401
    except ImportError:
        tv = types.ModuleType("torchvision")
        tv.transforms = types.ModuleType("torchvision.transforms")
        sys.modules["torchvision"] = tv
        sys.modules["torchvision.transforms"] = tv.transforms

import face_data_cases as fc  # noqa: E402
from data.face_dataset import FaceDataset, s2f  # noqa: E402
from torch.utils.data.dataloader import default_collate  # noqa: E402

COLLATE = {"s16": [0, 7, 3, 9, 3, 5], "s128": [1, 6]}          # item indices of the recorded batch
TEST_COLLATE = {"s16": [0, 1, 4], "s128": [3]}
FLOAT_KEYS = ("img_S", "img_F", "mask_S", "mask_F")


def dataset(c, isval):
    d = FaceDataset.__new__(FaceDataset)
    d.preload, d.load_size, d.isval = True, c["load_size"], isval
    d.opt = argparse.Namespace(aug=False, preload=True, load_size=c["load_size"])
    d.image_dict = {n: c["images"][i] for i, n in enumerate(c["names"])}
    d.mask_dict = {n: c["masks"][i][:, :, np.newaxis] for i, n in enumerate(c["names"])}
    d.files = list(c["names"])
    d.pairs = [(f, s2f(f)) for f in d.files]
    d.lm_dicts = c["lm_dicts"]
    return d


def main():
    cases = {name: fc.case(name) for name in ("s16", "s128")}
    # the reference's byte -> float table, read off an item whose source image holds every byte value
    c = cases["s16"]
    item = dataset(c, False)[0]
    src = torch.from_numpy(c["images"][0].transpose(2, 0, 1).copy()).long()
    table = torch.full((256,), float("nan"))
    table[src.reshape(-1)] = item["img_S"].reshape(-1)
    assert not torch.isnan(table).any() and torch.equal(table[src], item["img_S"]) and bool((table[1:] > table[:-1]).all())

    def encode(t):
        b = torch.searchsorted(table, t.contiguous())
        assert torch.equal(table[b.clamp(max=255)], t), "an output value that is no byte / 255 of the table"
        return b.to(torch.uint8)

    def pack(d):
        return {k: (encode(v) if k in FLOAT_KEYS else v) for k, v in d.items()}

    out = {"table": table, "cases": {}}
    for name, c in cases.items():
        train, test = dataset(c, False), dataset(c, True)
        rec = {"len_train": len(train), "len_test": len(test), "pairs": list(train.pairs),
               "items": {i: pack(train[i]) for i in (range(len(train)) if name == "s16" else COLLATE[name])},
               "collate_indices": COLLATE[name], "collate": pack(default_collate([train[i] for i in COLLATE[name]])),
               "test_items": {i: pack(test[i]) for i in (range(len(test)) if name == "s16" else ())},
               "test_collate_indices": TEST_COLLATE[name], "test_collate": pack(default_collate([test[i] for i in TEST_COLLATE[name]]))}
        out["cases"][name] = rec
        print(name, "P = %d, %d train items, %d test items recorded" % (len(train.pairs), len(rec["items"]), len(rec["test_items"])))
    path = os.path.join(HERE, "face_dataset.pt")
    torch.save(out, path)
    print("wrote face_dataset.pt  %.1f KiB" % (os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
