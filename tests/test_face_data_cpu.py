"""ffwm_amd.data on the CPU: FaceStore.host_item / host_batch against the reference's own FaceDataset (tests/golden/face_dataset.pt,
made by tests/golden/make_face_dataset_golden.py) bit for bit, pairing, the gallery, FaceLoader's epochs, the two file formats and the
argument checks of the C entry points (which return before any launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import face_data_cases as fc
from ffwm_amd import data as fd

HERE = os.path.dirname(os.path.abspath(__file__))
FLOAT_KEYS = ("img_S", "img_F", "mask_S", "mask_F")


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(HERE, "golden", "face_dataset.pt"))


def _store(name, isval=False, **kw):
    c = fc.case(name)
    return fd.FaceStore.from_arrays(c["images"], None if isval else c["masks"], c["names"], None if isval else c["lm_dicts"],
                                    isval=isval, load_size=c["load_size"], **kw)


def _decode(table, rec):
    return {k: (table[v.long()] if k in FLOAT_KEYS else v) for k, v in rec.items()}


def _same(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        if torch.is_tensor(w):
            assert got[k].dtype == w.dtype and got[k].shape == w.shape and torch.equal(got[k], w), k
        else:
            assert got[k] == w, k


def test_the_reference_divides_by_255(golden):
    """The fixture's table is the reference's byte -> float map: a true float32 division, which a multiplication by the rounded
    1 / 255 misses on 126 of the 256 bytes."""
    table = golden["table"]
    b = np.arange(256, dtype=np.float32)
    assert table.dtype == torch.float32 and np.array_equal(table.numpy(), b / np.float32(255))
    assert int((table.numpy() != b * (np.float32(1) / np.float32(255))).sum()) == 126


@pytest.mark.parametrize("name", ["s16", "s128"])
def test_train_items_and_collate_equal_the_reference(golden, name):
    rec, table = golden["cases"][name], golden["table"]
    store = _store(name)
    assert len(store) == rec["len_train"] == 2 * store.n_pairs and store.pairs == [tuple(p) for p in rec["pairs"]]
    assert len(rec["items"]) >= 2
    for i, want in rec["items"].items():
        _same(store.host_item(i), _decode(table, want))
    _same(store.host_batch(rec["collate_indices"]), _decode(table, rec["collate"]))
    flipped = [i for i in rec["collate_indices"] if i >= store.n_pairs]
    assert flipped and len(flipped) < len(rec["collate_indices"])


@pytest.mark.parametrize("name", ["s16", "s128"])
def test_test_items_and_collate_equal_the_reference(golden, name):
    rec, table = golden["cases"][name], golden["table"]
    store = _store(name, isval=True)
    assert len(store) == rec["len_test"] == store.n_pairs
    for i, want in rec["test_items"].items():
        _same(store.host_item(i), _decode(table, want))
    _same(store.host_batch(rec["test_collate_indices"]), _decode(table, rec["test_collate"]))
    with pytest.raises(IndexError):
        store.host_item(store.n_pairs)          # a test set has no flipped copies


def test_the_fixture_covers_what_it_should(golden):
    s16 = golden["cases"]["s16"]
    seen = torch.cat([s16["items"][0][k].reshape(-1) for k in FLOAT_KEYS]).unique()
    assert seen.numel() == 256                                             # every byte value
    assert sorted(s16["items"]) == list(range(10))                         # flipped and unflipped, P = 5
    hand = fc.case("s16")["lm_dicts"]["lm_S"]["001_01_01_041"]
    assert (hand != np.trunc(hand)).any() and hand.min() < 0 and hand.max() > 127          # non-integral, out of range
    lm, lm_flip = s16["items"][0]["lm_S"], s16["items"][5]["lm_S"]
    assert lm.dtype == torch.int64 and int(lm.min()) == 0 and int(lm.max()) == 15 and not torch.equal(lm, lm_flip)
    assert torch.equal(lm[:, 1], lm_flip[:, 1])
    assert golden["cases"]["s128"]["collate"]["img_S"].shape == (2, 3, 128, 128)


def test_flipped_landmarks_truncate_after_the_subtraction():
    """127 - 111.01 = 15.99 -> 15; truncating first would give 127 - 111 = 16.  And the constant is 127 at every image size."""
    plain, flipped = fd._landmark_rows(np.array([[111.01, 3.999], [-3.7, 0.5], [126.5, 200.9]]), 128)
    assert plain.tolist() == [[111, 3], [0, 0], [126, 127]] and flipped.tolist() == [[15, 3], [127, 0], [0, 127]]
    plain, flipped = fd._landmark_rows(np.array([[120.0, 2.0]]), 16)
    assert plain.tolist() == [[15, 2]] and flipped.tolist() == [[7, 2]]


def test_s2f_and_pairing_for_both_modes():
    assert fd.s2f("some/dir/001_01_01_190_06.png") == "001_01_01_051_06.png" == fd.s2f("001_01_01_051_06.png")
    c = fc.case("s16")
    store = _store("s16")
    assert store.pairs == [(n, fc.s2f(n)) for n in c["names"]] and len(store) == 2 * len(c["names"])
    other = fd.FaceStore.from_arrays(c["images"], c["masks"], c["names"], c["lm_dicts"], datamode="lfw", load_size=16)
    assert other.pairs == [(n, n) for n in c["names"]] and len(other) == 2 * len(c["names"])
    # lfw: lm_F is looked up under the file's own key, in the lm_F dict
    assert torch.equal(other.host_item(0)["lm_F"].int(), fd._landmark_rows(c["lm_dicts"]["lm_F"][fc.key(c["names"][0])], 16)[0])
    with pytest.raises(KeyError):
        fd.FaceStore.from_arrays(c["images"][:1], c["masks"][:1], c["names"][:1], c["lm_dicts"], load_size=16)          # no frontal file
    with pytest.raises(NotImplementedError, match="warpAffine"):
        fd.FaceStore.from_arrays(c["images"], c["masks"], c["names"], c["lm_dicts"], load_size=16, aug=True)
    with pytest.raises(NotImplementedError, match="warpAffine"):
        fd.FaceLoader(store, 2, aug=True)


def test_gallery_selection_and_values():
    c = fc.case("s16")
    store = _store("s16", isval=True)
    # the first *051_06.png per three-character identity, in the order of the names
    assert store.gallery_names == ["001_01_01_051_06.png", "002_01_01_051_06.png"]
    ids, planes = store.host_gallery()
    assert ids == ["001", "002"] and planes.shape == (2, 1, 16, 16) and planes.dtype == torch.float32
    for g, r in zip(planes, (1, 3)):
        x = torch.from_numpy(c["images"][r].transpose(2, 0, 1).astype("float32")).div(255)
        assert torch.equal(g, torch.mean(x, (0,), keepdim=True)) and torch.equal(g[0], ((x[0] + x[1]) + x[2]) / 3)
    listed = _store("s16", isval=True, gallery_list=np.array(["002_01_01_190_06.png"]))
    ids, planes = listed.host_gallery()
    x = torch.from_numpy(c["images"][2].transpose(2, 0, 1).astype("float32")).div(255)
    assert ids == ["002"] and torch.equal(planes[0], torch.mean(x, (0,), keepdim=True))
    with pytest.raises(KeyError):
        _store("s16", isval=True, gallery_list=["009_01_01_051_06.png"])
    with pytest.raises(ValueError):
        _store("s16").gallery_rows()          # a training set has none


def test_loader_epochs():
    store = _store("s16")
    n, P = len(store), store.n_pairs
    loader = fd.FaceLoader(store, 4, seed=5)
    assert loader.shuffle and len(loader) == 3
    epochs = []
    for _ in range(2):
        batches = list(loader)
        order = loader.permutation(loader.epoch - 1).tolist()
        assert sorted(order) == list(range(n))                                     # every index once
        assert [b.batch_weight for b in batches] == [4, 4, 2] == [b["img_S"].shape[0] for b in batches]          # the last batch is short
        assert [p for b in batches for p in b.input_path] == [store.names[i % P] for i in order]
        for s, b in enumerate(batches):
            want = store.host_batch(order[4 * s:4 * s + 4])
            assert b.input_path == want.pop("input_path") and set(b) == set(want) and all(torch.equal(b[k], want[k]) for k in want)
            assert b.invalid.tolist() == [0] * b.batch_weight
        epochs.append(order)
    assert epochs[0] != epochs[1] and epochs[0] != list(range(n))
    again = fd.FaceLoader(store, 4, seed=5)
    assert [again.permutation(e).tolist() for e in (0, 1)] == epochs            # the order follows from the seed
    assert fd.FaceLoader(store, 4, seed=6).permutation(0).tolist() != epochs[0]
    dropped = list(fd.FaceLoader(store, 4, seed=5, drop_last=True))
    assert [b.batch_weight for b in dropped] == [4, 4] and len(fd.FaceLoader(store, 4, drop_last=True)) == 2
    test = fd.FaceLoader(_store("s16", isval=True), 2)
    assert not test.shuffle and [b.input_path for b in test] == [store.names[0:2], store.names[2:4], store.names[4:5]]
    assert set(next(iter(test))) == {"img_S", "img_F"}


def test_batch_has_the_form_of_synthetic_batch():
    from ffwm_amd.trainer import synthetic_batch
    c = fc.synthetic(2, 128, 128, 1024, seed=3)
    store = fd.FaceStore.from_arrays(c["images"], c["masks"], c["names"], c["lm_dicts"])
    batch = next(iter(fd.FaceLoader(store, 3, seed=0)))
    want = synthetic_batch(3, "cpu")
    assert isinstance(batch, dict) and set(batch) == set(want) == set(fd.TRAIN_KEYS)
    for k, w in want.items():
        assert batch[k].dtype == w.dtype and batch[k].shape == w.shape and batch[k].is_contiguous(), k
    # what the trainers' capture() does with a batch: clone every value
    assert set({k: v.clone() for k, v in batch.items()}) == set(want)
    assert len(batch.input_path) == 3 and batch.batch_weight == 3


def test_npz_round_trip(tmp_path):
    for isval in (False, True):
        store = _store("s16", isval=isval)
        path = str(tmp_path / ("store%d.npz" % isval))
        store.save(path)
        back = fd.FaceStore.load(path)
        assert back.names == store.names and back.isval == isval and back.datamode == "multipie" and back.load_size == 16
        assert back.gallery_names == store.gallery_names
        for k, v in store.t.items():
            assert (back.t[k] is None) if v is None else (back.t[k].dtype == v.dtype and torch.equal(back.t[k], v)), k
        idx = list(range(len(store)))
        _same(back.host_batch(idx), store.host_batch(idx))


def test_directory_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    c = fc.case("s16")
    for split in ("train", "test"):
        base = tmp_path / "multipie" / split
        (base / "images").mkdir(parents=True)
        (base / "masks").mkdir()
        for i, n in enumerate(c["names"]):
            Image.fromarray(c["images"][i], "RGB").save(str(base / "images" / n))
            Image.fromarray(c["masks"][i], "L").save(str(base / "masks" / n))
        np.save(str(base / "landmarks.npy"), c["lm_dicts"], allow_pickle=True)
    order = sorted(range(len(c["names"])), key=lambda i: c["names"][i])
    want = fd.FaceStore.from_arrays(c["images"][order], c["masks"][order], [c["names"][i] for i in order], c["lm_dicts"], load_size=16)
    got = fd.FaceStore.from_directory(str(tmp_path), "multipie", isval=False, load_size=16, threads=2)
    assert got.names == want.names == sorted(c["names"])
    idx = list(range(len(want)))
    _same(got.host_batch(idx), want.host_batch(idx))
    test = fd.FaceStore.from_directory(str(tmp_path), "multipie", isval=True, load_size=16)
    assert test.isval and test.t["masks"] is None and test.gallery_names == ["001_01_01_051_06.png", "002_01_01_051_06.png"]
    np.save(str(tmp_path / "multipie" / "test" / "gallery_list.npy"), np.array(["002_01_01_190_06.png"]))
    assert fd.FaceStore.from_directory(str(tmp_path), "multipie", isval=True, load_size=16).gallery_names == ["002_01_01_190_06.png"]
    # a mask stored with colour channels is refused, and so is a grey image
    name = c["names"][0]
    Image.fromarray(c["images"][0], "RGB").save(str(tmp_path / "multipie" / "train" / "masks" / name))
    with pytest.raises(ValueError, match="single-channel"):
        fd.FaceStore.from_directory(str(tmp_path), "multipie", isval=False, load_size=16)
    Image.fromarray(c["masks"][0], "L").save(str(tmp_path / "multipie" / "test" / "images" / name))
    with pytest.raises(ValueError, match="RGB"):
        fd.FaceStore.from_directory(str(tmp_path), "multipie", isval=True, load_size=16)


def test_lazy_exports():
    import ffwm_amd
    assert ffwm_amd.FaceStore is fd.FaceStore and ffwm_amd.FaceLoader is fd.FaceLoader


def test_cpu_tensors_are_refused_by_the_op():
    from ffwm_amd import ops
    store = _store("s16")
    with pytest.raises(NotImplementedError):
        ops.face_batch(store.t["images"], store.t["pairs"], torch.zeros(1, dtype=torch.int32))


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from ffwm_amd import build, _lib
    build.build()
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(images=p, masks=p, pairs=p, pair_lm=p, lm=p, lm_flip=p, gate=p, index=p, img_S=p, img_F=p, mask_S=p, mask_F=p, lm_S=p,
                lm_F=p, gate_out=p, invalid=p, N=4, H=16, W=16, P=4, K=8, KG=4, L=9, B=2, train=1)

    def call(**kw):
        a = dict(good, **kw)
        return lib.ffwm_face_batch(*[a[k] for k in good], None)

    train_only = ("masks", "pair_lm", "lm", "lm_flip", "gate", "mask_S", "mask_F", "lm_S", "lm_F", "gate_out")
    for k in ("images", "pairs", "index", "img_S", "img_F", "invalid") + train_only:
        assert call(**{k: None}) == -1 and b"NULL" in lib.ffwm_last_error(), k
    for k in ("images", "pairs", "index", "img_S", "img_F", "invalid"):
        assert call(train=0, **{k: None}) == -1 and b"NULL" in lib.ffwm_last_error(), k
    for k in ("N", "H", "W", "P", "K", "KG", "L", "B"):
        for v in (0, -1):
            assert call(**{k: v}) == -1 and b"positive" in lib.ffwm_last_error(), (k, v)
    for v in (2, -1):
        assert call(train=v) == -1 and b"train" in lib.ffwm_last_error()
    assert call(W=8193) == -3 and call(H=8193) == -3 and b"8192" in lib.ffwm_last_error()
    assert call(B=65536) == -3 and call(L=(1 << 20) + 1) == -3 and call(N=1 << 31) == -3 and call(P=1 << 30) == -3

    gal = dict(images=p, rows=p, out=p, N=4, H=16, W=16, G=2)

    def gcall(**kw):
        a = dict(gal, **kw)
        return lib.ffwm_face_gallery(*[a[k] for k in gal], None)

    for k in ("images", "rows", "out"):
        assert gcall(**{k: None}) == -1 and b"NULL" in lib.ffwm_last_error(), k
    for k in ("N", "H", "W", "G"):
        assert gcall(**{k: 0}) == -1 and b"positive" in lib.ffwm_last_error(), k
    assert gcall(W=8193) == -3 and gcall(G=1 << 31) == -3 and gcall(N=1 << 31) == -3
