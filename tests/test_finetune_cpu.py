"""LightCNN fine-tuning on the CPU (trainer.LightCNNTrainer) against tests/golden/reference_finetune.pt, which the REFERENCE's own
lightcnn/finetune.py and light_cnn.py produced (tests/golden/make_finetune_golden.py): losses, logits, precisions, the learning-rate
schedule and the parameter deltas of four steps; then the names around it: targets_from_names, the checkpoint files and who can load
them (nets.LightCNN29, FaceIdentifier's loader, FFWMTrainer.load_lightcnn), and validate() against the reference's
MultiPIEAverageMeter restated."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import finetune_case as fc  # noqa: E402
import torch_refs  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return fc.fixture()


def _four_steps(tr, batch, mask):
    out = {"loss": [], "prec1": [], "prec5": [], "logits": [], "params": {}}
    for step in range(4):
        if step == 3:
            out["lr"] = tr.adjust_learning_rate(25)
        r = tr.step(batch, dropout_mask=mask)
        out["loss"].append(float(r["loss"]))
        out["prec1"].append(float(r["prec1"]))
        out["prec5"].append(float(r["prec5"]))
        out["logits"].append(tr.logits.detach().cpu().double().clone())
        if step >= 2:
            out["params"][step + 1] = {k: v.detach().cpu().double().clone() for k, v in tr.net.named_parameters()}
    return out


def test_float64_trainer_reproduces_the_reference(fx):
    """Losses and logits to 1e-9 relative; each stored parameter delta to 1e-7 of that tensor's largest delta.  The step is
    ill-conditioned: the generator measured that a float32 run of the REFERENCE deviates from its float64 run by 1.4e-2 of a tensor's
    largest delta after three steps (1.3e-2 after four).  The same amplification of 2^-53 gives about 3e-11, and 1e-7 leaves three
    decades."""
    tr, batch, mask, start = fc.make_trainer("cpu", fx, torch.float64)
    assert len(tr.optimizer.param_groups) == 62
    got = _four_steps(tr, batch, mask)
    for step in range(4):
        assert got["loss"][step] == pytest.approx(float(fx["loss"][step]), rel=1e-9)
        ref = fx["logits"][step]
        assert float((got["logits"][step] - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
        assert got["prec1"][step] == pytest.approx(float(fx["prec1"][step])) and got["prec5"][step] == pytest.approx(float(fx["prec5"][step]))
    assert got["lr"] == pytest.approx(fx["lr"].tolist(), rel=1e-15)
    assert sorted(set(round(v / float(fx["base_lr"]) / 0.457305051927326, 9) for v in got["lr"])) == [1.0, 2.0, 10.0, 20.0]
    for step in (3, 4):
        for name in fc.NAMED:
            delta = fc.sample(got["params"][step][name] - start[name], int(fx["samples"]))
            ref, largest = fx["delta%d" % step][name], fx["delta%d_max" % step][name]
            err = float((delta - ref).abs().max())
            print("step %d %s: error %.3g of the largest delta %.3g" % (step, name, err / largest, largest))
            assert err <= 1e-7 * largest, (step, name)
            # the WHOLE delta through its float64 sum and sum of squares (the large tensors are stored as samples): with every
            # element within e = 1e-7 of the largest delta, the sum moves by at most n e and the sum of squares by at most
            # sum (2 |d| e + e^2) <= 2 e sqrt(n sum d^2) + n e^2 (Cauchy-Schwarz)
            full = got["params"][step][name] - start[name]
            n, e = full.numel(), 1e-7 * largest
            assert n == fx["delta%d_numel" % step][name]
            assert abs(float(full.sum()) - fx["delta%d_sum" % step][name]) <= n * e, (step, name)
            sumsq = fx["delta%d_sumsq" % step][name]
            assert abs(float((full * full).sum()) - sumsq) <= 2 * e * (n * sumsq) ** 0.5 + n * e * e, (step, name)


def test_float32_trainer_reproduces_the_losses(fx):
    """Held to the losses alone, at 1e-5 relative (the reference's own float32 run is within 9.4e-8 of its float64 run), and not to
    the deltas: see the conditioning above."""
    tr, batch, mask, _ = fc.make_trainer("cpu", fx)
    got = _four_steps(tr, batch, mask)
    for step in range(4):
        assert got["loss"][step] == pytest.approx(float(fx["loss"][step]), rel=1e-5)


def test_targets_from_names():
    from ffwm_amd.trainer import LightCNNTrainer
    t = LightCNNTrainer.targets_from_names(["001_01_01_051_07.png", "/data/train/250_01_01_190_12_crop_128.png", "300_x.png"])
    assert t.dtype == torch.int64 and t.tolist() == [0, 249, 299]


@pytest.fixture(scope="module")
def small():
    from ffwm_amd import trainer
    tr = trainer.LightCNNTrainer("cpu", num_classes=7, seed=3)
    return tr


def test_checkpoint_names_and_loaders(small, tmp_path):
    from ffwm_amd import nets, trainer
    d = str(tmp_path / "ckpt")
    small.save_checkpoint(d, 0)
    assert sorted(os.listdir(d)) == ["lightCNN_1_checkpoint.pth", "lightCNN_latest_checkpoint.pth"]
    small.save_checkpoint(d, 1)
    assert sorted(os.listdir(d)) == ["lightCNN_1_checkpoint.pth", "lightCNN_latest_checkpoint.pth"]
    small.save_checkpoint(d, 5)
    assert sorted(os.listdir(d)) == ["lightCNN_1_checkpoint.pth", "lightCNN_6_checkpoint.pth", "lightCNN_latest_checkpoint.pth"]
    path = os.path.join(d, "lightCNN_latest_checkpoint.pth")
    sd = torch.load(path, map_location="cpu")
    assert list(sd) == list(nets.LightCNN29(7).state_dict()) and all(not v.is_cuda for v in sd.values())
    # nets.LightCNN29, and the loader of FaceIdentifier.from_checkpoints (identity_eval.py: a plain load_state_dict of the file)
    fresh = nets.LightCNN29(7)
    fresh.load_state_dict(torch.load(path, map_location="cpu"))
    fresh.eval()
    for (k, a), b in zip(fresh.state_dict().items(), small.net.state_dict().values()):
        assert torch.equal(a, b), k
    # load_checkpoint writes in place
    other = trainer.LightCNNTrainer("cpu", num_classes=7, seed=4)
    before = [p.data_ptr() for p in other.net.parameters()]
    other.load_checkpoint(path)
    assert before == [p.data_ptr() for p in other.net.parameters()]
    assert torch.equal(other.net.fc2.weight, small.net.fc2.weight)


def test_ffwm_trainer_loads_the_checkpoint(tmp_path):
    """--lightcnn of train_ffwm.py: FFWMTrainer's identity network has 79 077 classes, so the file comes from a trainer of that size."""
    from ffwm_amd import nets, trainer
    src = trainer.LightCNNTrainer("cpu", seed=11)
    d = str(tmp_path / "full")
    path = src.save_checkpoint(d, 9)[-1]
    assert sorted(os.listdir(d)) == ["lightCNN_latest_checkpoint.pth"]
    t = trainer.FFWMTrainer("cpu", seed=5, ngf=4, warp=torch_refs.warp, warp_flipcat=torch_refs.warp_flipcat)
    assert not torch.equal(t.lightCNN.fc2.bias, src.net.fc2.bias)
    t.load_lightcnn(path)
    assert not t.lightCNN.training and not any(p.requires_grad for p in t.lightCNN.parameters())
    fresh = nets.LightCNN29()
    fresh.load_state_dict(torch.load(path, map_location="cpu"))
    fresh.eval()
    img = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = fresh(t._light_input(img))[1]
    assert torch.equal(t.identity_feature(img), want)
    # FaceIdentifier.from_checkpoints reads the same file beside the trainer's own checkpoints (test_ffwm.py --lightcnn)
    from ffwm_amd.identity_eval import FaceIdentifier
    t.save_networks(d, "latest")
    ident = FaceIdentifier.from_checkpoints(d, "latest", path, ngf=4, device="cpu", graph=False)
    gray = img.mean(1, keepdim=True)
    with torch.no_grad():
        folded, plain = ident.feature(gray), fresh(gray)[1]
    assert float((folded - plain).abs().max()) <= 1e-4 * float(plain.abs().max())
    t._graphs = [object()]
    try:
        with pytest.raises(RuntimeError):
            t.load_lightcnn(path)
    finally:
        t._graphs = None


class _ReferenceMeter(object):
    """MultiPIEAverageMeter.update (lightcnn/finetune.py:251-263) restated."""

    def __init__(self):
        self.stat_dict = {}

    def update(self, test_feas, test_names, gallery_feas, gallery_keys, topk=1):
        for b in range(test_feas.size(0)):
            ss = os.path.basename(test_names[b]).split("_")
            dis = torch.cosine_similarity(gallery_feas, test_feas[b:b + 1, :], dim=1)
            iii = dis.topk(k=min(max(10, topk), dis.numel()), dim=0)[1].tolist()
            ids = [gallery_keys[ii] for ii in iii]
            stat = self.stat_dict.setdefault(ss[3], {"correct": 0, "all": 0})
            stat["all"] += 1
            if ss[0] in ids[:topk]:
                stat["correct"] += 1


@pytest.mark.parametrize("crop", [False, True], ids=["plain", "crop"])
def test_validate_counts_like_the_reference_meter(small, crop):
    gen = torch.Generator().manual_seed(5)
    keys = ["%03d" % (i + 1) for i in range(6)]
    gallery = [torch.rand(1, 128, 128, generator=gen) for _ in keys]
    cameras = ["050", "140", "041", "190", "050", "240", "110", "041", "080"]
    owners = [0, 1, 2, 3, 4, 5, 0, 2, 4]
    probes = torch.stack([(gallery[o] * 0.7 + 0.3 * torch.rand(1, 128, 128, generator=gen)) if i % 3 else torch.rand(1, 128, 128, generator=gen)
                          for i, o in enumerate(owners)])
    names = ["probe/%s_01_01_%s_07.png" % (keys[o], c) for o, c in zip(owners, cameras)]
    assert small.net.training
    meter = small.validate(keys, gallery, probes, names, crop=crop)
    assert small.net.training                                   # train mode is restored
    small.net.eval()
    try:
        with torch.no_grad():
            g = torch.stack(gallery)
            if crop:
                g = torch.nn.functional.interpolate(g[:, :, 28:-2, 15:-15], (128, 128), mode="bilinear")
            ref = _ReferenceMeter()
            ref.update(small.net(probes)[1], names, small.net(g)[1], keys)
    finally:
        small.net.train()
    assert meter.stat_dict == ref.stat_dict and sum(v["all"] for v in meter.stat_dict.values()) == len(names)


def test_the_bench_tool_without_a_gpu_leaves_the_report_alone(tmp_path):
    """tools/finetune_bench.py measures nothing without a GPU: it ends with a non-zero status and does not replace the report."""
    import subprocess
    out = tmp_path / "report.txt"
    out.write_text("kept\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), "tools", "finetune_bench.py"), "--out", str(out)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode != 0 and out.read_text() == "kept\n"
    failed = tmp_path / "report.txt.failed"
    assert failed.exists() and "part a ended with status" in failed.read_text() and "Traceback" not in failed.read_text()
