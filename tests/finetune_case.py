"""The setup of tests/golden/reference_finetune.pt (tests/golden/make_finetune_golden.py) on this repository's trainer -- a plain
helper module, not a conftest: LightCNNTrainer(num_classes=300), fill_module, every `weight` outside fc2 times the fixture's gain,
batch 4 of fill.image(4, 1, 128, 128, "ft"), the closed-form dropout mask (fill.wave(shape, "dropout") > 0) * 2."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import fill  # noqa: E402

NAMED = ("conv1.filter.weight", "conv1.filter.bias", "block2.0.conv1.filter.weight", "fc.filter.weight", "fc2.weight", "fc2.bias")


def fixture():
    return torch.load(os.path.join(HERE, "golden", "reference_finetune.pt"), map_location="cpu")


def fill_network(net, gain):
    fill.fill_module(net)
    with torch.no_grad():
        for name, value in net.named_parameters():
            if name.endswith("weight") and "fc2" not in name:
                value.mul_(gain)
    return net


def make_trainer(device, fx, dtype=torch.float32, **kw):
    """-> (trainer, batch, dropout mask, the filled start of every parameter on the CPU in float64)."""
    from ffwm_amd import trainer
    tr = trainer.LightCNNTrainer(device, num_classes=int(fx["num_classes"]), lr=float(fx["base_lr"]), **kw)
    # (filled in float32, as the generator fills the reference's module, then cast)
    fill_network(tr.net, float(fx["gain"]))
    if dtype != torch.float32:
        tr.cast(dtype)
    start = {k: v.detach().cpu().double().clone() for k, v in tr.net.named_parameters()}
    batch = {"img": fill.image(4, 1, 128, 128, "ft").to(device, dtype), "target": fx["targets"].to(device)}
    mask = ((fill.wave((4, 256), "dropout") > 0) * 2).to(device, dtype)
    return tr, batch, mask, start


def sample(t, samples):
    flat = t.reshape(-1)
    return flat[::-(-flat.numel() // samples)]
