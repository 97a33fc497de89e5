"""Generates tests/golden/reference_finetune.pt by running the REFERENCE's own fine-tuning step (lightcnn/finetune.py and
lightcnn/light_cnn.py, imported from /root/reference; CPU, float64): LightCNN_29Layers(num_classes=300) in train mode,
nn.CrossEntropyLoss, finetune.accuracy, torch.optim.SGD over the parameter groups of finetune.main() (finetune.py:74-90; main() is not importable, so the
groups are built here) -- three steps, then finetune.adjust_learning_rate(optimizer, 25) and a fourth.
Runs only in the build container; the fixture (tensors and numbers only) is what travels.

    python tests/golden/make_finetune_golden.py

Setup: batch 4 of fill.image(4, 1, 128, 128, "ft"), targets [3, 299, 0, 150], fill_module, then every `weight` outside fc2 times 0.5
(with the unscaled fill the reference itself diverges to 1e9 .. inf within two steps), lr 1e-4.  torch.nn.functional.dropout is
replaced by the closed-form mask (fill.wave(shape, "dropout") > 0) * 2 so that both sides drop the same units.  cv2, torchvision and
PIL (imported by lightcnn/dataset.py, never used here) are stubbed.

Stored: per step the loss, prec@1 / prec@5 from finetune.accuracy and the logits; the per-group learning rates after the schedule;
for six named tensors the parameter deltas (against the filled start) after step 3 and after step 4 -- of a tensor with more than
SAMPLES elements every stride-th element of the flattened delta (stride = ceil(numel / SAMPLES); fc.filter.weight alone has 4.2 M
elements and a committed file stays under 1 MiB), with the largest |delta|, the sum and the sum of squares of the WHOLE delta
(float64) beside it, so that an error confined to elements that are not sampled still shows.

The same run in float32 is printed beside it: how far a float32 run of the REFERENCE is from its float64 run, in losses and in units
of each tensor's largest delta -- the conditioning that tests/test_finetune_cpu.py quotes.
"""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
REF = "/root/reference/lightcnn"
sys.path.insert(0, REF)
for name in ("cv2", "torchvision", "torchvision.transforms", "PIL", "PIL.Image"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.modules["PIL"].Image = sys.modules["PIL.Image"]

import fill  # noqa: E402
import finetune  # noqa: E402
from light_cnn import LightCNN_29Layers  # noqa: E402

NUM_CLASSES, LR = 300, 1e-4
TARGETS = [3, 299, 0, 150]
GAIN = 0.5
SAMPLES = 4096
NAMED = ("conv1.filter.weight", "conv1.filter.bias", "block2.0.conv1.filter.weight", "fc.filter.weight", "fc2.weight", "fc2.bias")

MOMENTUM, DECAY = 0.9, 1e-4
finetune.args = types.SimpleNamespace(lr=LR, momentum=MOMENTUM, weight_decay=DECAY)          # adjust_learning_rate prints args.lr


def masked_dropout(x, p=0.5, training=True, inplace=False):
    if not training:
        return x
    return x * ((fill.wave(tuple(x.shape), "dropout") > 0) * 2).to(x.dtype)


torch.nn.functional.dropout = masked_dropout


def accuracy(output, target):
    try:
        return finetune.accuracy(output, target, topk=(1, 5))
    except RuntimeError:
        # finetune.py:305 calls .view(-1) on a slice of a transposed tensor, which current PyTorch refuses for k > 1; the same
        # function with the tensor made contiguous first (values unchanged)
        view = torch.Tensor.view
        torch.Tensor.view = lambda self, *shape: view(self.contiguous(), *shape)
        try:
            return finetune.accuracy(output, target, topk=(1, 5))
        finally:
            torch.Tensor.view = view


def sample(t):
    flat = t.reshape(-1)
    return flat[::-(-flat.numel() // SAMPLES)].clone()


def run(dtype):
    model = LightCNN_29Layers(num_classes=NUM_CLASSES)
    fill.fill_module(model)
    with torch.no_grad():
        for name, value in model.named_parameters():
            if name.endswith("weight") and "fc2" not in name:
                value.mul_(GAIN)
    model = model.to(dtype).train()
    # the groups of finetune.py:74-90: one per tensor; biases at twice the rate (fc2's at twenty times) without decay, fc2's weight
    # at ten times the rate, and the optimizer's defaults for whatever a group leaves open
    groups = []
    for name, value in model.named_parameters():
        last = "fc2" in name
        if "bias" in name:
            groups.append({"params": value, "lr": (20 if last else 2) * LR, "weight_decay": 0})
        else:
            groups.append({"params": value, "lr": (10 if last else 1) * LR})
    optimizer = torch.optim.SGD(groups, LR, momentum=MOMENTUM, weight_decay=DECAY)
    criterion = torch.nn.CrossEntropyLoss()
    start = {k: v.detach().clone() for k, v in model.named_parameters()}
    img = fill.image(4, 1, 128, 128, "ft").to(dtype)
    target = torch.tensor(TARGETS, dtype=torch.int64)
    out = {"loss": [], "prec1": [], "prec5": [], "logits": [], "grad_max": []}
    for step in range(4):
        if step == 3:
            finetune.adjust_learning_rate(optimizer, 25)
        output, _, _ = model(img)
        loss = criterion(output, target)
        optimizer.zero_grad()
        loss.backward()
        out["grad_max"].append(max(float(p.grad.abs().max()) for p in model.parameters()))
        optimizer.step()
        prec1, prec5 = accuracy(output.data, target)
        out["loss"].append(loss.item())
        out["prec1"].append(prec1.item())
        out["prec5"].append(prec5.item())
        out["logits"].append(output.detach().clone())
        if step >= 2:
            named = dict(model.named_parameters())
            out["delta%d" % (step + 1)] = {k: (named[k].detach() - start[k]).clone() for k in NAMED}
    out["lr"] = [g["lr"] for g in optimizer.param_groups]
    return out


torch.set_num_threads(8)
r64, r32 = run(torch.float64), run(torch.float32)
print("float64 losses", r64["loss"], "largest gradient per step", r64["grad_max"])
print("float32 losses", r32["loss"])
print("float32 against float64, losses (relative):", max(abs(a - b) / abs(b) for a, b in zip(r32["loss"], r64["loss"])))
for key in ("delta3", "delta4"):
    worst = max(float((r32[key][k].double() - r64[key][k]).abs().max() / r64[key][k].abs().max()) for k in NAMED)
    print("float32 against float64, %s (of a tensor's largest delta): %.3g" % (key, worst))

for key in ("delta3", "delta4"):
    r64[key + "_max"] = {k: float(v.abs().max()) for k, v in r64[key].items()}
    r64[key + "_sum"] = {k: float(v.sum()) for k, v in r64[key].items()}
    r64[key + "_sumsq"] = {k: float((v * v).sum()) for k, v in r64[key].items()}
    r64[key + "_numel"] = {k: v.numel() for k, v in r64[key].items()}
    r64[key] = {k: sample(v) for k, v in r64[key].items()}
fixture = {"loss": torch.tensor(r64["loss"], dtype=torch.float64), "prec1": torch.tensor(r64["prec1"], dtype=torch.float64),
           "prec5": torch.tensor(r64["prec5"], dtype=torch.float64), "logits": torch.stack(r64["logits"]),
           "lr": torch.tensor(r64["lr"], dtype=torch.float64), "delta3": r64["delta3"], "delta4": r64["delta4"],
           "delta3_max": r64["delta3_max"], "delta4_max": r64["delta4_max"], "samples": SAMPLES,
           **{"%s_%s" % (key, what): r64["%s_%s" % (key, what)] for key in ("delta3", "delta4") for what in ("sum", "sumsq", "numel")},
           "targets": torch.tensor(TARGETS), "num_classes": NUM_CLASSES, "gain": GAIN, "base_lr": LR}
path = os.path.join(HERE, "reference_finetune.pt")
torch.save(fixture, path)
print("wrote reference_finetune.pt  %.1f KiB" % (os.path.getsize(path) / 1024.0))
