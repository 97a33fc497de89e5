"""What the device-resident identity store (ffwm_amd.data.IdentityStore, csrc/identity_batch.hip) buys per LightCNN fine-tuning batch,
measured on an MI355X:

    python tools/identity_data_bench.py [--pairs 5] [--batches 10 64] [--out profiles/identity_data.txt]

Training batches at 128 x 128 with --crop, from a synthetic set of 256 files, at every batch size of --batches:
  A  what a user has without this module (and without torchvision): per item PIL's Image.rotate(angle, BICUBIC) and
     transpose(FLIP_LEFT_RIGHT) on the host, ToTensor's arithmetic, torch.mean, the slice and F.interpolate of dataset.py:62-67, the
     default collate and .to(device) -- in one process (the reference spreads the host half over 2 workers; the copy it cannot)
  B  IdentityLoader's step on the device store: slices of the uploaded index / matrix / flip vectors and one launch of
     ffwm_identity_batch
Both as wall-clock time per batch over a window of batches -- about half a second each -- that ends in one synchronisation, the
windows alternating for --pairs pairs, reported as median and min-max; the launch also as device time inside a captured graph, with
and without crop.  The acceptance condition of the record: B below A by more than the larger min-max spread at every batch size.
The GPU work runs in a child process under its own time limit; the parent never opens the GPU.  GPU only; A needs PIL.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from abtime import captured, line  # noqa: E402

DEV = "cuda:0"
LIMIT = 420          # seconds for the child
FILES = 256


def measure(args):
    import numpy as np
    import torch
    from PIL import Image
    import identity_data_cases as ic
    from ffwm_amd import data as fd
    names, images = ic.synthetic(FILES, 128, 128, seed=1)
    host = fd.IdentityStore.from_arrays(images, names)
    dev = host.to(DEV)
    print("# identity batches: 128 x 128 with --crop, %d files (%.1f MiB on the device), device %s" % (
        FILES, dev.nbytes() / 2.0 ** 20, torch.cuda.get_device_name(0)))
    print("# A = PIL rotate + flip per item, mean / crop with torch, collate, .to(device); B = one ffwm_identity_batch launch on the device "
          "store; wall-clock ms per batch, %d alternating pairs of windows of about half a second" % args.pairs)
    status = 0
    for B in args.batches:
        loader = fd.IdentityLoader(host, B, crop=True, seed=0)
        perm, angles, flips = loader.draws(0)
        index, matrix, flip = perm.to(DEV), loader.matrices(angles).to(DEV), flips.to(DEV)
        order, angle_list, flip_list, targets = perm.tolist(), angles.tolist(), flips.tolist(), host.t["targets"]
        per_epoch = FILES // B
        keep = {}

        def batch_a(lo):
            items = []
            for j in range(lo, lo + B):
                im = Image.fromarray(images[order[j]]).rotate(angle_list[j], resample=Image.BICUBIC, expand=False)
                if flip_list[j]:
                    im = im.transpose(Image.FLIP_LEFT_RIGHT)
                t = torch.from_numpy(np.asarray(im)).permute((2, 0, 1)).contiguous().to(dtype=torch.float32).div(255)
                t = torch.mean(t, dim=(0, ), keepdim=True)[:, 28:-2, 15:-15]
                items.append(torch.nn.functional.interpolate(t.unsqueeze(0), (128, 128), mode="bilinear")[0])
            keep["a"] = {"img": torch.stack(items).to(DEV), "target": targets[perm[lo:lo + B].long()].to(DEV)}

        def window_a(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(steps):
                batch_a(B * (s % per_epoch))
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / steps

        bufs = [{}, {}]

        def window_b(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(steps):
                lo = B * (s % per_epoch)
                bufs[s % 2].update(dev.batch(index[lo:lo + B], matrix[lo:lo + B], flip[lo:lo + B], crop=True, out=bufs[s % 2]))
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / steps

        # windows of about half a second, each a whole number of epochs so that A and B end on the same batch
        window_b(per_epoch)          # allocations, the library's load
        steps_a = per_epoch * max(1, int(round(500.0 / (window_a(per_epoch) * per_epoch))))
        steps_b = per_epoch * max(1, int(round(500.0 / (window_b(8 * per_epoch) * per_epoch))))
        window_b(steps_b)
        last = bufs[(steps_b - 1) % 2]
        diff = (keep["a"]["img"].double() - last["img"].double()).abs().max().item()
        same = diff <= 2.0 ** -21 and torch.equal(keep["a"]["target"], last["target"])
        status |= 0 if same else 1
        print("batch %d: windows of %d (A) and %d (B) batches; the last batch of A and of B: targets %s, images differ by at most %.3g "
              "(%s the 2^-21 of the float32 resize)" % (B, steps_a, steps_b, "equal" if torch.equal(keep["a"]["target"], last["target"])
                                                         else "DIFFERENT", diff, "within" if diff <= 2.0 ** -21 else "BEYOND"))
        ms = {"A": [], "B": []}
        for _ in range(args.pairs):
            ms["A"].append(window_a(steps_a))
            ms["B"].append(window_b(steps_b))
        print(line("  A (PIL per item + copy)", ms["A"], "ms"))
        print(line("  B (one launch)         ", ms["B"], "ms"))
        margin = statistics.median(ms["A"]) - statistics.median(ms["B"])
        worst = max(max(v) - min(v) for v in ms.values())
        print("  A - B = %.3f ms against the larger min-max spread %.3f ms: B is %s; A / B = %.1f" % (
            margin, worst, "below A by more than the spread" if margin > worst else "NOT below A by more than the spread",
            statistics.median(ms["A"]) / statistics.median(ms["B"])))
        for crop in (False, True):
            out = {}
            out.update(dev.batch(index[:B], matrix[:B], flip[:B], crop=crop))
            replay = captured(lambda: dev.batch(index[:B], matrix[:B], flip[:B], crop=crop, out=out), 20)
            dev_us = [1e3 * replay() for _ in range(args.pairs)]
            print(line("  B, device time of the launch in a captured graph, %s" % ("with crop   " if crop else "without crop"), dev_us, "us"),
                  flush=True)
    return status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[10, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "identity_data.txt"))
    ap.add_argument("--child", action="store_true", help="measure in this process (what the parent starts)")
    args = ap.parse_args()
    if args.pairs < 5:
        sys.exit("identity_data_bench: at least five pairs")
    if any(b < 1 or b > FILES for b in args.batches):
        sys.exit("identity_data_bench: batch sizes from 1 to %d" % FILES)
    if args.child:
        import torch
        if not torch.cuda.is_available():
            sys.exit("identity_data_bench: needs an MI355X; a CPU run measures nothing")
        sys.exit(measure(args))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--pairs", str(args.pairs), "--batches"] + [str(b) for b in args.batches]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT, cwd=ROOT)
        text, status = r.stdout, r.returncode
        if status != 0:
            text += "identity_data_bench: the measurement ended with status %d\n%s\n" % (status, r.stderr[-2000:])
    except subprocess.TimeoutExpired as e:
        text = (e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout or "") + "identity_data_bench: passed its limit of %d s\n" % LIMIT
        status = 124
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.exit(status)


if __name__ == "__main__":
    main()
