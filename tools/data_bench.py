"""What the device-resident face store (ffwm_amd.data, csrc/face_batch.hip) buys per training batch, measured on an MI355X:

    python tools/data_bench.py [--pairs 5] [--steps 256] [--steps-b 25600] [--out profiles/face_dataset.txt]

A batch of 8 at 128 x 128 with L = 1024 landmarks, from a synthetic set of 128 files (256 items):
  A  FaceStore.host_batch (the reference's work with --preload, item by item: float copies, flip, HWC -> CHW, / 255, collate) and
     .to(device) of its seven tensors -- how the reference's loader delivers a batch, in one process (the reference spreads the
     host half over --num_threads workers; the copy it cannot)
  B  FaceLoader's step on the device store: a slice of the uploaded permutation and one launch of ffwm_face_batch
Both as wall-clock time per batch over a window of --steps (A) / --steps-b (B) batches -- about half a second each -- that ends in
one synchronisation, the windows alternating for --pairs pairs, reported as median and min-max; B also as device time of the launch
alone inside a captured graph.  The acceptance condition of the record: B below A by more than the larger min-max spread.

    python tools/data_bench.py --rotation [--steps 64] [--out profiles/face_aug.txt]

measures the rotated batches of FaceLoader(rotation=True) the same way: A is host_batch with the epoch's angles (the stated
warpAffine in numpy, item by item), collate and copy; B is one launch of ffwm_face_batch_aug on slices of the uploaded index and
angle slots.  The device time of the rotated launch is reported beside the plain launch's, both inside captured graphs.  Which
staging route a block takes (LDS window or global taps) follows from the window's size and cannot be chosen from outside; at 128 x
128 under +-5 degrees every block stages its window in LDS (DESIGN.md has the routes timed against each other, from builds that
differ in the budget constant of csrc/face_batch.hip).
The GPU work runs in a child process under its own time limit; the parent never opens the GPU.  GPU only.
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
LIMIT = 300          # seconds for the child


def measure(args):
    import torch
    import face_data_cases as fc
    from ffwm_amd import data as fd
    B = args.batch
    c = fc.synthetic(64, 128, 128, 1024, seed=1)
    host = fd.FaceStore.from_arrays(c["images"], c["masks"], c["names"], c["lm_dicts"], rotation=args.rotation)
    dev = host.to(DEV)
    n = len(host)
    loader = fd.FaceLoader(dev, B, seed=0, rotation=True if args.rotation else None)
    order, angles = loader.draws(0)
    index = order.to(DEV)
    order = order.tolist()
    rot = loader.rotation
    slot = rot.slots(angles).to(DEV) if args.rotation else None
    angles = angles.tolist() if args.rotation else None
    # windows of about half a second each: B's batch takes ~1 % of A's
    starts, starts_b = ([B * (s % (n // B)) for s in range(k)] for k in (args.steps, args.steps_b))
    keep = {}

    def window_a():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for lo in starts:
            b = host.host_batch(order[lo:lo + B], angles[lo:lo + B] if args.rotation else None)
            keep["a"] = {k: v.to(DEV) for k, v in b.items() if k != "input_path"}
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / len(starts)

    bufs = [{}, {}]

    def launch(lo, out):
        if args.rotation:
            return dev.batch_rotated(index[lo:lo + B], slot[lo:lo + B], rot, out=out)
        return dev.batch(index[lo:lo + B], out=out)

    def window_b():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s, lo in enumerate(starts_b):
            bufs[s % 2].update(launch(lo, bufs[s % 2]))
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / len(starts_b)

    window_a(), window_b()          # allocations, the library's load
    lo = starts[-1]
    assert starts_b[-1] == lo
    same = all(torch.equal(keep["a"][k], bufs[(len(starts_b) - 1) % 2][k]) for k in keep["a"])
    print("# face batches: B = %d, 128 x 128, L = 1024, %d files (%d items, %.1f MiB on the device), device %s" % (
        B, len(host.names), n, dev.nbytes() / 2.0 ** 20, torch.cuda.get_device_name(0)))
    print("# A = host_batch%s + .to(device), B = one %s launch on the device store; wall-clock ms per batch over windows of %d (A) "
          "and %d (B) batches, %d alternating pairs" % (
              " with one angle of [-5, 5) per item" if args.rotation else "", "ffwm_face_batch_aug" if args.rotation else "ffwm_face_batch",
              len(starts), len(starts_b), args.pairs))
    print("the last batch of A and of B are %s" % ("equal bit for bit" if same else "DIFFERENT"))
    ms = {"A": [], "B": []}
    for _ in range(args.pairs):
        ms["A"].append(window_a())
        ms["B"].append(window_b())
    print(line("A (host_batch + copy)  ", ms["A"], "ms"))
    print(line("B (one launch)         ", ms["B"], "ms"))
    margin = statistics.median(ms["A"]) - statistics.median(ms["B"])
    worst = max(max(v) - min(v) for v in ms.values())
    print("A - B = %.3f ms against the larger min-max spread %.3f ms: B is %s; A / B = %.1f" % (
        margin, worst, "below A by more than the spread" if margin > worst else "NOT below A by more than the spread",
        statistics.median(ms["A"]) / statistics.median(ms["B"])))
    out = dict(bufs[0])
    replay = captured(lambda: launch(lo, out), 20)
    dev_us = [1e3 * replay() for _ in range(args.pairs)]
    print(line("B, device time of the launch in a captured graph", dev_us, "us"), flush=True)
    if args.rotation:
        replay = captured(lambda: dev.batch(index[lo:lo + B], out=out), 20)
        dev_us = [1e3 * replay() for _ in range(args.pairs)]
        print(line("the plain launch (ffwm_face_batch) beside it, likewise", dev_us, "us"), flush=True)
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256, help="batches per timed window of A")
    ap.add_argument("--steps-b", type=int, default=25600, help="batches per timed window of B (both a multiple of the 32 batches of the set)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rotation", action="store_true", help="the rotated batches of FaceLoader(rotation=True); --out defaults to profiles/face_aug.txt")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help="measure in this process (what the parent starts)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "face_aug.txt" if args.rotation else "face_dataset.txt")
    if args.pairs < 5:
        sys.exit("data_bench: at least five pairs")
    if args.child:
        import torch
        if not torch.cuda.is_available():
            sys.exit("data_bench: needs an MI355X; a CPU run measures nothing")
        sys.exit(measure(args))
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--pairs", str(args.pairs), "--steps", str(args.steps), "--steps-b", str(args.steps_b), "--batch", str(args.batch)] + (["--rotation"] if args.rotation else [])
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT, cwd=ROOT)
        text, status = r.stdout, r.returncode
        if status != 0:
            text += "data_bench: the measurement ended with status %d\n%s\n" % (status, r.stderr[-2000:])
    except subprocess.TimeoutExpired as e:
        text = (e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout or "") + "data_bench: passed its limit of %d s\n" % LIMIT
        status = 124
    print(text, end="", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.exit(status)


if __name__ == "__main__":
    main()
