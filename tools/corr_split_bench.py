"""The two correlation-maximum kernels side by side: one process, the same inputs, `--runs` runs of `--reps` launches each.

    python tools/corr_split_bench.py [--runs 3] [--reps 20] [--flowtrain STEPS]

Part 1: the profiler rows correlation_colmax (fp32 MFMA) and correlation_colmax_split (bf16 MFMA on hi/lo-split operands) at the
three scales of FlowNet pre-training, (B, N, C) = (6, 16384, 64), (6, 4096, 128), (6, 1024, 256), normalised random features; the
runs alternate between the kernels.  Per shape: mean, spread (max - min) of each, the speed-up, and its fraction of the MFMA-rate
ceiling 16/3.  Part 2: wall time of the fused correctness call (PerceptualCorrectness.calculate_loss forward + backward, fused=True)
per scale with each precision.  Part 3 (--flowtrain STEPS > 0): the FlowNetTrainer step with fused_correctness=True, each precision.
This is what profiles/correlation_split.txt records.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ffwm_amd import _lib, ops  # noqa: E402

DEV = "cuda:0"
ROW = {"fp32": "correlation_colmax", "bf16x3": "correlation_colmax_split"}


def row_ms(fn, row, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    _lib.prof_reset()
    _lib.prof_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    rows = _lib.prof_collect()
    _lib.prof_enable(False)
    assert rows[row]["launches"] == reps, rows.keys()
    return rows[row]["avg_ms"]


def wall_ms(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def fmt(v):
    return "[" + ", ".join("%.4f" % x for x in v) + "]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--flowtrain", type=int, default=0, help="time this many FlowNetTrainer steps per precision (0: skip)")
    args = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    print("# part 1: profiler rows, avg ms of %d launches, %d runs each, alternating" % (args.reps, args.runs))
    for (N, C) in ((16384, 64), (4096, 128), (1024, 256)):
        s = torch.randn(6, N, C, generator=g).to(DEV)
        t = torch.randn(6, C, N, generator=g).to(DEV)
        s = (s / (s.norm(dim=2, keepdim=True) + 1e-8)).contiguous()
        t = (t / (t.norm(dim=1, keepdim=True) + 1e-8)).contiguous()
        ms = {"fp32": [], "bf16x3": []}
        for _ in range(args.runs):
            for prec in ms:
                ms[prec].append(row_ms(lambda: ops.correlation_colmax(s, t, precision=prec), ROW[prec], args.reps))
        err = float((ops.correlation_colmax(s, t, precision="bf16x3") - ops.correlation_colmax(s, t)).abs().max())
        mean = {k: sum(v) / len(v) for k, v in ms.items()}
        spread = {k: max(v) - min(v) for k, v in ms.items()}
        speedup = mean["fp32"] / mean["bf16x3"]
        tf = 2.0 * 6 * N * N * C / 1e9
        print("(6,%d,%d) fp32   %s mean %.4f spread %.4f  %.1f TFLOP/s" % (N, C, fmt(ms["fp32"]), mean["fp32"], spread["fp32"], tf / mean["fp32"]))
        print("(6,%d,%d) bf16x3 %s mean %.4f spread %.4f  %.1f TFLOP/s (algorithmic)" % (N, C, fmt(ms["bf16x3"]), mean["bf16x3"], spread["bf16x3"],
                                                                                        tf / mean["bf16x3"]))
        print("(6,%d,%d) margin %.4f ms vs fp32 spread %.4f ms: %s; speed-up %.2fx = %.0f %% of the ceiling 16/3; max |bf16x3 - fp32| = %.2e"
              % (N, C, mean["fp32"] - mean["bf16x3"], spread["fp32"], "WINS" if mean["fp32"] - mean["bf16x3"] > spread["fp32"] else "does NOT win",
                 speedup, 100 * speedup / (16.0 / 3.0), err))
        del s, t
    print("# part 2: fused correctness call (calculate_loss fwd + bwd, with mask), wall ms of %d calls, %d runs each, alternating" % (args.reps, args.runs))
    from ffwm_amd.external_function import WarpNet
    from ffwm_amd.losses import PerceptualCorrectness
    mask = (torch.rand(6, 1, 128, 128, generator=g) < 0.6).float().to(DEV)
    for (C, S) in ((256, 32), (128, 64), (64, 128)):
        src = (torch.rand(6, C, S, S, generator=g) + 0.1).to(DEV)
        tgt = (torch.rand(6, C, S, S, generator=g) + 0.1).to(DEV)
        fl = (torch.rand(6, 2, S, S, generator=g) * 2.2 - 1.1).to(DEV).requires_grad_(True)
        ms = {"fp32": [], "bf16x3": []}
        mods = {}
        for prec in ms:
            mods[prec] = PerceptualCorrectness(None, WarpNet(), fused=True, corr_precision=prec)
            mods[prec].target_vgg, mods[prec].source_vgg = {"x": tgt}, {"x": src}

        def step(prec):
            fl.grad = None
            mods[prec].calculate_loss(fl, "x", mask, use_bilinear_sampling=True).backward()
        for _ in range(args.runs):
            for prec in ms:
                ms[prec].append(wall_ms(lambda: step(prec), args.reps))
        mfma = 6 * ((S * S + 127) // 128) >= 192
        for prec in ms:
            print("[6,%d,%d,%d] %-6s %s mean %.4f%s" % (C, S, S, prec, fmt(ms[prec]), sum(ms[prec]) / len(ms[prec]),
                                                      "" if mfma else "   (below the gate: bmm + max, whatever was asked)"))
        del src, tgt, fl
    if args.flowtrain > 0:
        print("# part 3: FlowNetTrainer(fused_correctness=True) eager step (no graph), batch 6, wall ms over %d steps, %d runs each, alternating" % (args.flowtrain, args.runs))
        from ffwm_amd import trainer
        trainers = {prec: trainer.FlowNetTrainer(DEV, seed=0, fused_correctness=True, corr_precision=prec) for prec in ("fp32", "bf16x3")}
        batch = trainer.synthetic_batch(6, torch.device(DEV), seed=1)
        ms = {"fp32": [], "bf16x3": []}
        for _ in range(args.runs):
            for prec in ms:
                ms[prec].append(wall_ms(lambda: trainers[prec].step(batch), args.flowtrain))
        for prec in ms:
            print("flowtrain step %-6s %s mean %.4f" % (prec, fmt(ms[prec]), sum(ms[prec]) / len(ms[prec])))


if __name__ == "__main__":
    main()
