"""What loss_precision="bf16x3" (FFWMTrainer; conv.WGS_TABLE: the frozen 3 x 3 layers of VGG19 and LightCNN-29 with their Winograd GEMMs
on the bf16 MFMA, hi / lo split operands, forward and data gradient) gains or loses against the step as it is, in ONE process,
alternating:

    python tools/split_loss_bench.py --part layers [--out profiles/wino_split_train.txt] [--classes 96x384,...]
    python tools/split_loss_bench.py --part step --append

layers  every distinct frozen 3 x 3 / stride-1 shape of the train step's loss networks at batch 8 (tools/wino_gemm_layers.py lists
        them by running the networks), forward and data gradient, the data gradient under a ReLU mask where the network has one
        (VGG19), as device time inside a captured graph: 20 calls per graph, median of 7 replays, five alternating pairs.
        leg A = the route the shape takes today: the fp32 GEMM route where conv.WG_TABLE names it (one call, epilogue / mask inside),
        else the vendor convolution + its epilogue launch (data gradient: aten::threshold_backward + the vendor data gradient).  A
        shape that conv.winograd_ok sends to conv_winograd.hip is listed and left there.
        leg B = the split route (ops.conv3x3_wg_split_frozen).
        A (class, direction, T) is a WINNER only where B's median is below A's by more than the larger min-max spread of the two;
        the last lines list winners and losers per (C, K): conv.WGS_TABLE holds the ranges of the winners.
step    the captured train step at batch 8: two trainers of one seed, loss_precision="fp32" and "bf16x3", alternating, five pairs of
        timed windows, medians and min-max spreads; and the loss values of each trainer's first replayed step side by side.

Each part is one invocation, so that a caller can give each its own time limit.  Nothing gates on these numbers: they fill
conv.WGS_TABLE and the documents.  GPU only: without a device the tool fails.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from abtime import captured  # noqa: E402
from frontalize_bench import time_leg  # noqa: E402
from wino_gemm_layers import step_shapes  # noqa: E402

DEV = "cuda:0"
CALLS, REPLAYS, PAIRS = 20, 7, 5


def leg(fn):
    """-> a callable that returns the median microseconds per call of REPLAYS replays of a graph of CALLS calls."""
    fn()
    torch.cuda.synchronize()
    replay = captured(fn, CALLS)
    return lambda: 1000.0 * replay(REPLAYS, stat=statistics.median)


def alternate(leg_a, leg_b):
    ta, tb = [], []
    for _ in range(PAIRS):
        ta.append(leg_a())
        tb.append(leg_b())
    return ta, tb


def verdict(ta, tb):
    """+1: B faster than A beyond the larger min-max spread, -1: slower beyond it, 0: inside it."""
    d = statistics.median(ta) - statistics.median(tb)
    spread = max(max(ta) - min(ta), max(tb) - min(tb))
    return (1 if d > spread else -1 if d < -spread else 0)


def layer_legs(net, B, C, H, W, K):
    """-> {direction: (name of leg A's route, leg A, leg B)} for one shape."""
    from ffwm_amd import conv, ops
    relu = net == "vgg"
    x = torch.randn(B, C, H, W, device=DEV)
    w = torch.nn.Parameter(torch.randn(K, C, 3, 3, device=DEV) / (9 * C) ** 0.5, requires_grad=False)
    b = torch.randn(K, device=DEV)
    go = torch.randn(B, K, H, W, device=DEV)
    y = torch.relu(torch.randn(B, K, H, W, device=DEV)) if relu else None
    T = B * ((H + 1) // 2) * ((W + 1) // 2)
    wd = w.detach()
    Sf, Sb = ops.conv3x3_wg_split_weights(wd), ops.conv3x3_wg_split_weights(wd, data_gradient=True)
    epi = "relu" if relu else "mfm"
    out = {}
    if conv.wg_route(T, w, "fp32", 0) == "fp32":
        Uf = ops.conv3x3_wg_weights(wd, False)
        out["fwd"] = ("fp32-gemm", lambda: ops.conv3x3_wg(x, Uf, b, epi), lambda: ops.conv3x3_wg_split_frozen(x, Sf, b, epi))
        if not relu:          # under autograd LightCNN keeps the pre-activation: the bare convolution, then csrc/mfm.hip's launch
            out["fwd+grad"] = ("fp32-gemm", lambda: ops.mfm_forward(ops.conv3x3_wg(x, Uf, None, "none", K=K), b),
                               lambda: ops.mfm_forward(ops.conv3x3_wg_split_frozen(x, Sf, None, "none", K=K), b))
    else:
        tail = ops.bias_relu_forward if relu else ops.mfm_forward
        out["fwd"] = ("vendor", lambda: tail(F.conv2d(x, w, None, 1, 1), b), lambda: ops.conv3x3_wg_split_frozen(x, Sf, b, epi))
        if not relu:
            out["fwd+grad"] = ("vendor", out["fwd"][1], lambda: ops.mfm_forward(ops.conv3x3_wg_split_frozen(x, Sf, None, "none", K=K), b))
    if conv.wg_route(T, w, "fp32", 1) == "fp32":
        Ub = ops.conv3x3_wg_weights(wd, True)
        out["dgrad"] = ("fp32-gemm", lambda: ops.conv3x3_wg(go, Ub, None, "none", relu_mask=y, K=C),
                        lambda: ops.conv3x3_wg_split_frozen(go, Sb, None, "none", relu_mask=y, K=C))
    else:
        def vendor_dgrad():
            g = torch.ops.aten.threshold_backward(go, y, 0) if relu else go
            return torch.ops.aten.convolution_backward(g, x, wd, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [True, False, False])[0]
        out["dgrad"] = ("vendor", vendor_dgrad, lambda: ops.conv3x3_wg_split_frozen(go, Sb, None, "none", relu_mask=y, K=C))
    return out


def part_layers(args):
    from ffwm_amd import conv, miopen_tuning, nets
    miopen_tuning.install()
    lines = ["# tools/split_loss_bench.py --part layers: %d calls per captured graph, median of %d replays, %d alternating pairs; "
             "microseconds per call, median [min .. max] of the pairs" % (CALLS, REPLAYS, PAIRS),
             "# A = the route of the shape today (fp32-gemm: conv.WG_TABLE's three launches; vendor: convolution + epilogue launch), "
             "B = the split route; the data gradient of vgg under a ReLU mask",
             "# WINNER: median B < median A - max(spread A, spread B); loser: the other way round; inside: neither",
             "%-9s %3s %4s %3s %3s %4s %5s %-8s %-9s %24s %24s  %s" % ("net", "B", "C", "H", "W", "K", "T", "dir", "A is", "A", "B", "")]
    table = {}
    for net, B, C, H, W, K in step_shapes():
        T = B * ((H + 1) // 2) * ((W + 1) // 2)
        if T > args.max_tiles or min(C, K) < args.min_channels:
            continue
        if args.classes and (C, K) not in args.classes:
            continue
        probe = torch.empty(B, C, H, W, device=DEV)
        # (nets.mfm asks conv.winograd_ok only under FFWM_WINOGRAD_MFM=1: LightCNN's layers do not reach the large-plane kernel today)
        if (net == "vgg" or nets._WINOGRAD_MFM) and conv.winograd_ok(probe, torch.empty(K, C, 3, 3, device=DEV), 1 if net == "vgg" else 0):
            lines.append("%-9s %3d %4d %3d %3d %4d %5d left with conv_winograd.hip (the large-plane kernel), not measured" % (net, B, C, H, W, K, T))
            continue
        for d, (name, a, b) in layer_legs(net, B, C, H, W, K).items():
            ta, tb = alternate(leg(a), leg(b))
            v = verdict(ta, tb)
            cell = lambda t: "%7.1f [%6.1f .. %6.1f]" % (statistics.median(t), min(t), max(t))
            lines.append("%-9s %3d %4d %3d %3d %4d %5d %-8s %-9s %24s %24s  %s" % (
                net, B, C, H, W, K, T, d, name, cell(ta), cell(tb), {1: "WINNER", 0: "inside", -1: "loser"}[v]))
            print(lines[-1], flush=True)
            table.setdefault((C, K), {}).setdefault(d, []).append((T, net, v))
    lines.append("# per (C, K): T that won / T that did not, forward (under autograd where the network has such a call: fwd+grad) | data gradient")
    for ck, dirs in sorted(table.items()):
        cells = []
        for d in ("fwd", "fwd+grad", "dgrad"):
            got = sorted(set((t, n, v) for t, n, v in dirs.get(d, [])))
            cells.append("%s %s / %s" % (d, [(t, n) for t, n, v in got if v > 0], [(t, n) for t, n, v in got if v <= 0]))
        lines.append("#   %-10s: %s" % (ck, " | ".join(cells)))
    return lines


def part_step(args):
    from ffwm_amd import conv, trainer
    torch.backends.cudnn.benchmark = False
    batch = trainer.synthetic_batch(args.batch, DEV, seed=1)
    made, first = {}, {}
    for p in ("fp32", "bf16x3"):
        t = trainer.FFWMTrainer(DEV, seed=0, capturable=True, loss_precision=p)
        t.capture(batch, warmup=3)
        first[p] = {k: float(v) for k, v in t.step(batch, batch_increment=0).items()}
        torch.cuda.synchronize()
        made[p] = t
    routed = sum(1 for net in (made["bf16x3"].vgg, made["bf16x3"].lightCNN) for m in net.modules()
                 if any(isinstance(k, str) and k != "key" for k in m.__dict__.get("_wg_frozen", {})))
    ta, tb = [], []
    for _ in range(PAIRS):
        ta.append(time_leg(lambda: made["fp32"].step(batch, batch_increment=0), args.seconds)[0])
        tb.append(time_leg(lambda: made["bf16x3"].step(batch, batch_increment=0), args.seconds)[0])
    v = verdict(ta, tb)
    cell = lambda t: "median %.3f [%.3f .. %.3f] spread %.3f" % (statistics.median(t), min(t), max(t), max(t) - min(t))
    lines = ["# tools/split_loss_bench.py --part step: the captured train step, batch %d, two trainers of one seed, %d alternating pairs of "
             "%.1f s windows, ms per step" % (args.batch, PAIRS, args.seconds),
             "# conv.WGS_TABLE at this measurement: %r" % (conv.WGS_TABLE,),
             "# layers of the loss networks that hold split weights under bf16x3: %d (%.1f MiB of transformed weights against %.1f MiB under fp32)" % (
                 routed, made["bf16x3"].wg_weight_bytes / 2 ** 20, made["fp32"].wg_weight_bytes / 2 ** 20),
             "step loss_precision=fp32    %s" % cell(ta),
             "step loss_precision=bf16x3  %s" % cell(tb),
             "step verdict: %s (difference of the medians %.3f ms, larger spread %.3f ms)" % (
                 {1: "bf16x3 faster beyond the spread", 0: "inside the spread", -1: "bf16x3 slower beyond the spread"}[v],
                 statistics.median(ta) - statistics.median(tb), max(max(ta) - min(ta), max(tb) - min(tb))),
             "# loss values of each trainer's first replayed step (one seed, one batch): name, fp32, bf16x3"]
    for k in sorted(first["fp32"]):
        lines.append("loss %-12s %.9g  %.9g" % (k, first["fp32"][k], first["bf16x3"][k]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["layers", "step"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wino_split_train.txt"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--max-tiles", type=int, default=2048, help="skip planes with more 2 x 2 tiles (the large-plane kernel's)")
    ap.add_argument("--min-channels", type=int, default=64)
    ap.add_argument("--classes", type=lambda v: [tuple(int(n) for n in ck.split("x")) for ck in v.split(",")], default=None,
                    help="layers: only these classes, as CxK[,CxK...] (default: all)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=1.0, help="length of one timed window of the step")
    args = ap.parse_args()
    lines = part_layers(args) if args.part == "layers" else part_step(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
