"""The result images of one test batch, two ways in ONE process, alternating:

    python tools/visuals_bench.py [--reps 5] [--seconds 0.5] [--out profiles/visuals.txt]

The visuals are test_ffwm.py's three (img_S, img_F, fake_F128) plus flow_F128 and att, 128 x 128, batch 1 and batch 8, seeded random
float32 tensors on the device (the conversion's cost does not depend on what the picture shows; att takes a seeded random palette,
the library ships none).

(A) what a user of Frontalizer had before ffwm_amd/visuals.py: per label and image `tensor[idx].cpu().float().numpy()` and the numpy
    restatement of the reference's converter (ffwm_amd.visuals.tensor2im / tensor2flow / tensor2att) -- the reference's own path;
(B) ffwm_amd.visuals.render (one ffwm_visuals call: two launches) and one device-to-host copy of the uint8 sheet (to_host).

Both end with the pictures as numpy arrays on the host, so a leg is timed with the host clock around calls that end synchronised; a
window holds as many calls as fill --seconds, the legs alternate A / B and each is reported as median and min-max over --reps
repetitions.  The device time of the render call alone is taken from device events around replays of a graph captured with
ffwm_amd/graphs.py.  The comparison is against A only; nothing here is a gate.  GPU only: without a device the tool fails.
"""
import argparse
import collections
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"


def time_host(fn, seconds):
    """ms per call by the host clock; fn ends synchronised (its result is on the host)."""
    t0 = time.perf_counter()
    for _ in range(3):
        fn()
    per = max((time.perf_counter() - t0) / 3, 1e-6)
    n = max(3, int(seconds / per) + 1)
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    return (time.perf_counter() - t0) * 1e3 / n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=0.5, help="length of one timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "visuals.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("visuals_bench: needs an MI355X; a CPU run measures nothing")

    from ffwm_amd import graphs, ops
    from ffwm_amd import visuals as V

    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    palette = np.random.RandomState(21).randint(0, 256, size=(256, 3)).astype(np.uint8)
    palette_dev = torch.from_numpy(palette).to(DEV)

    def batch(B):
        g = torch.Generator().manual_seed(100 + B)
        v = collections.OrderedDict()
        for label, C in (("img_S", 3), ("img_F", 3), ("fake_F128", 3)):
            v[label] = torch.rand(B, C, 128, 128, generator=g).to(DEV)
        v["flow_F128"] = (torch.rand(B, 2, 128, 128, generator=g) * 2 - 1).to(DEV)
        v["att"] = torch.rand(B, 1, 128, 128, generator=g).to(DEV)
        return v

    def leg_a(v):
        res = collections.OrderedDict()
        for label, x in v.items():
            kind = V.kind_of(label)
            fn = {V.IMAGE: V.tensor2im, V.MASK: V.tensor2mask, V.FLOW: V.tensor2flow}.get(kind)
            res[label] = [V.tensor2att(x, palette, idx=i) if kind == V.PALETTE else fn(x, idx=i) for i in range(x.shape[0])]
        return res

    def leg_b(v):
        return V.to_host(V.render(v, palette=palette_dev))

    out("# result images: img_S, img_F, fake_F128, flow_F128, att at 128 x 128, float32 in, uint8 RGB out, device %s"
        % torch.cuda.get_device_name(0))
    out("# A = per label and image tensor[idx].cpu().float().numpy() + the numpy restatement of the reference's converter")
    out("# B = visuals.render (one ffwm_visuals call) + one copy of the uint8 sheet to the host")
    out("# per leg: ms per batch of visuals by the host clock (both legs end on the host) over a window of >= %.2f s; %d repetitions, "
        "alternating A / B" % (args.seconds, args.reps))
    for B in (1, 8):
        v = batch(B)
        for _ in range(2):
            a, b = leg_a(v), leg_b(v)
        differ = {label: int((np.stack(a[label]) != b[label]).any(axis=-1).sum()) for label in v}
        out("batch %d  pixels where A and B differ: %s" % (B, ", ".join("%s %d" % kv for kv in differ.items())))
        ms, calls = {"A": [], "B": []}, {}
        for _ in range(args.reps):
            for name, fn in (("A", leg_a), ("B", leg_b)):
                t, n = time_host(lambda: fn(v), args.seconds)
                ms[name].append(t)
                calls[name] = n
        med = {k: statistics.median(x) for k, x in ms.items()}
        for k in ("A", "B"):
            out("batch %d  %s  median %.3f ms  min %.3f  max %.3f  (%d calls per window)  runs [%s]"
                % (B, k, med[k], min(ms[k]), max(ms[k]), calls[k], ", ".join("%.3f" % x for x in ms[k])))
        margin, worst = med["A"] - med["B"], max(max(x) - min(x) for x in ms.values())
        out("batch %d  A - B = %.3f ms against the larger min-max spread %.3f ms: %s; A / B = %.2f"
            % (B, margin, worst, "B is faster beyond the spread" if margin > worst else
               ("no difference beyond the spread" if margin >= -worst else "B is SLOWER beyond the spread"), med["A"] / med["B"]))
        # the render call alone, inside a captured graph: device events around replays
        items = [(x, V.kind_of(label), palette_dev if V.kind_of(label) == V.PALETTE else None) for label, x in v.items()]
        graphs.warm_up(lambda: ops.visuals(items), 2, sync=True)
        g, sheets = graphs.capture(lambda: ops.visuals(items))
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        per = []
        for _ in range(args.reps):
            n = 200
            start.record()
            for _ in range(n):
                g.replay()
            stop.record()
            stop.synchronize()
            per.append(start.elapsed_time(stop) * 1e3 / n)
        same = all((s.cpu().numpy() == b[label]).all() for s, label in zip(sheets, v))
        nbytes = sum(x.numel() * 4 + x.shape[0] * 128 * 128 * 3 for x in v.values())
        out("batch %d  render inside a captured graph (2 launches), device events over 200 back-to-back replays: median %.1f us  min %.1f  "
            "max %.1f per replay; %d bytes read and written per call; replayed sheets equal B's: %s"
            % (B, statistics.median(per), min(per), max(per), nbytes, same))


if __name__ == "__main__":
    main()
