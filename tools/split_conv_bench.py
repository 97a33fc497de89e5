"""What precision="bf16x3" (csrc/conv_winograd_gemm_split.hip: the Winograd GEMMs of the frozen 3 x 3 layers on the bf16 MFMA, hi / lo
split operands) gains or loses against the fp32 path, in ONE process, alternating:

    python tools/split_conv_bench.py --part layers [--out profiles/wino_gemm_split.txt]
    python tools/split_conv_bench.py --part e2e --append
    python tools/split_conv_bench.py --part memory --append

layers  every distinct routed shape of LightCNN-29 at a 128 px input and of netG at 128 x 128, batch 1 and 8, as device time inside a
        captured graph (20 calls per graph): leg A = the route the fp32 path gives the layer today, netG's bias + activation launch
        included where that route has one; leg B = the split route.  Five alternating pairs, median and min-max per leg.  LightCNN's
        mfm_tail launch follows both legs alike and is in neither.
e2e     FaceIdentifier and Frontalizer with "fp32" against "bf16x3" (graph=True), alternating, batch 1 and 8, the same statistics; and
        max |difference| of fake_F128 and of the feature, the cosine between the two features, whether the top-k indices agree.
memory  the bytes of split weights each network holds under "bf16x3".

Each part is one invocation, so that a caller can give each its own time limit.  Nothing gates on these numbers: they fill
SPLIT_EXCLUDED_LAYERS (a layer goes in when B is slower than A at BOTH batch sizes by more than the larger min-max spread) and the
documents.  GPU only: without a device the tool fails.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import torch  # noqa: E402

import fill  # noqa: E402
from abtime import captured  # noqa: E402
from frontalize_bench import time_leg  # noqa: E402

DEV = "cuda:0"
PAIRS = 5
GALLERY = 250


def alternate(leg_a, leg_b):
    """-> ([A's times], [B's times]) of PAIRS alternating measurements; a leg is a callable that returns one time."""
    ta, tb = [], []
    for _ in range(PAIRS):
        ta.append(leg_a())
        tb.append(leg_b())
    return ta, tb


def stats(v, scale=1.0, digits=1):
    return "median %.*f [%.*f .. %.*f]" % (digits, scale * statistics.median(v), digits, scale * min(v), digits, scale * max(v))


def verdict(ta, tb):
    """+1: B faster than A beyond the larger min-max spread, -1: slower beyond it, 0: inside it."""
    d = statistics.median(ta) - statistics.median(tb)
    spread = max(max(ta) - min(ta), max(tb) - min(tb))
    return (1 if d > spread else -1 if d < -spread else 0), d, spread


def networks():
    from ffwm_amd import nets
    flow = fill.fill_module(nets.FlowNet(64)).to(DEV).eval()
    netG = fill.fill_module(nets.FFWM(sn=True)).to(DEV).eval()
    fill.boost_output_gain(netG)
    torch.manual_seed(29)
    light = nets.LightCNN29().to(DEV).eval()          # default initialisation: timing does not depend on the weights
    return flow, netG, light


# ---------------------------------------------------------------------------------------------------- (a) per layer
def lightcnn_layers(light, out):
    from ffwm_amd import ffwm_eval, identity_eval
    fp32, split = identity_eval.FoldedLightCNN(light), identity_eval.FoldedLightCNN(light, precision="bf16x3")

    class Recorder(identity_eval._HipExec):
        def __init__(self, owner):
            identity_eval._HipExec.__init__(self, owner)
            self.inputs = {}

        def layer(self, name, x, residual=None, pool=False):
            self.inputs[name] = x
            return identity_eval._HipExec.layer(self, name, x, residual, pool)

    table = {}
    for B in (1, 8):
        x = fill.image(B, 1, 128, 128, "lightcnn_in").to(DEV)
        fp32.arena.begin(x.device)
        rec = Recorder(fp32)
        with torch.no_grad():
            fp32._run(rec, x)
        torch.cuda.synchronize()
        seen = {}
        for name in fp32.layer_names():
            L, xin = fp32.layers[name], rec.inputs[name]
            if not ffwm_eval.split_route_ok(L, xin):
                continue
            key = (L.w.shape[1], L.w.shape[0], xin.shape[2], xin.shape[3])
            seen.setdefault(key, []).append(name)
        for key, names in seen.items():
            name = names[0]
            xin, route = rec.inputs[name].clone(), fp32._route(names[0], rec.inputs[names[0]])

            def leg(owner, r, name=name, xin=xin):
                def fn():
                    owner.arena.begin(xin.device)
                    return identity_eval.run_conv(owner, name, xin, r)
                return captured(torch.no_grad()(fn), 20)
            ga, gb = leg(fp32, route), leg(split, "winograd_split")
            table.setdefault(key, {"names": names})[B] = (route,) + alternate(lambda: ga(1), lambda: gb(1))
    report("LightCNN-29, 128 px input", table, out)


def netg_layers(netG, out):
    from ffwm_amd import ffwm_eval
    fp32, split = ffwm_eval.FoldedFFWM(netG), ffwm_eval.FoldedFFWM(netG, precision="bf16x3")

    class Recorder(ffwm_eval._HipExec):
        def __init__(self, owner):
            ffwm_eval._HipExec.__init__(self, owner)
            self.inputs = {}

        def conv(self, name, x, act, slope=0.2):
            self.inputs[name] = (x, act, slope)
            return ffwm_eval._HipExec.conv(self, name, x, act, slope)

    table = {}
    for B in (1, 8):
        img = fill.image(B, 3, 128, 128, "netG_in").to(DEV)
        flows = [fill.flow_field(B, s, s, "netG_flow%d" % s).to(DEV) for s in (32, 64, 128)]
        fp32.arena.begin(img.device)
        rec = Recorder(fp32)
        with torch.no_grad():
            fp32._run(rec, img, flows, True)
        torch.cuda.synchronize()
        seen = {}
        for name, (xin, act, slope) in rec.inputs.items():
            L = fp32.layers[name]
            if not ffwm_eval.split_route_ok(L, xin):
                continue
            key = (L.w.shape[1], L.w.shape[0], xin.shape[2], xin.shape[3], "lrelu" if act else "bias")
            seen.setdefault(key, []).append(name)
        for key, names in seen.items():
            name = names[0]
            xin, act, slope = rec.inputs[name]
            xin = xin.contiguous().clone()
            route = fp32._route(name, xin, act)

            def leg(owner, name=name, xin=xin, act=act, slope=slope):
                def fn():
                    owner.arena.begin(xin.device)
                    return ffwm_eval._HipExec(owner).conv(name, xin, act, slope)
                return captured(torch.no_grad()(fn), 20)
            ga, gb = leg(fp32), leg(split)
            table.setdefault(key, {"names": names})[B] = (route,) + alternate(lambda: ga(1), lambda: gb(1))
    report("netG, 128 x 128 images (layers past the 256 MiB workspace condition keep their fp32 route and are not listed at that batch)",
           table, out)


def report(title, table, out):
    out("## %s: device us per call, 20 calls inside one captured graph, %d alternating pairs; A = today's fp32 route, B = split" % (title, PAIRS))
    exclude = []
    for key, row in table.items():
        cells, slower = [], []
        for B in (1, 8):
            if B not in row:
                cells.append("batch %d: not routed (workspace)" % B)
                continue
            route, ta, tb = row[B]
            v, d, spread = verdict(ta, tb)
            slower.append(v < 0)
            cells.append("batch %d A %s %s  B %s  A / B %.2f (%s)" % (B, route, stats(ta, 1e3), stats(tb, 1e3), statistics.median(ta) / statistics.median(tb),
                                                                     "B faster" if v > 0 else "B SLOWER" if v < 0 else "inside the spread"))
        shape = "%d -> %d at %d x %d%s" % (key[0], key[1], key[2], key[3], " " + key[4] if len(key) > 4 else "")
        out("%-28s %s   [%s]" % (shape, "   ".join(cells), ", ".join(row["names"])))
        if len(slower) == 2 and all(slower):
            exclude += row["names"]
    out("# slower at BOTH batch sizes beyond the spread (the exclusion rule): %s" % (", ".join(exclude) or "none"))


# ---------------------------------------------------------------------------------------------------- (b) end to end
def end_to_end(flow, netG, light, out, seconds):
    from ffwm_amd import FaceIdentifier, Frontalizer
    out("## end to end, graph=True, ms per call from device events over windows of >= %.2f s, %d alternating pairs; A = fp32, B = bf16x3" % (seconds, PAIRS))
    fronts = {p: Frontalizer(flow, netG, graph=True, precision=p) for p in ("fp32", "bf16x3")}
    idents = {p: FaceIdentifier(flow, netG, light, graph=True, topk=1, precision=p) for p in ("fp32", "bf16x3")}
    gallery = torch.cat([fill.image(50, 1, 128, 128, "gallery_%d" % i) for i in range(GALLERY // 50)], 0).to(DEV)
    for ident in idents.values():
        ident.set_gallery(["%04d" % i for i in range(GALLERY)], gallery)
    for B in (1, 8):
        img = fill.image(B, 3, 128, 128, "eval_img_S").to(DEV)
        for what, objs in (("Frontalizer", fronts), ("FaceIdentifier", idents)):
            for _ in range(3):
                for o in objs.values():
                    o(img)
            torch.cuda.synchronize()
            ta, tb = alternate(lambda: time_leg(lambda: objs["fp32"](img), seconds)[0], lambda: time_leg(lambda: objs["bf16x3"](img), seconds)[0])
            v, d, spread = verdict(ta, tb)
            out("batch %d  %-14s A %s ms  B %s ms  A - B = %.3f ms against the larger spread %.3f: %s; A / B = %.3f"
                % (B, what, stats(ta, digits=3), stats(tb, digits=3), d, spread,
                   "B faster beyond the spread" if v > 0 else "B SLOWER beyond the spread" if v < 0 else "inside the spread",
                   statistics.median(ta) / statistics.median(tb)))
        ra, rb = idents["fp32"](img), idents["bf16x3"](img)
        fa, fb = ra.feature.double(), rb.feature.double()
        out("batch %d  max |fake_F128 difference| %.3e (values in [0, 1]); max |feature difference| %.3e of max |feature| %.3e; cosine between "
            "the features min %.8f; top-%d indices agree: %s; top-1 agree: %s"
            % (B, (ra.frontal.fake_F128 - rb.frontal.fake_F128).abs().max().item(), (fa - fb).abs().max().item(), fa.abs().max().item(),
               torch.cosine_similarity(fa, fb, dim=1).min().item(), ra.top_idx.shape[1], bool(torch.equal(ra.top_idx, rb.top_idx)),
               bool(torch.equal(ra.top_idx[:, 0], rb.top_idx[:, 0]))))
        for p, o in (("netG", fronts["bf16x3"]), ("LightCNN", idents["bf16x3"])):
            plan = o.plan(B, 128, 128)
            kinds = {}
            for _, k in plan:
                kinds[k] = kinds.get(k, 0) + 1
            out("batch %d  %s launches under bf16x3 from plan(): %s" % (B, p, ", ".join("%s %d" % kv for kv in sorted(kinds.items()))))


# ---------------------------------------------------------------------------------------------------- (c) weight memory
def memory(flow, netG, light, out):
    from ffwm_amd import FaceIdentifier
    out("## split weights held under bf16x3 after one forward at batch 1 and one at batch 8 (made at a layer's first eager call, kept)")
    ident = FaceIdentifier(flow, netG, light, graph=False, precision="bf16x3")
    for B in (1, 8):
        ident(fill.image(B, 3, 128, 128, "eval_img_S").to(DEV))
    for name, owner in (("netG", ident.front.netG), ("LightCNN-29", ident.net)):
        split = sum(u.numel() * 4 for u in owner._split_u.values())
        own = sum(owner.layers[n].w.numel() * 4 for n in owner._split_u)
        every = sum(L.w.numel() * 4 for L in owner.layers.values())
        out("%-12s %d layers, split U %.2f MB beside their fp32 weights of %.2f MB (all convolution weights of the network: %.2f MB)"
            % (name, len(owner._split_u), split / 1e6, own / 1e6, every / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("layers", "e2e", "memory"), required=True)
    ap.add_argument("--seconds", type=float, default=0.5, help="length of one timed window (e2e)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wino_gemm_split.txt"))
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("split_conv_bench: needs an MI355X; a CPU run measures nothing")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if not args.append:
        open(args.out, "w").close()

    def out(s=""):
        print(s, flush=True)
        with open(args.out, "a") as f:
            f.write(s + "\n")

    flow, netG, light = networks()
    if args.part == "layers":
        out("# precision=\"bf16x3\" against \"fp32\": tools/split_conv_bench.py, float32 tensors, device %s" % torch.cuda.get_device_name(0))
        lightcnn_layers(light, out)
        netg_layers(netG, out)
    elif args.part == "e2e":
        end_to_end(flow, netG, light, out, args.seconds)
    else:
        memory(flow, netG, light, out)


if __name__ == "__main__":
    main()
