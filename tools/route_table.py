#!/usr/bin/env python3
"""Which kernels, with which launch geometry, does a fixed list of ffwm_amd.ops calls get?

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/route_table.py --labels DIR/labels.txt
    python tools/route_table.py --fold DIR DIR/labels.txt > routes.txt        (no GPU: folds the trace into one line per dispatch)
    python tools/route_table.py --scopes                                      (second pass, profiler on: LaunchScope coverage)

Two trees route alike when their folded files are identical.  Every call is preceded by one torch.bitwise_xor launch: the fold
recognises it in the trace and moves on to the next label; the inputs of a call are made before its marker.
"""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "ffwm_amd", "csrc")


def calls():
    """-> [(label, {option: value}, thunk)]; the thunk makes its inputs and returns the function that issues the library calls."""
    import torch
    from ffwm_amd import ops
    dev = "cuda:0"
    out = []

    def rnd(*shape, dtype=torch.float32, lo=0.0, hi=1.0):
        return (torch.rand(*shape, dtype=dtype, device=dev) * (hi - lo) + lo)

    def add(label, opts, make):
        out.append((label, opts, make))

    # ---------------------------------------------------------------- block_extractor
    def be(B, C, H, W, k, dtype=torch.float32, fwd=True, src=True, flow=True, strided=False):
        def make():
            s, f = rnd(B, C, H, W, dtype=dtype), rnd(B, 2, H, W, dtype=dtype, lo=-2, hi=2)
            go = rnd(B, C, k * H, k * W, dtype=dtype)
            if strided:
                go = rnd(B, C, k * W, k * H, dtype=dtype).transpose(2, 3)
            gs = torch.zeros_like(s) if src else None
            gf = torch.zeros_like(f) if flow else None

            def run():
                if fwd:
                    ops.block_extractor_forward(s, f, k)
                if src or flow:
                    ops.block_extractor_backward(s, f, go, k, gs, gf)
            return run
        return make

    for k in range(1, 9):
        add("be k%d 32x48" % k, {}, be(2, 8, 32, 48, k))
    add("be k3 32x48 f64", {}, be(2, 8, 32, 48, 3, torch.float64))
    add("be k3 160x160 f64", {}, be(1, 4, 160, 160, 3, torch.float64))
    for k in (1, 2, 3, 4, 5):
        add("be k%d 160x160" % k, {}, be(1, 8, 160, 160, k))
    add("be k3 160x160 src only", {}, be(1, 8, 160, 160, 3, fwd=False, flow=False))
    add("be k3 160x160 flow only", {}, be(1, 8, 160, 160, 3, fwd=False, src=False))
    add("be k3 32x48 src only", {}, be(2, 8, 32, 48, 3, fwd=False, flow=False))
    add("be k3 32x48 flow only", {}, be(2, 8, 32, 48, 3, fwd=False, src=False))
    add("be k3 32x48 strided", {}, be(2, 8, 32, 48, 3, fwd=False, strided=True))
    add("be k3 32x48 strided f64", {}, be(2, 8, 32, 48, 3, torch.float64, fwd=False, strided=True))
    for v in (1, 2, 9):
        add("be k3 160x160 fwd", {"be_fwd_variant": v}, be(1, 8, 160, 160, 3, src=False, flow=False))
        add("be k6 32x48 fwd", {"be_fwd_variant": v}, be(2, 8, 32, 48, 6, src=False, flow=False))
    for v in (1, 2, 4):
        add("be k3 160x160 fwd", {"rows_per_thread": v}, be(1, 8, 160, 160, 3, src=False, flow=False))
    add("be k3 1024x1024 fwd (nt stores)", {}, be(1, 8, 1024, 1024, 3, src=False, flow=False))
    for v in (1, 2, 3, 9):
        add("be k3 160x160 bwd", {"be_bwd_variant": v}, be(1, 8, 160, 160, 3, fwd=False))
        add("be k3 32x48 bwd", {"be_bwd_variant": v}, be(2, 8, 32, 48, 3, fwd=False))
    for opts in ({"be_bwd_halo": 8}, {"be_bwd_halo": 8, "be_bwd_variant": 2}, {"be_bwd_rows": 64, "be_bwd_variant": 2},
                 {"be_bwd_rows": 64, "be_bwd_variant": 2, "be_bwd_halo": 8}, {"be_bwd_rows": 64}, {"be_bwd_fixed": 2},
                 {"be_bwd_fixed": 2, "be_bwd_halo": 8}, {"be_bwd_flush": 1}, {"channel_slab": 8}, {"channel_slab": 2},
                 {"xcd_remap": 0}, {"scatter_variant": 1}):
        add("be k3 160x160 bwd", opts, be(1, 8, 160, 160, 3, fwd=False))
    add("be k2 160x160 bwd", {"be_bwd_rows": 64, "be_bwd_variant": 2}, be(1, 8, 160, 160, 2, fwd=False))
    add("be k3 32x48", {"scatter_variant": 1}, be(2, 8, 32, 48, 3))
    add("be k3 32x48", {"channel_slab": 2}, be(2, 8, 32, 48, 3))
    add("be k3 16x16 many channels (plane kernel, several channels per block)", {}, be(8, 512, 16, 16, 3, fwd=False))

    # ---------------------------------------------------------------- block attention
    def ba(B, C, H, W, k, dtype=torch.float32, fwd=True, src=True, rest=True):
        def make():
            s, f = rnd(B, C, H, W, dtype=dtype), rnd(B, 2, H, W, dtype=dtype, lo=-2, hi=2)
            w = torch.softmax(rnd(B, k * k, H, W, dtype=dtype), 1)
            go = rnd(B, C, H, W, dtype=dtype)
            gs = torch.zeros_like(s) if src else None
            gf, gw = (torch.zeros_like(f), torch.zeros_like(w)) if rest else (None, None)

            def run():
                if fwd:
                    ops.block_attention_forward(s, f, w, k)
                if src or rest:
                    ops.block_attention_backward(s, f, w, go, k, gs, gf, gw)
            return run
        return make

    for shape in ((2, 8, 32, 48), (1, 16, 128, 128), (2, 64, 160, 160)):
        name = "ba k3 %dx%dx%dx%d" % shape
        add(name, {}, ba(*shape, 3))
        for v in (0, 2, 3, 4):
            add(name + " fwd", {"ba_fwd_pix": v}, ba(*shape, 3, src=False, rest=False))
        for v in (1, 2):
            add(name + " bwd", {"ba_bwd_fused": v}, ba(*shape, 3, fwd=False))
        for v in (0, 1, 2, 3, 5):
            add(name + " bwd", {"ba_bwd_pix": v}, ba(*shape, 3, fwd=False))
    add("ba k3 32x48 src only", {}, ba(2, 8, 32, 48, 3, fwd=False, rest=False))
    add("ba k3 32x48 flow+weights only", {}, ba(2, 8, 32, 48, 3, fwd=False, src=False))
    add("ba k3 32x48 f64", {}, ba(2, 8, 32, 48, 3, torch.float64))
    add("ba k2 32x48", {}, ba(2, 8, 32, 48, 2))
    add("ba k3 32x48 generic", {"be_fwd_variant": 9, "be_bwd_variant": 9}, ba(2, 8, 32, 48, 3))
    add("ba k3 32x48", {"xcd_remap": 0}, ba(2, 8, 32, 48, 3))
    # values past the documented ones take the first configuration of their list
    for opts in ({"ba_bwd_pix": 6}, {"ba_bwd_pix": 9}, {"ba_bwd_fused": 0}, {"ba_bwd_fused": 4}, {"ba_fwd_pix": 5}):
        add("ba k3 2x64x160x160 past the list", opts, ba(2, 64, 160, 160, 3))

    # ---------------------------------------------------------------- resample2d
    def rs(B, C, H, W, ks, dil=1, dtype=torch.float32, fwd=True, g1=True, g2=True, strided=False, overwrite=False, smooth=False):
        def make():
            a = rnd(B, C, H, W, dtype=dtype)
            fl = rnd(B, 2, H, W, dtype=dtype, lo=-3, hi=3)
            if smooth:
                fl = fl * 0 + 0.75
            b = torch.cat((fl, torch.full((B, 1, H, W), 2.0, dtype=dtype, device=dev)), 1)
            go = rnd(B, C, H, W, dtype=dtype)
            if strided:
                go = rnd(B, C, W, H, dtype=dtype).transpose(2, 3)
            ga = (torch.empty_like(a) if overwrite else torch.zeros_like(a)) if g1 else None
            gb = torch.empty_like(b) if g2 else None

            def run():
                if fwd:
                    ops.resample2d_forward(a, b, ks, dil)
                if g1 or g2:
                    ops.resample2d_backward(a, b, go, ks, dil, ga, gb, overwrite_input1=overwrite)
            return run
        return make

    for ks in (2, 4, 6, 8):
        add("rs ks%d 32x32" % ks, {}, rs(2, 8, 32, 32, ks))
        add("rs ks%d 128x128" % ks, {}, rs(1, 8, 128, 128, ks))
        add("rs ks%d 512x512" % ks, {}, rs(1, 8, 512, 512, ks))
        add("rs ks%d 32x32 f64" % ks, {}, rs(2, 8, 32, 32, ks, dtype=torch.float64))
        add("rs ks%d 32x32 dil2" % ks, {}, rs(2, 8, 32, 32, ks, dil=2))
    add("rs ks4 16x16", {}, rs(2, 8, 16, 16, 4))
    add("rs ks4 160x160 f64", {}, rs(1, 4, 160, 160, 4, dtype=torch.float64))
    add("rs ks4 160x160 dil2", {}, rs(1, 4, 160, 160, 4, dil=2))
    add("rs ks4 1024x1024 fwd", {}, rs(1, 4, 1024, 1024, 4, g1=False, g2=False))
    for v in range(1, 8):
        add("rs ks4 64x64 fwd", {"rs_fwd_variant": v}, rs(2, 8, 64, 64, 4, g1=False, g2=False))
    add("rs ks2 64x64 fwd", {"rs_fwd_variant": 5}, rs(2, 8, 64, 64, 2, g1=False, g2=False))
    add("rs ks6 64x64 fwd", {"rs_fwd_variant": 2}, rs(2, 8, 64, 64, 6, g1=False, g2=False))
    for name, shape in (("32x32", (2, 8, 32, 32)), ("512x512", (1, 8, 512, 512)), ("256x256", (2, 8, 256, 256))):
        for ks in (2, 4):
            add("rs ks%d %s g1 only" % (ks, name), {}, rs(*shape, ks, fwd=False, g2=False))
            add("rs ks%d %s g2 only" % (ks, name), {}, rs(*shape, ks, fwd=False, g1=False))
            add("rs ks%d %s overwrite" % (ks, name), {}, rs(*shape, ks, fwd=False, overwrite=True))
            for opts in ({"rs_bwd1_owned": 2}, {"rs_bwd1_owned": 2, "rs_bwd1_fixed": 2}, {"rs_bwd1_fixed": 2},
                         {"rs_bwd1_owned": 2, "rs_bwd1_rpt": 2}, {"rs_bwd1_owned_min_pixels": 1 << 16},
                         {"rs_bwd1_owned_min_pixels": 1 << 20}, {"rs_bwd1_owned_blocks": 256}, {"rs_bwd1_owned_blocks": 4096},
                         {"scatter_variant": 1}, {"scatter_variant": 2}, {"xcd_remap": 0}):
                add("rs ks%d %s bwd" % (ks, name), opts, rs(*shape, ks, fwd=False))
            for v in (1, 2, 5, 6):
                add("rs ks%d %s bwd" % (ks, name), {"rs_bwd1_variant": v}, rs(*shape, ks, fwd=False))
                add("rs ks%d %s bwd" % (ks, name), {"rs_bwd1_variant": v, "rs_bwd1_fixed": 2}, rs(*shape, ks, fwd=False))
    add("rs ks4 512x512 bwd smooth", {"rs_bwd1_owned": 2, "rs_bwd1_fixed": 2}, rs(1, 8, 512, 512, 4, fwd=False, smooth=True))
    add("rs ks6 512x512 bwd", {"rs_bwd1_fixed": 2, "rs_bwd1_rpt": 2}, rs(1, 8, 512, 512, 6, fwd=False))
    add("rs ks4 64x64 fwd past the list", {"rs_fwd_variant": 8}, rs(2, 8, 64, 64, 4, g1=False, g2=False))
    add("rs ks6 32x32 many channels (plane kernel, several channels per block)", {}, rs(8, 512, 32, 32, 6, fwd=False, g2=False))
    add("rs ks4 32x32 strided", {}, rs(2, 8, 32, 32, 4, fwd=False, strided=True))
    add("rs ks4 32x32 strided f64 overwrite", {}, rs(2, 8, 32, 32, 4, dtype=torch.float64, fwd=False, strided=True, overwrite=True))

    # ---------------------------------------------------------------- warp
    def wp(B, C, Hi, Wi, H, W, flip, dtype=torch.float32, fwd=True, gfeat=True, gflow=True, overwrite=False):
        def make():
            a = rnd(B, C, Hi, Wi, dtype=dtype)
            fl = rnd(B, 2, H, W, dtype=dtype, lo=-1.1, hi=1.1)
            go = rnd(B, (2 if flip else 1) * C, H, W, dtype=dtype)
            ga = (torch.empty_like(a) if overwrite else torch.zeros_like(a)) if gfeat else None
            gf = torch.zeros_like(fl) if gflow else None

            def run():
                if fwd:
                    ops.warp_forward(a, fl, flip)
                if gfeat or gflow:
                    ops.warp_backward(a, fl, go, flip, ga, gf, overwrite_feat=overwrite)
            return run
        return make

    for flip in (False, True):
        tag = " flip" if flip else ""
        add("warp 32x32" + tag, {}, wp(2, 8, 32, 32, 32, 32, flip))
        add("warp 32x32 f64" + tag, {}, wp(2, 8, 32, 32, 32, 32, flip, torch.float64))
        add("warp 3ch 128x128" + tag, {}, wp(2, 3, 128, 128, 128, 128, flip))
        add("warp 256x256" + tag, {}, wp(2, 8, 256, 256, 256, 256, flip))
        add("warp 256x256 f64" + tag, {}, wp(1, 4, 256, 256, 256, 256, flip, torch.float64))
        add("warp 200x200 -> 256x256" + tag, {}, wp(2, 8, 200, 200, 256, 256, flip))
        add("warp 4x16x512x512" + tag, {}, wp(4, 16, 512, 512, 512, 512, flip))
        add("warp 4x16x512x512 flow only" + tag, {}, wp(4, 16, 512, 512, 512, 512, flip, fwd=False, gfeat=False))
        add("warp 4x16x512x512 flow only" + tag, {"warp_multi_lds": 1}, wp(4, 16, 512, 512, 512, 512, flip, fwd=False, gfeat=False))
        add("warp 256x256 feat only" + tag, {}, wp(2, 8, 256, 256, 256, 256, flip, fwd=False, gflow=False))
        add("warp 256x256 overwrite" + tag, {}, wp(2, 8, 256, 256, 256, 256, flip, fwd=False, overwrite=True))
        add("warp 32x32 overwrite" + tag, {}, wp(2, 8, 32, 32, 32, 32, flip, fwd=False, overwrite=True))
        add("warp 32x32 flow only" + tag, {}, wp(2, 8, 32, 32, 32, 32, flip, fwd=False, gfeat=False))
        for v in (1, 2):
            add("warp 256x256" + tag, {"warp_fwd_variant": v}, wp(2, 8, 256, 256, 256, 256, flip, gfeat=False))
            add("warp 4x16x512x512" + tag, {"warp_fwd_variant": v}, wp(4, 16, 512, 512, 512, 512, flip, gfeat=False))
        for v in (1, 3, 4):
            add("warp 256x256 bwd" + tag, {"warp_feat_fixed": v}, wp(2, 8, 256, 256, 256, 256, flip, fwd=False))
            add("warp 256x256 bwd overwrite" + tag, {"warp_feat_fixed": v}, wp(2, 8, 256, 256, 256, 256, flip, fwd=False, overwrite=True))
        for opts in ({"warp_feat_gps": 1}, {"warp_feat_gps": 3}, {"scatter_variant": 1}, {"channel_slab": 8}, {"xcd_remap": 0}):
            add("warp 256x256" + tag, opts, wp(2, 8, 256, 256, 256, 256, flip))
        add("warp 2x64x256x256 bwd" + tag, {}, wp(2, 64, 256, 256, 256, 256, flip, fwd=False))
        add("warp 32x32" + tag, {"scatter_variant": 1}, wp(2, 8, 32, 32, 32, 32, flip))
        add("warp 256x256 bwd past the list" + tag, {"warp_feat_fixed": 2}, wp(2, 8, 256, 256, 256, 256, flip, fwd=False))
        # plane kernels with 2 / 4 / 8 channels per block (>= 512 blocks of them)
        add("warp 16x16 512x2ch" + tag, {}, wp(512, 2, 16, 16, 16, 16, flip, fwd=False))
        add("warp 16x16 512x4ch" + tag, {}, wp(512, 4, 16, 16, 16, 16, flip, fwd=False))
        add("warp 16x16 8x512ch" + tag, {}, wp(8, 512, 16, 16, 16, 16, flip, fwd=False))
        add("warp 16x16 8x512ch f64" + tag, {}, wp(8, 512, 16, 16, 16, 16, flip, torch.float64, fwd=False))

    def wm(levels, flip, dtype=torch.float32, gfeat=True, gflow=True):
        def make():
            feats = [rnd(B, C, S, S, dtype=dtype) for B, C, S in levels]
            flows = [rnd(B, 2, S, S, dtype=dtype, lo=-1.1, hi=1.1) for B, C, S in levels]
            gos = [rnd(B, (2 if flip else 1) * C, S, S, dtype=dtype) for B, C, S in levels]
            gfe = [torch.zeros_like(t) if gfeat else None for t in feats]
            gfl = [torch.zeros_like(t) if gflow else None for t in flows]

            def run():
                ops.warp_multi_forward(feats, flows, flip)
                ops.warp_multi_backward(feats, flows, gos, flip, gfe, gfl)
            return run
        return make

    net = [(2, 3, 32), (2, 3, 64), (2, 3, 128), (2, 128, 32), (2, 64, 64), (2, 64, 128), (2, 3, 128), (2, 16, 16)]
    for flip in (False, True):
        tag = " flip" if flip else ""
        add("warp multi" + tag, {}, wm(net, flip))
        add("warp multi f64" + tag, {}, wm(net[:5], flip, torch.float64))
        add("warp multi feat only" + tag, {}, wm(net, flip, gflow=False))
        add("warp multi flow only" + tag, {}, wm(net, flip, gfeat=False))
        add("warp multi 20 problems" + tag, {}, wm([(1, 3, 32)] * 20, flip))
        add("warp multi 2 / 4 / 8 channels per block" + tag, {}, wm([(512, 2, 16)] * 2 + [(512, 4, 16)] * 2 + [(128, 8, 16)] * 2, flip))
        add("warp multi with a large level" + tag, {}, wm([(2, 3, 64), (4, 16, 512)], flip))
        for opts in ({"warp_multi_lds": 1}, {"warp_multi_lds": 2}, {"warp_multi_planes": 1}, {"warp_multi_order": 1}, {"warp_nt": 1},
                     {"warp_nt": 2}, {"warp_pair_loads": 0}, {"scatter_variant": 1}, {"channel_slab": 8}):
            add("warp multi" + tag, opts, wm(net, flip))
    return out


def scope_names():
    """Every literal LaunchScope name of the three sampling files (scope_at names without their @size)."""
    names = set()
    for f in ("block_extractor.hip", "resample2d.hip", "warp.hip"):
        text = open(os.path.join(CSRC, f)).read()
        for m in re.finditer(r"LaunchScope\b[^;]*?;", text, re.S):
            names.update(n for n in re.findall(r'"([a-z0-9_]+)"', m.group(0)) if "_" in n)
    return names


def drive(labels_path, scopes):
    import torch
    from ffwm_amd import _lib
    torch.manual_seed(1234)
    mark = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    one = torch.ones(64, dtype=torch.int32, device="cuda:0")
    if scopes:
        _lib.prof_enable(True)
    labels = []
    for label, opts, make in calls():
        name = label + "".join(" %s=%d" % kv for kv in sorted(opts.items()))
        run = make()
        torch.cuda.synchronize()
        prev = {k: _lib.set_option(k, v) for k, v in opts.items()}
        try:
            torch.bitwise_xor(mark, one, out=mark)          # the marker the fold looks for
            run()
            torch.cuda.synchronize()
        finally:
            for k, v in prev.items():
                _lib.set_option(k, v)
        labels.append(name)
        print("CALL %d %s" % (len(labels), name), flush=True)
    if labels_path:
        with open(labels_path, "w") as f:
            f.write("\n".join(labels) + "\n")
    if scopes:
        seen = set(k.split("@")[0] for k in _lib.prof_collect())
        missing = sorted(scope_names() - seen)
        print("SCOPES %d named in the three files, %d of them produced, missing: %s" % (len(scope_names()), len(scope_names() & seen), missing))
        return 1 if missing else 0
    return 0


def fold(trace_dir, labels_path):
    labels = open(labels_path).read().splitlines()
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))

    def col(r, *names):
        for n in names:
            if n in r:
                return r[n]
        raise KeyError(names)

    rows.sort(key=lambda r: int(col(r, "Dispatch_Id")))
    call = 0
    for r in rows:
        name = col(r, "Kernel_Name")
        if "bitwise_xor" in name.lower() or "bitwisexor" in name.lower():
            call += 1
            continue
        if "ffwm" not in name or call == 0:
            continue
        name = re.sub(r"\(anonymous namespace\)::|^void |ffwm::", "", name)
        name = re.sub(r"\(.*$", "", name)
        grid = "x".join(col(r, "Grid_Size_" + a, "Grid_Size") for a in "XYZ")
        wg = "x".join(col(r, "Workgroup_Size_" + a, "Workgroup_Size") for a in "XYZ")
        print("%s | %s | grid %s | wg %s | lds %s" % (labels[call - 1], name, grid, wg, col(r, "LDS_Block_Size")))
    print("# %d calls, %d markers in the trace" % (len(labels), call))
    return 0 if call == len(labels) else 1


if __name__ == "__main__":
    a = sys.argv[1:]
    if a[:1] == ["--fold"]:
        sys.exit(fold(a[1], a[2]))
    sys.exit(drive(a[a.index("--labels") + 1] if "--labels" in a else None, "--scopes" in a))
