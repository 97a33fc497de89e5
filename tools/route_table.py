#!/usr/bin/env python3
"""Which kernels, with which launch geometry, does a fixed list of ffwm_amd.ops calls get?

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/route_table.py --labels DIR/labels.txt
    python tools/route_table.py --fold DIR DIR/labels.txt > routes.txt        (no GPU: folds the trace into one line per dispatch)
    python tools/route_table.py --scopes                                      (second pass, profiler on: LaunchScope coverage)
    ... --match REGEX                                                         (only the calls whose label matches, e.g. '^(wino|conv|wgrad|bn_|flow head|bias_act|local_attn|affine)')

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
    add("be k3 1024x1024 fwd (nt stores)", {}, be(1, 8, 1024, 1024, 3, src=False, flow=False))
    for v in (1, 2, 3, 9):
        add("be k3 160x160 bwd", {"be_bwd_variant": v}, be(1, 8, 160, 160, 3, fwd=False))
        add("be k3 32x48 bwd", {"be_bwd_variant": v}, be(2, 8, 32, 48, 3, fwd=False))
    for opts in ({"be_bwd_halo": 8}, {"be_bwd_halo": 8, "be_bwd_variant": 2}, {"be_bwd_rows": 64, "be_bwd_variant": 2},
                 {"be_bwd_rows": 64, "be_bwd_variant": 2, "be_bwd_halo": 8}, {"be_bwd_rows": 64}, {"be_bwd_fixed": 2},
                 {"be_bwd_fixed": 2, "be_bwd_halo": 8}, {"xcd_remap": 0}, {"scatter_variant": 1}):
        add("be k3 160x160 bwd", opts, be(1, 8, 160, 160, 3, fwd=False))
    add("be k2 160x160 bwd", {"be_bwd_rows": 64, "be_bwd_variant": 2}, be(1, 8, 160, 160, 2, fwd=False))
    add("be k3 32x48", {"scatter_variant": 1}, be(2, 8, 32, 48, 3))
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
    for name, shape in (("32x32", (2, 8, 32, 32)), ("512x512", (1, 8, 512, 512)), ("256x256", (2, 8, 256, 256))):
        for ks in (2, 4):
            add("rs ks%d %s g1 only" % (ks, name), {}, rs(*shape, ks, fwd=False, g2=False))
            add("rs ks%d %s g2 only" % (ks, name), {}, rs(*shape, ks, fwd=False, g1=False))
            add("rs ks%d %s overwrite" % (ks, name), {}, rs(*shape, ks, fwd=False, overwrite=True))
            for opts in ({"rs_bwd1_owned": 2}, {"rs_bwd1_owned": 2, "rs_bwd1_fixed": 2}, {"rs_bwd1_fixed": 2},
                         {"scatter_variant": 1}, {"scatter_variant": 2}, {"xcd_remap": 0}):
                add("rs ks%d %s bwd" % (ks, name), opts, rs(*shape, ks, fwd=False))
            for v in (1, 2, 5, 6):
                add("rs ks%d %s bwd" % (ks, name), {"rs_bwd1_variant": v}, rs(*shape, ks, fwd=False))
                add("rs ks%d %s bwd" % (ks, name), {"rs_bwd1_variant": v, "rs_bwd1_fixed": 2}, rs(*shape, ks, fwd=False))
    add("rs ks4 512x512 bwd smooth", {"rs_bwd1_owned": 2, "rs_bwd1_fixed": 2}, rs(1, 8, 512, 512, 4, fwd=False, smooth=True))
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
        for opts in ({"scatter_variant": 1}, {"xcd_remap": 0}):
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
        for opts in ({"warp_multi_planes": 1}, {"scatter_variant": 1}):
            add("warp multi" + tag, opts, wm(net, flip))
    # ---------------------------------------------------------------- conv_winograd.hip
    def wino(B, C, H, W, K, dgrad=False, act=0, bias=False, reuse=False):
        def make():
            x = rnd(B, C, H, W, lo=-1, hi=1)          # (the data gradient: grad_output with C = the layer's output channels, K = its inputs)
            w = rnd(*((C, K) if dgrad else (K, C)), 3, 3, lo=-0.1, hi=0.1)
            b = rnd(K) if bias else None
            frozen = {} if reuse else None

            def run():
                for _ in range(2 if reuse else 1):          # (the second call of a frozen layer finds its transformed weights)
                    ops.conv3x3_winograd(x, w, b, data_gradient=dgrad, act=act, slope=0.2, frozen=frozen)
            return run
        return make

    add("wino 1x8x10x12 -> 64 (generic)", {}, wino(1, 8, 10, 12, 64))
    add("wino 8x64x16x16 -> 64 (raw)", {}, wino(8, 64, 16, 16, 64))
    add("wino 1x256x16x16 -> 64 (split 2)", {}, wino(1, 256, 16, 16, 64))
    add("wino 1x512x16x16 -> 64 (split 4)", {}, wino(1, 512, 16, 16, 64))
    add("wino 1x512x16x16 -> 64", {"conv_wino_split": 2}, wino(1, 512, 16, 16, 64))
    add("wino 1x512x16x16 -> 64", {"conv_wino_split": 0}, wino(1, 512, 16, 16, 64))
    add("wino 8x64x16x16 -> 64", {"conv_wino_ws": 1}, wino(8, 64, 16, 16, 64))
    add("wino 1x512x16x16 -> 64 (split keeps the plain raw kernel)", {"conv_wino_ws": 1}, wino(1, 512, 16, 16, 64))
    add("wino 8x64x16x16 -> 64", {"conv_wino_raw": 0}, wino(8, 64, 16, 16, 64))
    for W in (32, 64, 128):
        add("wino 1x64x%dx%d -> 64 (raw)" % (2 * 64 // (W // 2), W), {}, wino(1, 64, 2 * 64 // (W // 2), W, 64))
    add("wino 8x64x16x16 -> 67 (thin tail)", {}, wino(8, 64, 16, 16, 67, bias=True, act=1))
    add("wino 8x64x16x16 -> 67", {"conv_thin_tail": 0}, wino(8, 64, 16, 16, 67))
    add("wino 8x64x16x16 -> 3 (thin alone)", {}, wino(8, 64, 16, 16, 3, bias=True))
    for K in (65, 66, 68):
        add("wino 1x8x8x12 -> %d (generic + thin)" % K, {}, wino(1, 8, 8, 12, K))
    add("wino 1x8x10x10 -> 67 (width not a multiple of 4: no thin tail)", {}, wino(1, 8, 10, 10, 67))
    add("wino 8x64x16x16 dgrad -> 64", {}, wino(8, 64, 16, 16, 64, dgrad=True))
    add("wino 1x512x16x16 dgrad -> 64 (split 4)", {}, wino(1, 512, 16, 16, 64, dgrad=True))
    add("wino 8x64x16x16 -> 64 act", {}, wino(8, 64, 16, 16, 64, act=1, bias=True))
    add("wino 1x512x16x16 -> 64 act (no split)", {}, wino(1, 512, 16, 16, 64, act=1, bias=True))
    add("wino 8x64x16x16 -> 67 reused workspace", {}, wino(8, 64, 16, 16, 67, reuse=True))

    def wino_multi(n):
        def make():
            items = [(rnd(67, 70, 3, 3), False, True), (rnd(67, 70, 3, 3), False, False), (rnd(64, 8, 3, 3), True, True),
                     (rnd(3, 16, 3, 3), False, True)]
            items = (items * ((n + 3) // 4))[:n]
            return lambda: ops.conv3x3_winograd_weights_multi(items)
        return make

    add("wino weights_multi 4 items (thin and not)", {}, wino_multi(4))
    add("wino weights_multi 4 items", {"conv_thin_tail": 0}, wino_multi(4))
    add("wino weights_multi 26 items (two launches)", {}, wino_multi(26))

    # ---------------------------------------------------------------- conv_fwd.hip
    def cf(B, C, H, W, K, k, stride, pad, mode, split=True, act=1, odd_dst=False):
        def make():
            from ffwm_amd.flownet_eval import conv_mfma
            x = rnd(B, C, H, W, lo=-1, hi=1)
            w = rnd(*((K, C) if mode == 0 else (C, K)), k, k, lo=-0.1, hi=0.1)
            b = rnd(K)
            dst = None
            if odd_dst:          # a destination that is not 16-byte aligned: the scalar reduce kernel
                Ho, Wo = ((2 * H, 2 * W) if mode in (1, 2) else (H, W) if mode == 3 else
                          ((H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1))
                dst = torch.empty(B * K * Ho * Wo + 1, device=dev)[1:].view(B, K, Ho, Wo)
            return lambda: conv_mfma(x, w, b, stride, pad, mode, act, dst=dst, split=split)
        return make

    for v in (0, 1, 2, 3, 4):
        opts = {"conv_tile_variant": v} if v else {}
        add("conv_fwd 3x3 s1 2x32x8x8 -> 64", opts, cf(2, 32, 8, 8, 64, 3, 1, 1, 0))
        add("conv_fwd 4x4 s2 2x32x8x8 -> 64", opts, cf(2, 32, 8, 8, 64, 4, 2, 1, 0))
        add("conv_fwd transposed 2x64x8x8 -> 32", opts, cf(2, 64, 8, 8, 32, 4, 2, 1, 1))
        add("conv_fwd dgrad 3x3 s2 2x64x8x8 -> 32", opts, cf(2, 64, 8, 8, 32, 3, 2, 1, 2, act=0))
        add("conv_fwd dgrad 3x3 s1 2x64x8x8 -> 32", opts, cf(2, 64, 8, 8, 32, 3, 1, 1, 3, act=0))
    add("conv_fwd 3x3 s1 2x32x8x8 -> 64 no workspace", {}, cf(2, 32, 8, 8, 64, 3, 1, 1, 0, split=False))
    add("conv_fwd 3x3 s1 8x32x64x64 -> 128 (fills the chip: 64 x 128 tiles, no split)", {}, cf(8, 32, 64, 64, 128, 3, 1, 1, 0))
    add("conv_fwd 3x3 s1 6x256x7x7 -> 512 (split, 49-pixel planes: scalar reduce)", {}, cf(6, 256, 7, 7, 512, 3, 1, 1, 0))
    add("conv_fwd 3x3 s1 2x32x8x8 -> 64 unaligned destination", {}, cf(2, 32, 8, 8, 64, 3, 1, 1, 0, odd_dst=True))
    add("conv_fwd 3x3 s1 2x32x8x8 -> 64", {"conv_fwd_split_target": 128}, cf(2, 32, 8, 8, 64, 3, 1, 1, 0))

    # ---------------------------------------------------------------- conv_bwd.hip, conv_wgrad.hip, conv_wgrad_wino.hip
    def wg(B, C, H, W, K, k, stride, pad, tiled=True, bias=False, prezeroed=False):
        def make():
            Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
            rows, x = rnd(B, K, Ho, Wo, lo=-1, hi=1), rnd(B, C, H, W, lo=-1, hi=1)
            zeroed = torch.zeros(K * C * k * k + (K if bias else 0), device=dev) if prezeroed else None
            if tiled:
                return lambda: ops.conv2d_wgrad_tiled(rows, x, k, stride, pad, want_bias=bias, zeroed=zeroed)
            return lambda: ops.conv2d_wgrad(rows, x, k, stride, pad)
        return make

    for k, stride, pad in ((1, 1, 0), (3, 1, 1), (3, 2, 1), (4, 2, 1)):
        name = "%dx%d s%d" % (k, k, stride)
        # K and C k^2 <= 64 / > 64: the four tile shapes (wmt, wnt) are open to the cost estimate
        for C, K in ((4, 32), (4, 128), (96, 32), (96, 128)):
            add("wgrad tiled %s 2x%dx16x16 -> %d" % (name, C, K), {}, wg(2, C, 16, 16, K, k, stride, pad, bias=True))
        add("wgrad tiled %s 8x96x32x32 -> 128 (sliced)" % name, {}, wg(8, 96, 32, 32, 128, k, stride, pad))
        add("wgrad tiled %s 8x96x32x32 -> 128" % name, {"conv_wgrad_unsliced": 1}, wg(8, 96, 32, 32, 128, k, stride, pad))
        add("wgrad tiled %s 8x96x32x32 -> 128 prezeroed" % name, {}, wg(8, 96, 32, 32, 128, k, stride, pad, bias=True, prezeroed=True))
        add("wgrad generic %s 2x24x9x9 -> 40" % name, {}, wg(2, 24, 9, 9, 40, k, stride, pad, tiled=False))
    add("wgrad tiled 3x3 s1 6x512x8x8 -> 512 (FlowNet's 8 x 8 layers)", {}, wg(6, 512, 8, 8, 512, 3, 1, 1))

    def wg3(B, C, H, W, K, bias=True):
        def make():
            x, go = rnd(B, C, H, W, lo=-1, hi=1), rnd(B, K, H, W, lo=-1, hi=1)
            gb = torch.zeros(K, device=dev) if bias else None
            return lambda: ops.conv3x3_wgrad(x, go, grad_bias=gb)
        return make

    for v in (0, 1, 2):
        opts = {"conv_wgrad_wino": v} if v else {}
        add("conv3x3_wgrad 2x64x64x64 -> 64", opts, wg3(2, 64, 64, 64, 64))
        add("conv3x3_wgrad 8x64x128x128 -> 64", opts, wg3(8, 64, 128, 128, 64))
        add("conv3x3_wgrad 2x67x8x64 -> 70 (full tiles + both remainders)", opts, wg3(2, 67, 8, 64, 70))
        add("conv3x3_wgrad 2x3x64x64 -> 64 (remainder columns only)", opts, wg3(2, 3, 64, 64, 64))
    add("conv3x3_wgrad 1x64x2x64 -> 64 (fewer than 16 chunks: direct kernel)", {"conv_wgrad_wino": 1}, wg3(1, 64, 2, 64, 64, bias=False))

    # ---------------------------------------------------------------- bn_lrelu.hip
    def bn(B, C, H, W, res=False, scratch=False, act=0):
        def make():
            from ffwm_amd import _lib
            lib = _lib.load()
            x, go, r = rnd(B, C, H, W, lo=-1, hi=1), rnd(B, C, H, W, lo=-1, hi=1), rnd(B, C, H, W, lo=-1, hi=1)
            y, dx, dr = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
            g, b, rb = rnd(C), rnd(C), rnd(C)
            rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
            sm, si, dg, db = (torch.empty(C, device=dev) for _ in range(4))
            sc = torch.zeros(2 * C + (C + 1) // 2, device=dev, dtype=torch.float64) if scratch else None
            P = lambda t: None if t is None else t.data_ptr()

            def run():
                st = torch.cuda.current_stream().cuda_stream
                if res:
                    _lib.check(lib.ffwm_bn_res_act_forward(P(x), P(g), P(b), P(rm), P(rv), P(r), P(rb), P(y), P(sm), P(si), P(sc), B, C, H * W,
                                                           1e-5, 0.1, 0.2, act, _lib.F32, st), "ffwm_bn_res_act_forward")
                    _lib.check(lib.ffwm_bn_res_act_backward(P(x), P(y), P(go), P(g), P(sm), P(si), P(dx), P(dr), P(dg), P(db), P(sc), B, C,
                                                            H * W, 0.2, act, _lib.F32, st), "ffwm_bn_res_act_backward")
                else:
                    _lib.check(lib.ffwm_bn_lrelu_forward(P(x), P(g), P(b), P(rm), P(rv), P(y), P(sm), P(si), P(sc), B, C, H * W, 1e-5, 0.1,
                                                         0.2, _lib.F32, st), "ffwm_bn_lrelu_forward")
                    _lib.check(lib.ffwm_bn_lrelu_backward(P(x), P(go), P(g), P(b), P(sm), P(si), P(dx), P(dg), P(db), P(sc), B, C, H * W, 0.2,
                                                          _lib.F32, st), "ffwm_bn_lrelu_backward")
            return run
        return make

    for res in (False, True):
        tag = "bn_res_act" if res else "bn_lrelu"
        add(tag + " 6x40x8x8 (wave per channel)", {}, bn(6, 40, 8, 8, res))
        add(tag + " 6x40x8x8 with scratch (still the wave kernel)", {}, bn(6, 40, 8, 8, res, scratch=True))
        add(tag + " 2x40x32x32 (block per channel)", {}, bn(2, 40, 32, 32, res))
        add(tag + " 2x40x32x32 with scratch (too small to slice)", {}, bn(2, 40, 32, 32, res, scratch=True))
        add(tag + " 2x8x128x128 with scratch (2 slices, two phases)", {}, bn(2, 8, 128, 128, res, scratch=True))
        add(tag + " 8x8x256x256 with scratch (32 slices)", {}, bn(8, 8, 256, 256, res, scratch=True))
        add(tag + " 2x8x127x129 with scratch (H W % 4 != 0: unsliced)", {}, bn(2, 8, 127, 129, res, scratch=True))
    add("bn_res_act 2x8x128x128 sigmoid", {}, bn(2, 8, 128, 128, True, scratch=True, act=1))

    # ---------------------------------------------------------------- flownet_ops.hip
    def fh(B, C, H, W):
        def make():
            from ffwm_amd import _lib
            from ffwm_amd.flownet_eval import flow_head
            x, w, b = rnd(B, C, H, W, lo=-1, hi=1), rnd(2, C, 3, 3, lo=-0.1, hi=0.1), rnd(2)
            gy, gz, gx = rnd(B, 2, H, W), torch.empty(B, 2, H, W, device=dev), torch.empty(B, C, H, W, device=dev)

            def run():
                y = flow_head(x, w, b)
                _lib.check(_lib.load().ffwm_flow_head_backward(y.data_ptr(), gy.data_ptr(), w.data_ptr(), gz.data_ptr(), gx.data_ptr(), B, C, H, W,
                                                               _lib.F32, torch.cuda.current_stream().cuda_stream), "ffwm_flow_head_backward")
            return run
        return make

    add("flow head 6x32x32x32 (tile 64)", {}, fh(6, 32, 32, 32))
    add("flow head 6x32x16x16 (tile 16)", {}, fh(6, 32, 16, 16))
    add("flow head 6x32x8x8 (tile 4)", {}, fh(6, 32, 8, 8))
    add("flow head 96x32x4x4 (tile 16: plane below 64 pixels)", {}, fh(96, 32, 4, 4))
    add("flow head 1x32x3x3 (tile 4: plane below 16 pixels)", {}, fh(1, 32, 3, 3))

    def ba_(B, C, H, W, act, two=False):
        def make():
            from ffwm_amd.flownet_eval import bias_act
            h, b = rnd(B, C, H, W, lo=-1, hi=1), rnd(C)
            y, y2 = torch.empty_like(h), (torch.empty_like(h) if two else None)
            return lambda: bias_act(h, b, act, y=y, y2=y2)
        return make

    for act in (0, 1, 2):
        add("bias_act act %d 2x16x8x8 (float4)" % act, {}, ba_(2, 16, 8, 8, act, two=True))
        add("bias_act act %d 2x16x7x9 (scalar)" % act, {}, ba_(2, 16, 7, 9, act))

    def ct(B, C, H, W, K):
        def make():
            from ffwm_amd.flownet_eval import conv_thin
            x, w, b = rnd(B, C, H, W, lo=-1, hi=1), rnd(C, 3, 3, K, lo=-0.1, hi=0.1), rnd(K)
            return lambda: conv_thin(x, w, b, 1)
        return make

    for v in (0, 1, 2, 5, 6):
        for K in (8, 16):
            add("conv_thin 2x6x20x70 -> %d" % K, {"conv_thin_variant": v} if v else {}, ct(2, 6, 20, 70, K))

    # ---------------------------------------------------------------- local_attn_reshape.hip, affine_reg.hip
    def lar(k, dtype=torch.float32):
        def make():
            a = rnd(2, k * k, 12, 20, dtype=dtype)
            go = rnd(2, 1, 12 * k, 20 * k, dtype=dtype)
            gi = torch.zeros_like(a)

            def run():
                ops.local_attn_reshape_forward(a, k)
                ops.local_attn_reshape_backward(go, k)
                ops.local_attn_reshape_backward(go, k, gi, accumulate=True)
            return run
        return make

    for k in range(1, 10):
        add("local_attn_reshape k%d" % k, {}, lar(k))
    add("local_attn_reshape k3 f64", {}, lar(3, torch.float64))
    add("local_attn_reshape k8 f64", {}, lar(8, torch.float64))

    def ar(kz, dtype=torch.float32, grad=True):
        def make():
            fl = rnd(2, 2, 20, 70, dtype=dtype, lo=-1, hi=1)
            ktk = rnd(kz * kz, kz * kz, dtype=dtype)
            return lambda: ops.affine_regularization(fl, ktk, kz, want_grad=grad)
        return make

    for kz in (3, 5, 7):
        add("affine_regularization k%d" % kz, {}, ar(kz))
        add("affine_regularization k%d f64 loss only" % kz, {}, ar(kz, torch.float64, grad=False))
    return out


def scope_names():
    """Every literal LaunchScope name of the three sampling files (scope_at names without their @size)."""
    names = set()
    for f in ("block_extractor.hip", "resample2d.hip", "warp.hip"):
        text = open(os.path.join(CSRC, f)).read()
        for m in re.finditer(r"LaunchScope\b[^;]*?;", text, re.S):
            names.update(n for n in re.findall(r'"([a-z0-9_]+)"', m.group(0)) if "_" in n)
    return names


def drive(labels_path, scopes, match=None):
    import torch
    from ffwm_amd import _lib
    torch.manual_seed(1234)
    mark = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    one = torch.ones(64, dtype=torch.int32, device="cuda:0")
    if scopes:
        _lib.prof_enable(True)
    labels = []
    for label, opts, make in calls():
        if match and not re.search(match, label):
            continue
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
    sys.exit(drive(a[a.index("--labels") + 1] if "--labels" in a else None, "--scopes" in a,
                   a[a.index("--match") + 1] if "--match" in a else None))
