"""The identity evaluation of the reference's inference loop: LightCNN-29 as a launch-lean path, the centre-face crop and the rank-1
matcher, behind one class.

`test_ffwm.py` frontalises a profile face, takes the LightCNN-29 feature of the result (models/ffwm_model.py:191-202) and ranks it
against the gallery's features by cosine similarity, counting rank-1 hits by pose (util/util.py:141-181).  `ffwm_eval.Frontalizer`
is the first third; this module is the rest:

* `FoldedLightCNN`: lightcnn/light_cnn.py:82-129 in eval mode without its 79 077-way classifier.  Each of the 29 convolutions runs
  once without its bias -- on csrc/conv_winograd.hip where `conv.winograd_ok` says so, on csrc/conv_fwd.hip where
  `conv.fwd_route_ok` and the module route's own condition say so, `F.conv2d(..., bias=None)` for the rest (the 5 x 5 stem, the 1 x 1
  `conv_a` layers, what neither kernel serves) -- followed by ONE `mfm_tail` launch (csrc/lightcnn_eval.hip): bias, max-feature-map,
  the residual block's add and the MaxPool2d(2, 2, ceil_mode=True) behind the layer in a single pass.  `fc` is `F.linear` without
  bias and the bias + max-feature-map kernel of csrc/mfm.hip.
* `FaceIdentifier`: Frontalizer -> channel mean (or the centre-face crop of `--crop`: mean -> WarpNet(build_grid(b, 98)) -> bilinear
  resize, one kernel) -> FoldedLightCNN -> cosine top-k against a stored gallery, replayed from ONE captured hipGraph.
* `RankMeter`: the reference's `AverageMeter` over the matcher's indices.

Weights are snapshotted at construction: build from networks in `.eval()` and rebuild after the weights change.
"""
import collections
import os

import torch
import torch.nn.functional as F

from .ffwm_eval import Frontalizer, _Spec, check_precision, conv_route, planned_precision, split_conv, split_route_ok, torch_warp
from .graphs import GraphedForward

KINDS = ("winograd", "winograd_split", "conv_mfma", "vendor_conv", "mfm_tail", "linear", "mfm")

# Layers that stay on the vendor's convolution although a hand-written kernel would serve them: those where the vendor's kernel measured
# faster at BOTH batch 1 and batch 8 as device time inside a captured graph, which is where FaceIdentifier runs them
# (tools/identity_bench.py; the table is in profiles/identity_eval.txt): the 96-channel residual layers at 32 x 32 (19 against 15 us,
# 48 against 38-40) and the 128-channel layers at 16 x 16 (14.6 against 10.8 us, 30.4 against 27.5).
VENDOR_LAYERS = frozenset(["block2.%d.conv%d" % (j, c) for j in range(2) for c in (1, 2)]
                          + ["block4.%d.conv%d" % (j, c) for j in range(4) for c in (1, 2)] + ["group4.conv"])

# Layers that stay on their fp32 route under precision="bf16x3": those where the split route (csrc/conv_winograd_gemm_split.hip)
# measured slower than the layer's present route at BOTH batch 1 and batch 8 by more than the larger min-max spread
# (tools/split_conv_bench.py; the table is in profiles/wino_gemm_split.txt): the 48-channel layers at 64 x 64 -- 16.5 against 21.8 us
# and 24.2 against 46.2 us (48 -> 96), 16.1 against 27.6 and 42.1 against 69.4 (48 -> 192).  C = 48 is padded to two 32-channel
# stages, and at these planes the transforms around the GEMM move more bytes than the fused fp32 kernels.
SPLIT_EXCLUDED_LAYERS = frozenset(["block1.0.conv1", "block1.0.conv2", "group1.conv"])

_Layer = collections.namedtuple("_Layer", "w b k stride pad")
_BLOCKS = (1, 2, 3, 4)          # residual blocks in front of group1 .. group4
_POOL_BEHIND = {"conv1": True, "group1.conv": True, "group2.conv": True, "group3.conv": False, "group4.conv": True}


def crop_grid(b, d=98, dtype=torch.float32, device=None):
    """IdentityLoss.build_grid (models/losses.py:102-112) as [b, 2, d, d]: linspace(-d // 2, d // 2, d) around the centre (64, 77) of a
    128 x 128 image, over 64."""
    r = d // 2
    lin = torch.linspace(-r, r, d, dtype=dtype, device=device)
    gx = (lin.view(1, d).expand(d, d) + (64 - 64)) / 64
    gy = (lin.view(d, 1).expand(d, d) + (77 - 64)) / 64
    return torch.stack((gx, gy), 0).unsqueeze(0).repeat(b, 1, 1, 1)


def torch_identity_input(img, crop=False, grid=None):
    """ops.identity_input as the reference's PyTorch composition (any dtype and device): gray first, then the crop
    (models/ffwm_model.py:196-200).  grid: the sampling grid [B, 2, 98, 98] when it is not `crop_grid` in the image's own dtype."""
    gray = torch.mean(img, dim=(1,), keepdim=True)
    if not crop:
        return gray
    if tuple(img.shape[2:]) != (128, 128):
        raise ValueError("identity_input: the centre-face crop is defined for 128 x 128 images only")
    warped = torch_warp(gray, crop_grid(img.shape[0], 98, img.dtype, img.device) if grid is None else grid)
    return F.interpolate(warped, (128, 128), mode="bilinear")


# ------------------------------------------------------------------------------------------------ the three executors
def _pooled(n):
    return (n + 1) // 2


class _PlanExec(object):
    """Shapes only: records (layer name, kind) of every launch the HIP executor would issue."""

    def __init__(self, owner):
        self.o, self.launches = owner, []

    def layer(self, name, x, residual=None, pool=False):
        L = self.o.layers[name]
        self.launches.append((name, self.o._route(name, x)))
        self.launches.append((name, "mfm_tail"))
        B, _, H, W = x.shape
        Ho, Wo = (H + 2 * L.pad - L.k) // L.stride + 1, (W + 2 * L.pad - L.k) // L.stride + 1
        return _Spec(B, L.w.shape[0] // 2, _pooled(Ho) if pool else Ho, _pooled(Wo) if pool else Wo)

    def fc(self, p):
        if p.shape[1] * p.shape[2] * p.shape[3] != self.o.fc_w.shape[1]:
            raise ValueError("FoldedLightCNN: fc takes %d features, the last pool gives %s" % (self.o.fc_w.shape[1], tuple(p.shape[1:])))
        self.launches += [("fc", "linear"), ("fc", "mfm")]
        return _Spec(p.shape[0], self.o.fc_w.shape[0] // 2)


def run_conv(owner, name, x, route):
    """Convolution `name` of a FoldedLightCNN without its bias on the kernel `route` names (tools/identity_bench.py times the routes
    through this)."""
    from . import flownet_eval, ops
    L = owner.layers[name]
    if route == "winograd_split":
        return split_conv(owner, name, x, None, "none")
    if route == "winograd":
        return ops.conv3x3_winograd(x, L.w, None, act=0, frozen=owner._wino.setdefault(name, {}))
    if route == "conv_mfma":
        return flownet_eval.conv_mfma(x, L.w, None, L.stride, L.pad, False, 0, arena=owner.arena)
    return F.conv2d(x, L.w, None, L.stride, L.pad)


class _HipExec(_PlanExec):
    """The launches themselves; `launches` records them as plan() lists them."""

    def layer(self, name, x, residual=None, pool=False):
        from . import ops
        route = self.o._route(name, x)
        self.launches.append((name, route))
        h = run_conv(self.o, name, x, route)
        self.launches.append((name, "mfm_tail"))
        return ops.mfm_tail(h, self.o.layers[name].b, residual, pool)

    def fc(self, p):
        from . import ops
        _PlanExec.fc(self, p)
        return ops.mfm_forward(F.linear(p.flatten(1), self.o.fc_w, None), self.o.fc_b)


class _TorchExec(object):
    """The same arithmetic as a PyTorch composition (any dtype, any device); the bias rides in the convolution, as in the module."""

    def __init__(self, owner):
        self.o, self.launches = owner, []

    @staticmethod
    def _mfm(h):
        a, b = torch.split(h, h.shape[1] // 2, 1)
        return torch.max(a, b)

    def layer(self, name, x, residual=None, pool=False):
        L = self.o.layers[name]
        y = self._mfm(F.conv2d(x, L.w, L.b, L.stride, L.pad))
        if residual is not None:
            y = y + residual
        return F.max_pool2d(y, 2, 2, ceil_mode=True) if pool else y

    def fc(self, p):
        return self._mfm(F.linear(p.flatten(1), self.o.fc_w, self.o.fc_b))


# ------------------------------------------------------------------------------------------------ FoldedLightCNN
class FoldedLightCNN(object):
    """nets.LightCNN29's eval forward without the classifier (see the module docstring).

        net = FoldedLightCNN(lightcnn.eval(), graph=True)
        fc, pool = net(gray)            # [B, 256], [B, 128, 8, 8] for 128 x 128 inputs

    backend: "hip" (float32 GPU network; the default on a GPU) or "torch" (the same arithmetic as a PyTorch composition, any dtype
    and device).  precision: "fp32" (the default) or, hip only, "bf16x3": the 3 x 3 / stride 1 layers that ffwm_eval.split_route_ok
    names run on csrc/conv_winograd_gemm_split.hip (bf16 MFMA, hi / lo split operands; float32 tensors in and out).  graph=True (hip only) replays the forward from one captured hipGraph, re-captured when the input shape changes:
    THE OUTPUTS ARE STATIC BUFFERS THAT THE NEXT CALL OVERWRITES -- clone what must survive it.  `fc2` is neither kept nor run."""

    def __init__(self, net, graph=False, backend=None, precision="fp32"):
        from . import nets
        if not isinstance(net, nets.LightCNN29):
            raise TypeError("FoldedLightCNN: a nets.LightCNN29 is expected")
        if net.training:
            raise ValueError("FoldedLightCNN snapshots eval-mode weights (dropout off): call net.eval() first")
        p = net.conv1.filter.weight
        if backend is None:
            backend = "hip" if p.is_cuda else "torch"
        if backend not in ("hip", "torch"):
            raise ValueError("FoldedLightCNN: backend must be 'hip' or 'torch'")
        if backend == "hip" and not (p.is_cuda and p.dtype == torch.float32):
            raise NotImplementedError("FoldedLightCNN: the hip backend takes float32 GPU networks only (backend='torch' for the rest)")
        if graph and backend != "hip":
            raise ValueError("FoldedLightCNN: graph replay needs the hip backend")
        self.precision = check_precision("FoldedLightCNN", precision, backend)
        self._split_u = {}
        self.backend, self.use_graph = backend, bool(graph)
        self.device, self.dtype = p.device, p.dtype
        self.layers = collections.OrderedDict()
        self._wino = {}
        self._graph = None
        self.last_launches = []
        if backend == "hip":
            from .flownet_eval import Arena
            self.arena = Arena()
        for name in self.layer_names():
            f = net.get_submodule(name).filter
            self.layers[name] = _Layer(f.weight.detach().clone().contiguous(), f.bias.detach().clone().contiguous(), f.kernel_size[0],
                                       f.stride[0], f.padding[0])
        self.fc_w = net.fc.filter.weight.detach().clone().contiguous()
        self.fc_b = net.fc.filter.bias.detach().clone().contiguous()

    @staticmethod
    def layer_names():
        """The 29 convolution layers in forward order."""
        names = ["conv1"]
        for i, n in enumerate(_BLOCKS, start=1):
            for j in range(n):
                names += ["block%d.%d.conv1" % (i, j), "block%d.%d.conv2" % (i, j)]
            names += ["group%d.conv_a" % i, "group%d.conv" % i]
        return names

    def _route(self, name, x):
        """Which kernel serves convolution `name` on input x (a tensor or a _Spec): ffwm_eval.conv_route, FoldedFFWM's predicates,
        with no activation; a layer of VENDOR_LAYERS stays on the vendor's kernel.  precision="bf16x3": the split route wherever
        ffwm_eval.split_route_ok says so (VENDOR_LAYERS included), but for the layers of SPLIT_EXCLUDED_LAYERS."""
        if self.precision == "bf16x3" and name not in SPLIT_EXCLUDED_LAYERS and split_route_ok(self.layers[name], x):
            return "winograd_split"
        if name in VENDOR_LAYERS:
            return "vendor_conv"
        return conv_route(self.layers[name], x, 0)

    def _run(self, ex, x):
        x = ex.layer("conv1", x, pool=_POOL_BEHIND["conv1"])
        for i, n in enumerate(_BLOCKS, start=1):
            for j in range(n):
                h = ex.layer("block%d.%d.conv1" % (i, j), x)
                x = ex.layer("block%d.%d.conv2" % (i, j), h, residual=x)
            x = ex.layer("group%d.conv_a" % i, x)
            x = ex.layer("group%d.conv" % i, x, pool=_POOL_BEHIND["group%d.conv" % i])
        return ex.fc(x), x

    def plan(self, B, H, W, precision=None):
        """The ordered launches of one forward at batch B and H x W inputs as [(layer name, kind)], kind in KINDS; no device is touched.
        precision: the plan the hip backend would follow under that precision (default: this object's own)."""
        ex = _PlanExec(self)
        with planned_precision(self, precision):
            self._run(ex, _Spec(B, 1, H, W))
        return ex.launches

    def _forward(self, x):
        if self.backend == "torch":
            return self._run(_TorchExec(self), x)
        if not (x.is_cuda and x.dtype == torch.float32):
            raise NotImplementedError("FoldedLightCNN: the hip backend takes float32 GPU tensors")
        self.arena.begin(x.device)
        ex = _HipExec(self)
        out = self._run(ex, x.contiguous())
        self.last_launches = ex.launches
        return out

    @torch.no_grad()
    def __call__(self, gray):
        if gray.dim() != 4 or gray.shape[1] != 1:
            raise ValueError("FoldedLightCNN: gray [B, 1, H, W] expected, got %s" % (tuple(gray.shape),))
        if not self.use_graph:
            return self._forward(gray)
        if self._graph is None:
            # two warm-up passes outside the capture: a layer's first Winograd call synchronises to publish its kept transform
            self._graph = GraphedForward(self._forward)
        return self._graph(gray)


# ------------------------------------------------------------------------------------------------ FaceIdentifier
IdentityResult = collections.namedtuple("IdentityResult", "frontal feature top_sim top_idx")


def torch_cosine_topk(probe, gallery, k):
    """ops.cosine_topk in PyTorch: per probe row torch.cosine_similarity against the gallery and its k best, the lower index first
    among equal similarities (a stable descending sort; topk itself leaves the order of ties open)."""
    sims = torch.stack([torch.cosine_similarity(gallery, probe[b:b + 1], dim=1) for b in range(probe.shape[0])])
    order = torch.sort(sims, dim=1, descending=True, stable=True)[1][:, :k]
    return torch.gather(sims, 1, order), order.to(torch.int32)


class FaceIdentifier(object):
    """FFWMModel.test (models/ffwm_model.py:191-202) and the matching of test_ffwm.py without a trainer: frontalise, take the
    LightCNN-29 feature of the channel mean of fake_F128 (crop=True: of its centre-face crop, the reference's --crop), rank it against a
    gallery.

        ident = FaceIdentifier.from_checkpoints("checkpoints/ffwm", "latest", "checkpoints/LightCNN_29Layers.pth")
        ident.set_gallery(keys, gallery_images)          # images [G, 1 | 3, 128, 128]
        r = ident(img_S)                                 # r.frontal (a FrontalizerResult), r.feature [B, 256], r.top_sim / r.top_idx [B, k]
        meter.update(r.top_idx, names, ident.gallery_keys)

    k = min(max(10, topk), G), as AverageMeter.update takes it; before set_gallery the two top-k fields are None.  With graph=True (hip
    backend) the frontaliser, the input kernel, the LightCNN and the matcher replay from ONE captured hipGraph, re-captured when the
    input shape or the gallery size changes: THE RESULT'S TENSORS ARE STATIC BUFFERS THAT THE NEXT CALL OVERWRITES -- clone what must
    survive it."""

    def __init__(self, flowNetF, netG, lightcnn, crop=False, graph=True, topk=1, backend=None, precision="fp32"):
        self.front = Frontalizer(flowNetF, netG, graph=False, backend=backend, precision=precision)
        self.backend = self.front.backend
        if graph and self.backend != "hip":
            raise ValueError("FaceIdentifier: graph replay needs the hip backend")
        self.net = FoldedLightCNN(lightcnn, graph=False, backend=self.backend, precision=precision)
        self.precision = self.net.precision
        self.crop, self.use_graph, self.topk = bool(crop), bool(graph), int(topk)
        self.gallery_keys, self.gallery_features = None, None
        self._graph = None
        if self.backend == "hip":
            from .flownet_eval import Arena
            self._eager_arena = Arena()          # feature()'s: see there

    @classmethod
    def from_checkpoints(cls, load_dir, epoch, lightcnn_path, ngf=64, crop=False, device=None, graph=True, backend=None, topk=1,
                         precision="fp32"):
        """Frontalizer.from_checkpoints' two files, and `lightcnn_path`: a plain LightCNN-29 state dict as FFWMModel.load_network reads
        it (models/ffwm_model.py:212-215)."""
        from . import nets
        device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        mods = {"flowNetF": nets.FlowNet(ngf), "netG": nets.FFWM(sn=True)}
        for name, mod in mods.items():
            sd = torch.load(os.path.join(load_dir, "%s_net_%s.pth" % (epoch, name)), map_location="cpu")
            if hasattr(sd, "_metadata"):
                del sd._metadata
            mod.load_state_dict(sd)
            mod.to(device).eval()
        light = nets.LightCNN29()
        light.load_state_dict(torch.load(lightcnn_path, map_location="cpu"))
        light.to(device).eval()
        return cls(mods["flowNetF"], mods["netG"], light, crop=crop, graph=graph, topk=topk, backend=backend, precision=precision)

    def plan(self, B, H=128, W=128, precision=None):
        """The LightCNN's launches (FoldedLightCNN.plan); the frontaliser's are Frontalizer.plan's, plus one input and the matcher's."""
        return self.net.plan(B, H, W, precision)

    def _input(self, img):
        if self.backend == "torch":
            return torch_identity_input(img, self.crop)
        from . import ops
        return ops.identity_input(img.contiguous(), self.crop)

    @torch.no_grad()
    def feature(self, img):
        """get_gallery_fea's per-image path (models/ffwm_model.py:164-176) on img [B, 1 | 3, 128, 128] -> [B, 256] (a fresh tensor)."""
        if self.backend != "hip":
            return self.net._forward(self._input(img))[0]
        # on an arena of its own: the captured graph holds addresses inside the network's arena, which an eager pass at a larger batch
        # would make Arena.begin replace
        kept, self.net.arena = self.net.arena, self._eager_arena
        try:
            return self.net._forward(self._input(img))[0]
        finally:
            self.net.arena = kept

    @torch.no_grad()
    def set_gallery(self, keys, images, batch=64):
        """Store the gallery: keys (one per image) and the features of images [G, 1 | 3, 128, 128]."""
        keys = list(keys)
        if len(keys) != images.shape[0] or not keys:
            raise ValueError("set_gallery: one key per gallery image expected")
        feats = [self.feature(images[i:i + batch].to(self.net.device)).clone() for i in range(0, len(keys), batch)]
        self.gallery_keys, self.gallery_features = keys, torch.cat(feats, 0).contiguous()
        self._graph = None          # the matcher's grid and workspace depend on the gallery size

    @property
    def k(self):
        return None if self.gallery_features is None else min(max(10, self.topk), self.gallery_features.shape[0])

    def _forward(self, img):
        r = self.front._forward(img)
        fea = self.net._forward(self._input(r.fake_F128))[0]
        if self.gallery_features is None:
            return IdentityResult(r, fea, None, None)
        if self.backend == "torch":
            sim, idx = torch_cosine_topk(fea, self.gallery_features, self.k)
        else:
            from . import ops
            sim, idx = ops.cosine_topk(fea, self.gallery_features, self.k)
        return IdentityResult(r, fea, sim, idx)

    @torch.no_grad()
    def __call__(self, img_S):
        if not self.use_graph:
            return self._forward(img_S)
        if self._graph is None:
            # two warm-up passes outside the capture: kept Winograd transforms are published with a synchronisation
            self._graph = GraphedForward(self._forward)
        return self._graph(img_S)


# ------------------------------------------------------------------------------------------------ RankMeter
class RankMeter(object):
    """util.util.AverageMeter (util/util.py:141-181) over the matcher's indices instead of the features: rank-1 (top-k) hits per
    camera, summed per pose.  A probe name is `<id>_.._.._<camera>_...`: basename(name).split('_')[0] is the identity and [3] the
    camera; a gallery key is an identity."""

    DEG = collections.OrderedDict([("15", ["050", "140"]), ("30", ["041", "130"]), ("45", ["080", "190"]), ("60", ["090", "200"]),
                                   ("75", ["010", "120"]), ("90", ["110", "240"])])

    def __init__(self):
        self.deg = self.DEG
        self.reset()

    def reset(self):
        self.stat_dict = {}

    def update(self, top_idx, names, gallery_keys, topk=1):
        """top_idx [B, k >= topk]: gallery indices by falling similarity (FaceIdentifier's top_idx); one device-to-host copy."""
        rows = top_idx.detach().cpu().tolist() if torch.is_tensor(top_idx) else [list(r) for r in top_idx]
        if len(rows) != len(names):
            raise ValueError("RankMeter.update: one name per row of top_idx expected")
        for row, name in zip(rows, names):
            ss = os.path.basename(name).split("_")
            ids = [gallery_keys[i] for i in row]
            stat = self.stat_dict.setdefault(ss[3], {"correct": 0, "all": 0})
            stat["all"] += 1
            if ss[0] in ids[:topk]:
                stat["correct"] += 1

    def __str__(self):
        s, s1 = "", ""
        for k, v in self.stat_dict.items():
            s += "{}: [{}/{}, {}] \n".format(k, v["correct"], v["all"], 1.0 * v["correct"] / v["all"])
        for k, cameras in self.deg.items():
            seen = [self.stat_dict[c] for c in cameras if c in self.stat_dict]
            if not seen:
                continue          # (the reference raises KeyError here)
            _c, _a = sum(v["correct"] for v in seen), sum(v["all"] for v in seen)
            s += "{}: [{}/{}, {}] \n".format(k, _c, _a, 1.0 * _c / _a)
            s1 += " {:.2f} |".format(100.0 * _c / _a)
        return s + s1 + "\n"
