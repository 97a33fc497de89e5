"""netG's eval forward as a launch-lean path, and the reference's inference composition around it.

The reference's published use is inference: `test_ffwm.py` loads `latest_net_flowNetF.pth` and `latest_net_netG.pth` and runs
flowNetF -> WarpNet -> netG in eval mode (models/ffwm_model.py:183-189).  `nets.FFWM.forward` (= models/base_networks.py:314-347)
evaluates the generator as the training modules: eval-mode BatchNorm, LeakyReLU, `torch.cat`, `PixelShuffle`, `F.interpolate`
and the gate product are separate launches, each a full pass over the largest activations of the network.

`FoldedFFWM` computes the SAME function with

* the spectral-norm weights of eval mode, `weight_orig / (u . (W v))`, taken once from the state dict (float64, rounded once);
* eval-mode BatchNorm folded into the convolution in front of it -- conv blocks: w * s and (b - mean) * s + beta with
  s = gamma / sqrt(var + eps); PixelShuffle blocks: BatchNorm channel k scales conv channels 4k .. 4k + 3 and its shift is the
  bias of the shuffle kernel; residual blocks: both BatchNorms folded, the second one's shift and the 1 x 1 shortcut's bias summed
  into the bias of the second 3 x 3 convolution;
* every dense convolution once, bias + LeakyReLU in its epilogue where the serving kernel has one: the Winograd kernel
  (csrc/conv_winograd.hip) where `conv.winograd_ok` says so, csrc/conv_fwd.hip where `conv.fwd_route_ok` and the module route's
  own condition say so; the 7 x 7 stem, the 1 x 1 shortcuts and what neither kernel serves stay `F.conv2d(..., bias=None)`
  followed by `ffwm_bias_act_forward`;
* one launch per residual tail; the attention gates' tail and product as one launch that writes into the decoder's
  concatenation buffer, as do the shuffle epilogue and the bilinear upsampler (csrc/netg_eval.hip): cat(skip * att, dec,
  up(recon)) is never copied;
* all three warps in one `warp_many(..., flipcat=True)` launch, the image heads as one direct kernel each;
* the whole forward replayed from ONE captured hipGraph (`graph=True`).

`Frontalizer` is the reference's `test_forward` without a trainer: FoldedFlowNet, the image warp and FoldedFFWM inside one
captured graph.  Weights are snapshotted at construction: build from networks in `.eval()` and rebuild after the weights change.
"""
import collections
import contextlib
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .graphs import GraphedForward

LRELU, NONE, SIGMOID = 1, 0, 3
KINDS = ("winograd", "winograd_split", "conv_mfma", "vendor_conv", "bias_act", "add_act", "gate", "shuffle_bias_act", "image_head", "upsample2x",
         "warp_multi")

PRECISIONS = ("fp32", "bf16x3")
# A memory condition, not a tuned threshold: a layer whose split-route workspace (V and M of csrc/conv_winograd_gemm_split.hip) would
# make the executor's arena hold more than this keeps its fp32 route (netG's 195-channel layers at 128 x 128, batch 8: over 400 MB).
SPLIT_WORKSPACE_LIMIT = 256 << 20
# netG layers that stay on their fp32 route under precision="bf16x3": those where the split route measured slower than the layer's
# present route at BOTH batch 1 and batch 8 by more than the larger min-max spread (tools/split_conv_bench.py,
# profiles/wino_gemm_split.txt) -- the rule identity_eval.VENDOR_LAYERS was made by.  The measurement names none: e0.2.blocks.0 / .3
# (64 -> 64 at 128 x 128) are slower at batch 1 (34 against 23 us) and past SPLIT_WORKSPACE_LIMIT at batch 8, where the rule has nothing
# to compare.
SPLIT_EXCLUDED_LAYERS = frozenset()

_Layer = collections.namedtuple("_Layer", "w b k stride pad")
_Res = collections.namedtuple("_Res", "act slope inner_slope")


def sn_weight(sd, prefix):
    """The float64 weight of the layer `prefix` (with its trailing dot) of a state dict: for a spectrally normalised layer what
    torch.nn.utils.spectral_norm computes in eval mode from the stored u and v, weight_orig / (u . (W v)); else `weight`."""
    if prefix + "weight_orig" in sd:
        w = sd[prefix + "weight_orig"].detach().double()
        u, v = sd[prefix + "weight_u"].detach().double(), sd[prefix + "weight_v"].detach().double()
        return w / torch.dot(u, torch.mv(w.reshape(w.size(0), -1), v))
    return sd[prefix + "weight"].detach().double()


def torch_warp(images, flow):
    """WarpNet (models/base_networks.py:168-173) in PyTorch, for the torch backend."""
    return F.grid_sample(images, flow.permute(0, 2, 3, 1), mode="bilinear", padding_mode="zeros", align_corners=False)


class _Spec(object):
    """The shape of a float32 GPU tensor, for the route predicates of conv.py: plan() decides routes without a device."""

    is_cuda, dtype = True, torch.float32

    def __init__(self, *shape):
        self.shape = tuple(int(s) for s in shape)

    def dim(self):
        return len(self.shape)

    def size(self, i):
        return self.shape[i]

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n


def check_precision(who, precision, backend):
    if precision not in PRECISIONS:
        raise ValueError("%s: precision must be one of %s" % (who, ", ".join(repr(p) for p in PRECISIONS)))
    if backend == "torch" and precision != "fp32":
        raise ValueError("%s: the torch backend computes in the network's own dtype: precision='fp32' only" % who)
    return precision


@contextlib.contextmanager
def planned_precision(owner, precision):
    """plan(..., precision=...): the owner's routes under `precision` while the plan is drawn up."""
    kept = owner.precision
    owner.precision = kept if precision is None else check_precision(type(owner).__name__, precision, "hip")
    try:
        yield
    finally:
        owner.precision = kept


def split_workspace_bytes(B, C, H, W, K):
    """ffwm_conv3x3_wg_split_workspace_bytes without the library (plan() touches no device; test_wino_split_cpu.py holds the two
    together): V (a hi and a lo bf16 per entry, C rounded up to 32) and fp32 M, both padded to the 128 tile."""
    T = (B * ((H + 1) // 2) * ((W + 1) // 2) + 127) // 128 * 128
    return 16 * T * ((C + 31) // 32 * 32 + (K + 127) // 128 * 128) * 4


def split_route_ok(L, x):
    """The split route (csrc/conv_winograd_gemm_split.hip) serves a 3 x 3 / stride 1 / pad 1 layer with min(C, K) >= 32 whose
    workspace fits SPLIT_WORKSPACE_LIMIT."""
    K, C = L.w.shape[0], L.w.shape[1]
    B, _, H, W = x.shape
    return (L.k == 3 and L.stride == 1 and L.pad == 1 and min(C, K) >= 32
            and split_workspace_bytes(B, C, H, W, K) <= SPLIT_WORKSPACE_LIMIT)


def split_conv(owner, name, x, bias, epilogue, slope=0.2):
    """Layer `name` of a folded network on the split route: its split weights are made at the first EAGER call (never inside a
    capture: the rule conv.wg_entry states), the workspace is a slice of the owner's arena."""
    from . import ops
    L = owner.layers[name]
    U = owner._split_u.get(name)
    if U is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("%s: the split weights of %s would be made inside a graph capture; run one eager pass first" % (type(owner).__name__, name))
        U = owner._split_u[name] = ops.conv3x3_wg_split_weights(L.w)
    B, C, H, W = x.shape
    K = L.w.shape[0]
    ws = owner.arena.take(ops.conv3x3_wg_split_workspace_floats(B, C, H, W, K), x.device)
    return ops.conv3x3_wg_split(x, U, bias, epilogue, slope=slope, K=K, workspace=ws)


def conv_route(L, x, act, precision="fp32"):
    """Which kernel serves the convolution L (a layer tuple with w, k, stride, pad) on input x (a tensor or a _Spec): the predicates
    of conv.py, no thresholds here.  Shared by FoldedFFWM and identity_eval.FoldedLightCNN.  precision="bf16x3": "winograd_split"
    wherever split_route_ok says so."""
    from . import conv
    K, C = L.w.shape[0], L.w.shape[1]
    if precision == "bf16x3" and split_route_ok(L, x):
        return "winograd_split"
    if L.k == 3 and L.stride == 1 and L.pad == 1 and min(C, K) >= 32 and conv.winograd_ok(x, L.w, act):
        return "winograd"                                   # conv.winograd_eligible + winograd_ok
    if (L.k in (3, 4) and L.stride in (1, 2) and L.pad < L.k and min(C, K) >= 32 and (L.stride == 2 or L.k == 3)
            and conv.fwd_route_ok(x, L.w) and (L.stride == 2 or x.shape[2] <= 32)):
        return "conv_mfma"                                  # conv.fwd_eligible + MfmaFwdConv2d's condition
    return "vendor_conv"


# ------------------------------------------------------------------------------------------------ the three executors
class _PlanExec(object):
    """Shapes only: records (layer name, kind) of every launch the HIP executor would issue."""

    def __init__(self, owner):
        self.o, self.launches = owner, []

    def conv(self, name, x, act, slope=0.2):
        L = self.o.layers[name]
        route = self.o._route(name, x, act)
        self.launches.append((name, route))
        if route == "vendor_conv":
            self.launches.append((name, "bias_act"))
        B, _, H, W = x.shape
        return _Spec(B, L.w.shape[0], (H + 2 * L.pad - L.k) // L.stride + 1, (W + 2 * L.pad - L.k) // L.stride + 1)

    def stem(self, name, x, slope):
        return self.conv(name, x, LRELU, slope)

    def shortcut(self, name, x):
        self.launches.append((name, "vendor_conv"))
        return _Spec(x.shape[0], self.o.layers[name].w.shape[0], x.shape[2], x.shape[3])

    def add_act(self, name, a, s, act, slope):
        self.launches.append((name, "add_act"))
        return a

    def gate(self, name, a, s, skip, dst, want_att):
        self.launches.append((name, "gate"))
        return a if want_att else None

    def shuffle(self, name, h, bias, slope, dst):
        self.launches.append((name, "shuffle_bias_act"))

    def head(self, name, x):
        self.launches.append((name, "image_head"))
        return _Spec(x.shape[0], 3, x.shape[2], x.shape[3])

    def up(self, name, x, dst):
        self.launches.append((name, "upsample2x"))

    def warps(self, feats, flows):
        self.launches.append(("warp", "warp_multi"))
        return [_Spec(f.shape[0], 2 * f.shape[1], f.shape[2], f.shape[3]) for f in feats]

    def buffer(self, like, B, C, H, W):
        return _Spec(B, C, H, W)

    def channels(self, buf, a, b):
        return _Spec(buf.shape[0], b - a, buf.shape[2], buf.shape[3])


class _HipExec(_PlanExec):
    """The launches themselves; `launches` records them as plan() lists them."""

    def conv(self, name, x, act, slope=0.2):
        from . import flownet_eval, ops
        L = self.o.layers[name]
        route = self.o._route(name, x, act)
        self.launches.append((name, route))
        if route == "winograd_split":
            if L.b is None:
                return split_conv(self.o, name, x, None, "none")
            return split_conv(self.o, name, x, L.b, "lrelu" if act == LRELU else "bias", slope)
        if route == "winograd":
            return ops.conv3x3_winograd(x, L.w, L.b, act=act, slope=slope if act else 0.0, frozen=self.o._wino.setdefault(name, {}))
        if route == "conv_mfma":
            return flownet_eval.conv_mfma(x, L.w, L.b, L.stride, L.pad, False, act, slope, arena=self.o.arena)
        self.launches.append((name, "bias_act"))
        return flownet_eval.bias_act(F.conv2d(x, L.w, None, L.stride, L.pad), L.b, act, slope=slope)

    def shortcut(self, name, x):
        self.launches.append((name, "vendor_conv"))
        return F.conv2d(x, self.o.layers[name].w, None)

    def add_act(self, name, a, s, act, slope):
        from . import ops
        self.launches.append((name, "add_act"))
        return ops.add_act_forward(a, s, "sigmoid" if act == SIGMOID else "lrelu", slope)

    def gate(self, name, a, s, skip, dst, want_att):
        from . import ops
        self.launches.append((name, "gate"))
        return ops.sigmoid_gate_forward_strided(a, s, skip, out=dst, want_att=want_att)[1]

    def shuffle(self, name, h, bias, slope, dst):
        from . import ops
        self.launches.append((name, "shuffle_bias_act"))
        ops.shuffle_bias_act(h, bias, slope, out=dst)

    def head(self, name, x):
        from . import ops
        L = self.o.layers[name]
        self.launches.append((name, "image_head"))
        return ops.image_head(x, L.w, L.b)

    def up(self, name, x, dst):
        from . import ops
        self.launches.append((name, "upsample2x"))
        ops.upsample2x_bilinear(x, out=dst)

    def warps(self, feats, flows):
        from .external_function import warp_many
        self.launches.append(("warp", "warp_multi"))
        return warp_many(feats, flows, True)

    def buffer(self, like, B, C, H, W):
        return like.new_empty((B, C, H, W))

    def channels(self, buf, a, b):
        return buf[:, a:b]


class _TorchExec(object):
    """The same folded arithmetic as a PyTorch composition (any dtype, any device): pins the folding algebra without a GPU."""

    def __init__(self, owner):
        self.o, self.launches = owner, []

    @staticmethod
    def _act(h, act, slope):
        if act == LRELU:
            return F.leaky_relu(h, slope)
        return torch.sigmoid(h) if act == SIGMOID else h

    def conv(self, name, x, act, slope=0.2):
        L = self.o.layers[name]
        return self._act(F.conv2d(x, L.w, L.b, L.stride, L.pad), act, slope)

    def stem(self, name, x, slope):
        return self.conv(name, x, LRELU, slope)

    def shortcut(self, name, x):
        return F.conv2d(x, self.o.layers[name].w, None)

    def add_act(self, name, a, s, act, slope):
        return self._act(a + s, act, slope)

    def gate(self, name, a, s, skip, dst, want_att):
        att = torch.sigmoid(a + s)
        dst.copy_(skip * att)
        return att if want_att else None

    def shuffle(self, name, h, bias, slope, dst):
        dst.copy_(F.leaky_relu(F.pixel_shuffle(h, 2) + bias.view(1, -1, 1, 1), slope))

    def head(self, name, x):
        L = self.o.layers[name]
        return torch.sigmoid(F.conv2d(x, L.w, L.b, 1, 1))

    def up(self, name, x, dst):
        dst.copy_(F.interpolate(x, scale_factor=2, mode="bilinear"))

    def warps(self, feats, flows):
        out = []
        for f, fl in zip(feats, flows):
            w = torch_warp(f, fl)
            out.append(torch.cat((w, torch.flip(w, (3,))), 1))
        return out

    def buffer(self, like, B, C, H, W):
        return like.new_empty((B, C, H, W))

    def channels(self, buf, a, b):
        return buf[:, a:b]


# ------------------------------------------------------------------------------------------------ FoldedFFWM
class FoldedFFWM(object):
    """nets.FFWM's eval forward with folded weights (see the module docstring).

        folded = FoldedFFWM(netG.eval(), graph=True)
        rec32, rec64, rec128, att = folded(img, [flow32, flow64, flow128], return_att=True)

    backend: "hip" (float32 GPU network; the default on a GPU) or "torch" (a PyTorch composition of the same folded arithmetic, any
    dtype and device).  precision: "fp32" (the default) or, hip only, "bf16x3": the 3 x 3 / stride 1 layers that split_route_ok names
    run their Winograd GEMMs on the bf16 MFMA with hi / lo split operands (csrc/conv_winograd_gemm_split.hip; float32 tensors in and
    out, error bound and non-finite contract in include/ffwm_hip.h).  graph=True (hip only) replays the forward from one captured hipGraph, re-captured when the input shape
    changes: the OUTPUTS ARE STATIC BUFFERS THAT THE NEXT CALL OVERWRITES -- clone what must survive it.  return_features=True also
    returns {"e0".."e3", "d0".."d2", "dres0".."dres2"}, the outputs of those modules, and always runs un-captured."""

    def __init__(self, net, graph=False, backend=None, precision="fp32"):
        from . import nets
        if not isinstance(net, nets.FFWM):
            raise TypeError("FoldedFFWM: a nets.FFWM is expected")
        if net.training:
            raise ValueError("FoldedFFWM folds eval-mode BatchNorm statistics and spectral-norm weights: call net.eval() first")
        if not net.isflip:
            raise NotImplementedError("FoldedFFWM: the isflip=True generator only")
        p = next(net.parameters())
        if backend is None:
            backend = "hip" if p.is_cuda else "torch"
        if backend not in ("hip", "torch"):
            raise ValueError("FoldedFFWM: backend must be 'hip' or 'torch'")
        if backend == "hip" and not (p.is_cuda and p.dtype == torch.float32):
            raise NotImplementedError("FoldedFFWM: the hip backend takes float32 GPU networks only (backend='torch' for the rest)")
        if graph and backend != "hip":
            raise ValueError("FoldedFFWM: graph replay needs the hip backend")
        self.precision = check_precision("FoldedFFWM", precision, backend)
        self._split_u = {}
        self.backend, self.use_graph = backend, bool(graph)
        self.device, self.dtype = p.device, p.dtype
        self.n_levels = net.layers
        self.layers, self.res, self.sn_weights, self.shifts = {}, {}, {}, {}
        self.stem_slope = 0.2
        self._wino = {}
        self._graph = None
        self.last_launches = []
        if backend == "hip":
            from .flownet_eval import Arena
            self.arena = Arena()
        self._fold(net)

    # ---- construction: spectral-norm weights and folded BatchNorm ------------------------------------------------------
    def _fold(self, net):
        sd = net.state_dict()
        dt = self.dtype

        def bn_terms(path):
            bn = net.get_submodule(path)
            s = sd[path + ".weight"].double() / torch.sqrt(sd[path + ".running_var"].double() + bn.eps)
            return s, sd[path + ".bias"].double() - sd[path + ".running_mean"].double() * s          # scale, shift

        def add(path, bn=None, extra_bias=None, per=1, with_shift=True):
            """Layer `path` (a Conv2d) folded with the BatchNorm `bn` behind it; per = 4: a BatchNorm behind PixelShuffle(2)."""
            m = net.get_submodule(path)
            w = sn_weight(sd, path + ".")
            self.sn_weights[path] = w.to(dt)
            b = sd[path + ".bias"].double() if path + ".bias" in sd else torch.zeros(w.size(0), dtype=torch.float64, device=w.device)
            if bn is not None:
                s, shift = bn_terms(bn)
                sr = s.repeat_interleave(per) if per > 1 else s
                w = w * sr.view(-1, 1, 1, 1)
                b = b * sr
                if with_shift:
                    b = b + shift
                else:
                    self.shifts[path] = shift.to(dt).contiguous()
            if extra_bias is not None:
                b = b + extra_bias
            self.layers[path] = _Layer(w.to(dt).contiguous(), b.to(dt).contiguous(), m.kernel_size[0], m.stride[0], m.padding[0])

        def res(path):
            rb = net.get_submodule(path)
            add(path + ".blocks.0", path + ".blocks.1")
            add(path + ".blocks.3", path + ".blocks.4", extra_bias=sd[path + ".input.bias"].double())
            w_in = sn_weight(sd, path + ".input.")
            self.sn_weights[path + ".input"] = w_in.to(dt)
            self.layers[path + ".input"] = _Layer(w_in.to(dt).contiguous(), None, 1, 1, 0)
            sig = isinstance(rb.activ, nn.Sigmoid)
            if not sig and not isinstance(rb.activ, nn.LeakyReLU):
                raise NotImplementedError("FoldedFFWM: residual blocks end in LeakyReLU or Sigmoid")
            self.res[path] = _Res(SIGMOID if sig else LRELU, 0.2 if sig else rb.activ.negative_slope, rb.blocks[2].negative_slope)

        add("e0.0")
        self.stem_slope = net.e0[1].negative_slope
        res("e0.2")
        for i in range(1, self.n_levels + 1):
            add("e%d.0" % i, "e%d.1" % i)
            res("e%d.3" % i)
        for i in range(self.n_levels):
            add("d%d.0" % i, "d%d.2" % i, per=4, with_shift=False)
            res("dres%d.0" % i)
            res("dres%d.1" % i)
            add("rec%d.0" % i)
            add("att%d.0.0" % i, "att%d.0.1" % i)
            res("att%d.1" % i)

    # ---- routes -------------------------------------------------------------------------------------------------------
    def _route(self, name, x, act):
        """Which kernel serves convolution `name` on input x (a tensor or a _Spec): the predicates of conv.py, no thresholds here.
        precision="bf16x3" sends what split_route_ok names to the split route, but for the layers of SPLIT_EXCLUDED_LAYERS."""
        if act not in (LRELU, NONE) or name in SPLIT_EXCLUDED_LAYERS:
            return conv_route(self.layers[name], x, act)
        return conv_route(self.layers[name], x, act, self.precision)

    # ---- the forward, once for all executors ----------------------------------------------------------------------------
    def _res_block(self, ex, path, x, gate=None):
        r = self.res[path]
        h = ex.conv(path + ".blocks.0", x, LRELU, r.inner_slope)
        a = ex.conv(path + ".blocks.3", h, NONE)                 # its bias holds the second BatchNorm's shift and the shortcut's bias
        s = ex.shortcut(path + ".input", x)
        if gate is None:
            return ex.add_act(path, a, s, r.act, r.slope)
        skip, dst, want_att = gate
        return ex.gate(path, a, s, skip, dst, want_att)

    def _run(self, ex, x, flows, want_att=False, features=None, beside=None):
        n = self.n_levels
        # beside: a context in which the encoder, which needs no flow, is issued (Frontalizer: a side stream)
        with (beside() if beside is not None else contextlib.nullcontext()):
            f = self._res_block(ex, "e0.2", ex.stem("e0.0", x, self.stem_slope))
            enc = [f]
            for i in range(1, n + 1):
                f = self._res_block(ex, "e%d.3" % i, ex.conv("e%d.0" % i, f, LRELU))
                enc.append(f)
        if features is not None:
            features.update(("e%d" % i, e) for i, e in enumerate(enc))
        if callable(flows):
            flows = flows()                                      # a caller that computes the flows meanwhile, and joins the encoder
        skips = ex.warps([enc[n - 1 - i] for i in range(n)], [flows[i] for i in range(n)])
        fdec, recons, att = enc[-1], [], None
        for i in range(n):
            skip = skips[i]
            B, cs, H, W = skip.shape
            cd = self.shifts["d%d.0" % i].numel()
            buf = ex.buffer(x, B, cs + cd + (3 if recons else 0), H, W)
            ex.shuffle("d%d" % i, ex.conv("d%d.0" % i, fdec, NONE), self.shifts["d%d.0" % i], 0.2, ex.channels(buf, cs, cs + cd))
            g = ex.conv("att%d.0.0" % i, skip, LRELU)
            last = i == n - 1
            a = self._res_block(ex, "att%d.1" % i, g, gate=(skip, ex.channels(buf, 0, cs), last and (want_att or features is not None)))
            if last:
                att = a
            if recons:
                ex.up("up%d" % i, recons[-1], ex.channels(buf, cs + cd, cs + cd + 3))
            if features is not None:
                features["d%d" % i] = ex.channels(buf, cs, cs + cd)
            fdec = self._res_block(ex, "dres%d.1" % i, self._res_block(ex, "dres%d.0" % i, buf))
            if features is not None:
                features["dres%d" % i] = fdec
            recons.append(ex.head("rec%d.0" % i, fdec))
        return tuple(recons[-3:]) + (att,)

    def plan(self, B, H, W, precision=None):
        """The ordered launches of one forward at batch B and H x W images as [(layer name, kind)], kind in KINDS; no device is touched.
        precision: the plan the hip backend would follow under that precision (default: this object's own)."""
        ex = _PlanExec(self)
        with planned_precision(self, precision):
            self._run(ex, _Spec(B, 3, H, W), [_Spec(B, 2, H >> (self.n_levels - 1 - i), W >> (self.n_levels - 1 - i)) for i in range(self.n_levels)], True)
        return ex.launches

    def _forward(self, x, flows, want_att=True, features=None, beside=None):
        if self.backend == "torch":
            return self._run(_TorchExec(self), x, flows, want_att, features)
        if not (x.is_cuda and x.dtype == torch.float32):
            raise NotImplementedError("FoldedFFWM: the hip backend takes float32 GPU tensors")
        self.arena.begin(x.device)
        ex = _HipExec(self)
        out = self._run(ex, x.contiguous(), flows, want_att, features, beside)
        self.last_launches = ex.launches
        return out

    def _forward_with_att(self, x, *flows):
        return self._forward(x, list(flows), True)

    @torch.no_grad()
    def __call__(self, x, flows, return_att=False, return_features=False):
        if return_features:
            feats = {}
            out = self._forward(x, list(flows), True, feats)
            return (out if return_att else out[:3]) + (feats,)
        if not self.use_graph:
            out = self._forward(x, list(flows), return_att)
            return out if return_att else out[:3]
        if self._graph is None:
            # two warm-up passes outside the capture: a layer's first Winograd call synchronises to publish its kept transform
            self._graph = GraphedForward(self._forward_with_att)
        out = self._graph(x, *flows)
        return out if return_att else out[:3]


# ------------------------------------------------------------------------------------------------ Frontalizer
FrontalizerResult = collections.namedtuple("FrontalizerResult", "fake_F128 fake_F64 fake_F32 img_S_warp att flows")


class Frontalizer(object):
    """FFWMModel.test_forward (models/ffwm_model.py:183-189) without a trainer: flows = flowNetF(img_S); img_S_warp = WarpNet(img_S,
    flow128); fake_F32 / 64 / 128, att = netG(img_S, [flow32, flow64, flow128]); att = mean of its first 64 channels.

        f = Frontalizer.from_checkpoints("checkpoints/ffwm", "latest")
        r = f(img_S)            # r.fake_F128, r.fake_F64, r.fake_F32, r.img_S_warp, r.att, r.flows = (flow128, flow64, flow32)

    On the GPU FoldedFlowNet, the image warp and FoldedFFWM run inside ONE captured hipGraph (graph=True), netG's encoder,
    which needs no flow, on a side stream beside the flow net.  THE RESULT'S TENSORS ARE STATIC BUFFERS THAT THE NEXT CALL OVERWRITES.  The
    guided filter (it needs the ground truth) and the LightCNN feature are the caller's: INTEGRATION.md."""

    def __init__(self, flowNetF, netG, graph=True, backend=None, precision="fp32"):
        if flowNetF.training or netG.training:
            raise ValueError("Frontalizer snapshots eval-mode weights: call .eval() on both networks first")
        self.netG = FoldedFFWM(netG, graph=False, backend=backend, precision=precision)          # the flow net stays fp32
        self.backend, self.precision = self.netG.backend, self.netG.precision
        if graph and self.backend != "hip":
            raise ValueError("Frontalizer: graph replay needs the hip backend")
        self.use_graph = bool(graph)
        if self.backend == "hip":
            from .external_function import WarpNet
            from .flownet_eval import FoldedFlowNet
            self.flow = FoldedFlowNet(flowNetF, graph=False)
            self.warp = WarpNet()
            self._side = None
        else:
            self.flow, self.warp = flowNetF, torch_warp
        self._graph = None

    @classmethod
    def from_checkpoints(cls, load_dir, epoch="latest", ngf=64, device=None, graph=True, backend=None, precision="fp32"):
        """Load `<epoch>_net_flowNetF.pth` and `<epoch>_net_netG.pth` as the reference's BaseModel.save_networks wrote them
        (models/base_model.py:172-229) into nets.FlowNet(ngf) / nets.FFWM(sn=True); no trainer is constructed."""
        from . import nets
        device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        mods = {"flowNetF": nets.FlowNet(ngf), "netG": nets.FFWM(sn=True)}
        for name, mod in mods.items():
            sd = torch.load(os.path.join(load_dir, "%s_net_%s.pth" % (epoch, name)), map_location="cpu")
            if hasattr(sd, "_metadata"):
                del sd._metadata
            mod.load_state_dict(sd)
            mod.to(device).eval()
        return cls(mods["flowNetF"], mods["netG"], graph=graph, backend=backend, precision=precision)

    def plan(self, B, H, W, precision=None):
        """netG's launches (FoldedFFWM.plan); the flow net's and the image warp's are FoldedFlowNet's and one `warp` launch."""
        return self.netG.plan(B, H, W, precision)

    def _forward(self, img):
        if self.backend == "torch":
            flows = self.flow(img)
            warped = self.warp(img, flows[0])
            r32, r64, r128, att = self.netG._forward(img, [flows[2], flows[1], flows[0]], True)
        else:
            cur = torch.cuda.current_stream(img.device)
            if self._side is None:
                self._side = torch.cuda.Stream(device=img.device)
            side = self._side
            box = {}

            # netG's encoder goes to the side stream and the flow net stays on the caller's, not the other way round: FoldedFlowNet
            # forks a stream of its own, and a stream forked from a side branch and joined back into it crashes hipStreamEndCapture
            # (ROCm 7.0, profiles/r04_dp_capture_modes.txt) -- so both forks start from the captured stream itself
            @contextlib.contextmanager
            def beside():
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    yield

            def flows_then_join():
                fl = box["flows"] = self.flow(img)
                box["warp"] = self.warp(img, fl[0])
                cur.wait_stream(side)                            # the encoder's features are ready
                return [fl[2], fl[1], fl[0]]
            r32, r64, r128, att = self.netG._forward(img, flows_then_join, True, beside=beside)
            flows, warped = box["flows"], box["warp"]
        att = torch.mean(att[:, :64, :, :], (1,), keepdim=True)
        return FrontalizerResult(r128, r64, r32, warped, att, tuple(flows))

    @torch.no_grad()
    def __call__(self, img_S):
        if not self.use_graph:
            return self._forward(img_S)
        if self._graph is None:
            # two warm-up passes outside the capture: kept Winograd transforms are published with a synchronisation
            self._graph = GraphedForward(self._forward)
        return self._graph(img_S)
