"""The reference's callers of the custom ops, restated on top of the HIP operator API.

``AffineRegularizationLoss`` / ``MultiAffineRegularizationLoss`` (/root/reference/models/losses.py:163-223)
are the only place the reference really runs BlockExtractor + LocalAttnReshape (FlowNet pre-training,
models/flownet_model.py:30-31,67-68): on 1-channel pixel-coordinate grids, with the constant flow kz//2,
kz = 3 / 5 / 7 on the 32 / 64 / 128 px flows.  Same constructor arguments, same call, same arithmetic;
the two ops are the gfx950 kernels behind ``ffwm_amd.external_function``.  ``fused=True`` evaluates the
same loss and its gradient with ONE kernel per scale (csrc/affine_reg.hip) instead of
6 launches forward + ~10 backward per coordinate grid.

``IdentityLoss`` (/root/reference/models/losses.py:76-112) is the identity term of FFWM's own training, with the ``--crop``
option of train_ffwm.py: the network's input stage -- channel mean, centre-face crop, resize -- is one kernel per direction
(csrc/lightcnn_eval.hip).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

from . import ops
from .external_function import BlockExtractor, LocalAttnReshape, Resample2d


class _FusedAffineReg(Function):
    """loss and d(loss)/d(flow) from one launch (csrc/affine_reg.hip)."""

    @staticmethod
    def forward(ctx, flow, ktk, kz):
        loss, grad = ops.affine_regularization(flow, ktk, kz, want_grad=flow.requires_grad)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        (grad,) = ctx.saved_tensors
        return (grad * grad_output if grad is not None else None), None, None


class _FusedSamplingCorrectness(Function):
    """The correctness loss of one scale and d(loss)/d(flow) from one call (csrc/sampling_correctness.hip); the features, the
    correlation maximum and the mask get no gradient."""

    @staticmethod
    def forward(ctx, flow, source, target, corr_max, mask, eps):
        out, grad, _ = ops.sampling_correctness(source, target, flow, corr_max, mask, eps, want_grad=ctx.needs_input_grad[0])
        if grad is not None:
            ctx.save_for_backward(grad, out)
        return out[0]

    @staticmethod
    def backward(ctx, grad_output):
        if not ctx.saved_tensors:
            return (None,) * 6
        grad, out = ctx.saved_tensors
        return (grad * (grad_output / out[1]), None, None, None, None, None)


class _FusedLandmarks(Function):
    """The landmark loss of all scales and d(loss)/d(flow) of every flow that needs one, from one call (csrc/landmark_loss.hip);
    the landmarks and the gate get no gradient.  `owner.skipped` receives the call's device counter."""

    @staticmethod
    def forward(ctx, lm_S, lm_F, gate, divisors, weights, owner, *flows):
        ctx.wants = tuple(ctx.needs_input_grad[6:])
        out, grads, skipped = ops.landmark_loss([f.contiguous() for f in flows], lm_S, lm_F, gate.contiguous(), divisors, weights, ctx.wants)
        owner.skipped = skipped
        ctx.save_for_backward(*[g for g in grads if g is not None])
        return out[0]

    @staticmethod
    def backward(ctx, grad_output):
        saved = iter(ctx.saved_tensors)
        return (None,) * 6 + tuple(next(saved) * grad_output if want else None for want in ctx.wants)


def _landmarks_take_kernel(flows, lm_S, lm_F, gate):
    """The fused kernel serves 1 .. 4 square float32 / float64 flows of one batch with int64 landmarks and a gate of the flows'
    dtype, all on the GPU, when the gate wants no gradient."""
    if not 1 <= len(flows) <= 4:
        return False
    first = flows[0]
    if first.dtype not in (torch.float32, torch.float64) or gate.requires_grad:
        return False
    if not (lm_S.is_cuda and lm_F.is_cuda and gate.is_cuda and lm_S.dtype == torch.int64 and lm_F.dtype == torch.int64):
        return False
    if gate.dtype != first.dtype or lm_S.dim() != 3 or lm_S.numel() == 0 or lm_S.shape != lm_F.shape or gate.shape != lm_S.shape:
        return False
    return all(f.is_cuda and f.dtype == first.dtype and f.dim() == 4 and f.shape[0] == lm_S.shape[0] and f.shape[1] == 2
               and f.shape[2] == f.shape[3] and f.shape[2] > 0 for f in flows)


class _FusedClassifier(Function):
    """Mean cross entropy, d(loss)/d(logits), prec@1 and prec@5 from one call (csrc/softmax_xent.hip); the gradient is kept from the
    forward call.  `owner` receives prec1, prec5, rank and the device counter of skipped rows."""

    @staticmethod
    def forward(ctx, logits, target, owner):
        want = ctx.needs_input_grad[0]
        out, _, rank, grad, skipped = ops.softmax_xent(logits, target, want_grad=want)
        owner.prec1, owner.prec5, owner.rank, owner.skipped = out[1], out[2], rank, skipped
        if want:
            ctx.save_for_backward(grad)
        return out[0]

    @staticmethod
    def backward(ctx, grad_output):
        if not ctx.saved_tensors:
            return None, None, None
        return ctx.saved_tensors[0] * grad_output, None, None


def accuracy(output, target, topk=(1,)):
    """lightcnn/finetune.py:294-307: precision@k in percent, from topk's indices."""
    maxk = max(topk)
    pred = output.topk(maxk, 1, True, True)[1].t()
    correct = pred.eq(target.view(1, -1).expand_as(pred))
    return [correct[:k].reshape(-1).float().sum(0).mul_(100.0 / target.size(0)) for k in topk]


class ClassifierLoss(nn.Module):
    """nn.CrossEntropyLoss plus accuracy(output, target, (1, 5)) of every step (lightcnn/finetune.py:109,152-159).  forward(logits
    [B, N], target int64 [B]) -> loss; ``.prec1`` / ``.prec5`` hold the step's precisions as scalars on the logits' device.

    ``fused=True``: loss, gradient and both precisions from one call of csrc/softmax_xent.hip wherever it applies (contiguous float32 /
    float64 logits on the GPU); ``.rank`` and ``.skipped`` are then set as well.  Ties in the logits go to the lower index there, where
    topk leaves their order open, and a target outside [0, N) is skipped and counted instead of raising.  Everywhere else: the composition."""

    def __init__(self, fused=False):
        super().__init__()
        self.fused = bool(fused)
        self.prec1 = self.prec5 = self.rank = self.skipped = None

    def forward(self, logits, target):
        if (self.fused and logits.is_cuda and target.is_cuda and logits.dim() == 2 and logits.is_contiguous() and logits.numel() > 0
                and logits.dtype in (torch.float32, torch.float64) and target.dtype == torch.int64 and target.dim() == 1):
            return _FusedClassifier.apply(logits, target, self)
        loss = F.cross_entropy(logits, target)
        self.rank = self.skipped = None
        self.prec1, self.prec5 = accuracy(logits.detach(), target, (1, min(5, logits.shape[1])))
        return loss


def affine_residual_kernels(kz):
    """The kz^2 filters [kz^2, 1, kz, kz] (float64) whose responses, dotted with a window of the sampling grid, give the squared
    distance of that window from the nearest affine map (what losses.py:192-199 builds).  With the design matrix D of the window's
    kz^2 cells -- one row (y, x, 1) per cell, y-major -- the least-squares affine fit of a window g is P g, P = D (D^T D)^-1 D^T,
    and the residual is R g with R = I - P.  R is a symmetric projector, so the reference's K^T K (K = P - I) is R itself up to
    rounding; it is formed as R^T R here to follow the reference's arithmetic to the last bits the fixtures pin."""
    ys, xs = torch.meshgrid(torch.arange(kz, dtype=torch.float64), torch.arange(kz, dtype=torch.float64), indexing="ij")
    design = torch.stack((ys.reshape(-1), xs.reshape(-1), torch.ones(kz * kz, dtype=torch.float64)), 1)          # [kz^2, 3]
    fit = design @ torch.linalg.solve(design.T @ design, design.T)                                                # P
    resid = fit - torch.eye(kz * kz, dtype=torch.float64)                                                         # -R
    return (resid.T @ resid).reshape(kz * kz, 1, kz, kz)


class AffineRegularizationLoss(nn.Module):
    """Penalises the deviation of every kz x kz window of the sampling grid from an affine map
    (losses.py:181-223).  kernel = K^T K with K = A (A^T A)^-1 A^T - I, A = [row, col, 1]."""

    def __init__(self, kz, fused=False):
        super().__init__()
        self.kz = kz
        self.fused = fused        # True: the whole loss (and its gradient) as one HIP kernel per scale
        self.extractor = BlockExtractor(kernel_size=kz)
        self.reshape = LocalAttnReshape()
        self.kernel = affine_residual_kernels(kz)
        self._cache = {}

    def _weights(self, like):
        """self.kernel.type_as(flow) of the reference, cached per (device, dtype): the reference re-uploads
        the CPU tensor on every call (a synchronous host-to-device copy)."""
        key = (like.device, like.dtype)
        w = self._cache.get(key)
        if w is None:
            w = self._cache[key] = self.kernel.to(device=like.device, dtype=like.dtype)
        return w

    def forward(self, flow_fields):
        weights = self._weights(flow_fields)
        if self.fused:
            return _FusedAffineReg.apply(flow_fields, weights.view(self.kz ** 2, self.kz ** 2), self.kz)
        grid = self.flow2grid(flow_fields)
        grid_x = grid[:, 0, :, :].unsqueeze(1)
        grid_y = grid[:, 1, :, :].unsqueeze(1)
        return self.calculate_loss(grid_x, weights) + self.calculate_loss(grid_y, weights)

    @staticmethod
    def _patch_products(grid, weights):
        """F.conv2d(grid, weights) of the reference (models/losses.py:196: ONE input channel, kz^2 output channels) as im2col +
        matmul on the GPU: with one input channel the vendor library's heuristics pick an NHWC implicit-GEMM data-gradient kernel
        (igemm_bwd_gtcx35_nhwc_fp32 ... bt256x32x4) that reads out of bounds -- a GPU memory fault whenever the neighbouring
        page is unmapped (seen under rocgdb after a trainer had shaped the allocator).  Same sums, rocBLAS instead."""
        if not grid.is_cuda:
            return F.conv2d(grid, weights)
        b, _, h, w = grid.shape
        kz = weights.shape[-1]
        cols = F.unfold(grid, kz)                                    # [b, kz*kz, (h - kz + 1) (w - kz + 1)]
        return torch.matmul(weights.reshape(weights.shape[0], -1), cols).view(b, weights.shape[0], h - kz + 1, w - kz + 1)

    def calculate_loss(self, grid, weights):
        results = self._patch_products(grid, weights)                # K^T K patch: [b, kz*kz, h, w]
        b, c, h, w = results.size()
        kernels_new = self.reshape(results, self.kz)                 # HIP local_attn_reshape
        f = torch.full((b, 2, h, w), float(int(self.kz / 2)), dtype=kernels_new.dtype, device=kernels_new.device)
        grid_H = self.extractor(grid, f)                             # HIP block_extractor
        result = F.avg_pool2d(grid_H * kernels_new, self.kz, self.kz)
        return torch.mean(result) * self.kz ** 2

    @staticmethod
    def flow2grid(flow_field):
        return flow_field.add(1.0).div(2.0).mul(128.0)


class MultiAffineRegularizationLoss(nn.Module):
    """losses.py:163-179: one AffineRegularizationLoss per flow scale; ``kz_dic`` maps layer -> kz and the
    flows are matched to the layers in DESCENDING layer order (flownet_model.py:31 builds {1: 7, 2: 5, 3: 3}
    and :68 passes the flows smallest first)."""

    def __init__(self, kz_dic, fused=False):
        super().__init__()
        self.kz_dic = kz_dic
        self.method_dic = {key: AffineRegularizationLoss(kz_dic[key], fused=fused) for key in kz_dic}
        self.layers = sorted(kz_dic, reverse=True)

    def forward(self, flow_fields):
        loss = 0
        for i in range(len(flow_fields)):
            loss = loss + self.method_dic[self.layers[i]](flow_fields[i])
        return loss


# ------------------------------------------------------------------------------------------------
# The other two losses of FlowNet pre-training (models/flownet_model.py:64-72)
class LandmarkLoss(nn.Module):
    """MSE between the flow sampled at the frontal landmarks and the (normalised) profile landmarks
    (losses.py:61-74).  flow [B,2,s,s]; lm_S / lm_F integer pixel coordinates [B,L,2]; gate [B,L,2].
    ``fused=True``: loss and gradient from one call of csrc/landmark_loss.hip wherever it applies (GPU tensors, a float32 /
    float64 flow); a landmark outside the plane is then skipped and counted in ``.skipped`` (a device int32 scalar, the last
    call's) where ``gather`` would raise a device assert.  Everywhere else the composition below, unchanged."""

    def __init__(self, fused=False):
        super().__init__()
        self.fused = fused
        self.skipped = None

    def forward(self, flow, lm_S, lm_F, gate):
        if self.fused and _landmarks_take_kernel([flow], lm_S, lm_F, gate):
            return _FusedLandmarks.apply(lm_S, lm_F, gate, (1,), (1.0,), self, flow)
        side = flow.size(-1)
        # the flow vectors at the frontal landmarks: pixel (x, y) of the row-major plane is element y * side + x
        cell = (lm_F[..., 1] * side + lm_F[..., 0]).unsqueeze(1).expand(-1, 2, -1)             # [B, 2, L]
        picked = flow.flatten(2).gather(2, cell).transpose(1, 2)                                # [B, L, 2] = (flow_x, flow_y) per landmark
        wanted = lm_S.to(flow.dtype) * (2.0 / side) - 1                                         # profile landmarks on the [-1, 1] grid
        return F.mse_loss(picked * gate, wanted * gate)


class MultiScaleLDLoss(nn.Module):
    """losses.py:114-126: LandmarkLoss on the 128 / 64 / 32 px flows, weights 1000 / 1000 / 1500.  The integer
    landmarks are divided by the scale with INTEGER division: that is what ``lm.div(scale)`` did for integer
    tensors in the reference's pinned PyTorch 1.5.0 (README.md:14); from 1.6 on ``div`` is true division and
    the reference's own ``torch.gather`` call rejects the float index.
    ``fused=True``: ONE call of csrc/landmark_loss.hip for the three scales (divisors 128 // s) wherever it applies, see
    LandmarkLoss; the gradients of the flows come without float atomics, so two runs agree bit for bit."""

    def __init__(self, fused=False):
        super().__init__()
        self.criterionLD = LandmarkLoss()
        self.weights = [1000, 1000, 1500]
        self.img_size = 128
        self.fused = fused
        self.skipped = None          # the device counter of the last fused call; nothing in a step reads it back

    def forward(self, flows, lm_S, lm_F, gate):
        if self.fused and len(flows) <= len(self.weights) and _landmarks_take_kernel(flows, lm_S, lm_F, gate) \
                and all(0 < f.size(3) <= self.img_size for f in flows):
            divisors = tuple(self.img_size // f.size(3) for f in flows)
            return _FusedLandmarks.apply(lm_S, lm_F, gate, divisors, tuple(float(w) for w in self.weights[:len(flows)]), self, *flows)
        ld_loss = 0
        for i, flow in enumerate(flows):
            scale = self.img_size // flow.size(3)
            lms = torch.div(lm_S, scale, rounding_mode="floor") if scale > 1 else lm_S
            lmf = torch.div(lm_F, scale, rounding_mode="floor") if scale > 1 else lm_F
            ld_loss = ld_loss + self.weights[i] * self.criterionLD(flow, lms, lmf, gate)
        return ld_loss


class PerceptualCorrectness(nn.Module):
    """losses.py:322-396 (the sampling-correctness loss of Global-Flow-Local-Attention) on the bilinear
    path the reference really takes (``use_bilinear_sampling=True``): for every flow scale,
    exp(-cos(warp(source_vgg, flow), target_vgg) / max_j cos(source_vgg_j, target_vgg)) averaged under the
    mask.  ``vgg`` maps an image to {'relu1_1': ..., ...}; ``warp`` is WarpNet (HIP) or a stand-in.

    Result-preserving difference: the VGG features and the N^2 x N^2 correlation maximum do not depend on
    the flow, and neither the images nor VGG are trained, so they are evaluated under no_grad -- the
    reference back-propagates through a [B, N^2, N^2] matrix (1 GiB per sample at relu1_1) for nothing."""

    def __init__(self, vgg, warp, layer=("relu1_1", "relu2_1", "relu3_1", "relu4_1"), resample=None, fused=False,
                 corr_precision="fp32"):
        super().__init__()
        # "bf16x3": the correlation maximum of the MFMA branch on the bf16 matrix instruction with hi/lo-split operands
        # (ops.correlation_colmax); the bmm + max branch (small grids, CPU, float64) is the same whatever is asked
        self.corr_precision = ops.check_corr_precision(corr_precision, "PerceptualCorrectness")
        self.vgg = vgg
        self.warp = warp
        # True: warp, cosine, exp, mask and the sums of a scale as one HIP kernel (csrc/sampling_correctness.hip) wherever it applies
        self.fused = fused
        self.layer = list(layer)
        self.eps = 1e-8
        # losses.py:329: the Gaussian-weighted resampler of the `use_bilinear_sampling=False` branch (the one call site
        # of resample2d in the reference; its flow argument is handed over unscaled, exactly as the reference does)
        self.resample = resample if resample is not None else Resample2d(4, 1, sigma=2)

    def forward(self, target, source, flow_list, used_layers, norm_mask=None, use_bilinear_sampling=True):
        used_layers = sorted(used_layers, reverse=True)
        with torch.no_grad():
            self.target_vgg, self.source_vgg = self.vgg(target), self.vgg(source)
        loss = 0
        for i in range(len(flow_list)):
            loss = loss + self.calculate_loss(flow_list[i], self.layer[used_layers[i]], norm_mask, use_bilinear_sampling)
        return loss

    def calculate_loss(self, flow, layer, norm_mask=None, use_bilinear_sampling=False):       # the reference's default (:342)
        target_vgg = self.target_vgg[layer]
        source_vgg = self.source_vgg[layer]
        b, c, h, w = target_vgg.shape
        flow = F.interpolate(flow, [h, w])
        target_all = target_vgg.reshape(b, c, -1)                       # [b, C, N2]
        with torch.no_grad():
            source_all = source_vgg.reshape(b, c, -1).transpose(1, 2)   # [b, N2, C]
            source_norm = source_all / (source_all.norm(dim=2, keepdim=True) + self.eps)
            target_norm = target_all / (target_all.norm(dim=1, keepdim=True) + self.eps)
            # (the MFMA kernels want >= 192 workgroups of 128 columns, both precisions; below that rocBLAS + max is as fast)
            if source_norm.is_cuda and source_norm.dtype == torch.float32 and c in (64, 128, 256) and b * ((h * w + 127) // 128) >= 192:
                correction_max = ops.correlation_colmax(source_norm, target_norm, precision=self.corr_precision)   # MFMA, no [b, N2, N2] matrix
            else:
                correction_max = torch.bmm(source_norm, target_norm).max(dim=1)[0]  # [b, N2]
        if self._takes_kernel(flow, source_vgg, target_vgg, use_bilinear_sampling):
            mask = None
            if norm_mask is not None:
                mask = F.interpolate(norm_mask, size=(h, w)).reshape(-1, h * w).to(flow.dtype).contiguous()
            return _FusedSamplingCorrectness.apply(flow.contiguous(), source_vgg.contiguous(), target_vgg.contiguous(),
                                                   correction_max.contiguous(), mask, self.eps)
        if use_bilinear_sampling:                                                  # losses.py:356-357
            input_sample = self.warp(source_vgg, flow).reshape(b, c, -1)
        else:                                                                      # losses.py:358-359 -> resample2d
            input_sample = self.resample(source_vgg.contiguous(), flow.contiguous()).reshape(b, c, -1)
        correction_sample = F.cosine_similarity(input_sample, target_all)          # [b, N2]
        loss_map = torch.exp(-correction_sample / (correction_max + self.eps))
        e1 = _exp_minus_one(loss_map.dtype)      # exp(-1) rounded in the map's dtype, as a host constant (no H2D copy: capturable)
        if norm_mask is None:
            return torch.mean(loss_map) - e1
        norm_mask = F.interpolate(norm_mask, size=(h, w)).reshape(-1, h * w)
        return (torch.sum(norm_mask * loss_map) - e1) / (torch.sum(norm_mask) + self.eps)

    def _takes_kernel(self, flow, source_vgg, target_vgg, use_bilinear_sampling):
        """The fused kernel serves the bilinear branch on float32 / float64 GPU tensors when only the flow wants a gradient (the
        features' gradient exists in the composition alone); the resample2d branch stays composed."""
        if not (self.fused and use_bilinear_sampling and flow.is_cuda and source_vgg.is_cuda and target_vgg.is_cuda):
            return False
        if flow.dtype not in (torch.float32, torch.float64) or source_vgg.dtype != flow.dtype or target_vgg.dtype != flow.dtype:
            return False
        return not (source_vgg.requires_grad or target_vgg.requires_grad)


_E1 = {}


def _exp_minus_one(dtype):
    if dtype not in _E1:
        _E1[dtype] = float(torch.exp(torch.tensor(-1.0, dtype=dtype)))
    return _E1[dtype]


# ================================================================================= identity loss (csrc/lightcnn_eval.hip)
def identity_network_input(img, crop=False):
    """The identity network's input [B, 1, H, W] of img [B, Cin, H, W], differentiable: on float32 GPU tensors one kernel per
    direction (external_function.IdentityInputFunction), everywhere else (CPU, float64, half) the PyTorch composition
    `identity_eval.torch_identity_input`, which autograd differentiates."""
    if img.is_cuda and img.dtype == torch.float32:
        from .external_function import IdentityInputFunction
        return IdentityInputFunction.apply(img, bool(crop))
    from .identity_eval import crop_grid, torch_identity_input
    if crop and img.dtype != torch.float32:
        # the reference builds its grid in float32 and casts it (`build_grid(b, 98).type_as(out)`, models/losses.py:85): a float64 run
        # samples at the float32 grid's coordinates, and so does this one
        return torch_identity_input(img, True, grid=crop_grid(img.shape[0], 98, device=img.device).type_as(img))
    return torch_identity_input(img, crop)


class IdentityLoss(nn.Module):
    """The reference's IdentityLoss (models/losses.py:76-112): same constructor, same forward(out, gt), same build_grid(b, d).
        loss = L1(fc(out), fc(gt)) + L1(pool(out), pool(gt)),   (_, fc, pool) = lightcnn(input), the features of gt under no_grad
    with the network's input the channel mean or, with crop=True (train_ffwm.py --crop), the centre-face crop resized back to the
    image's size: WarpNet(build_grid(b, 98)) and a bilinear F.interpolate.  The reference warps and resizes the 3-channel image and
    takes the mean last; here the mean comes first (as FFWMModel.test does, models/ffwm_model.py:196-200) and the crop runs on one
    channel.  Both steps are linear and act on different axes -- the mean over channels, the crop over the plane -- so they commute and
    the two orders differ by rounding only.  The crop is defined for 128 x 128 images."""

    def __init__(self, lightcnn, crop=False):
        super().__init__()
        self.lightcnn = lightcnn
        self.criterionL1 = torch.nn.L1Loss()
        self.crop = crop

    def forward(self, out, gt):
        _, fc_out, pool_out = self.lightcnn(identity_network_input(out, self.crop))
        with torch.no_grad():
            _, fc_gt, pool_gt = self.lightcnn(identity_network_input(gt, self.crop))
        loss = self.criterionL1(fc_out, fc_gt.detach())
        loss = loss + self.criterionL1(pool_out, pool_gt.detach())
        return loss

    def build_grid(self, b, d):
        """[b, 2, d, d]: linspace(-d // 2, d // 2, d) around the face centre (64, 77) of a 128 x 128 image, over 64."""
        from .identity_eval import crop_grid
        return crop_grid(b, d)


# ================================================================================= fused L1 terms (csrc/l1_loss.hip)
class _L1Terms(torch.autograd.Function):
    """out[n_slots] = sum over the terms of weight * mean |x m - y m| (models/ffwm_model.py:107-139: the pixel, perceptual, illumination
    and identity terms of backward_G), ONE launch forward and ONE backward for all terms instead of 5-7 element-wise / reduction
    launches per term and direction.  y and the masks are data / detached features in every term of the reference: no gradient."""

    @staticmethod
    def forward(ctx, n_slots, meta, *xs):
        from . import ops
        xs = [x.contiguous() for x in xs]
        terms = []
        for x, (y, m, segments) in zip(xs, meta):
            row = x.numel() // max(x.shape[0], 1)
            terms.append((x, y.contiguous(), None if m is None else m.contiguous(),
                          [(x0, y0, rows, w / float(max(rows * row, 1)), slot) for (x0, y0, rows, w, slot) in segments]))
        # saved through autograd (not parked on ctx): an in-place change of x, y or a mask between forward and backward is then caught by
        # the version check instead of silently producing the gradient of other data
        flat, layout = [], []
        for (x, y, m, segs) in terms:
            layout.append((len(flat), m is not None, segs))
            flat += [x, y] + ([m] if m is not None else [])
        ctx.save_for_backward(*flat)
        ctx.layout = layout
        return ops.l1_multi_forward(terms, n_slots)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        from . import ops
        saved = ctx.saved_tensors
        terms = [(saved[i], saved[i + 1], saved[i + 2] if has_m else None, segs) for (i, has_m, segs) in ctx.layout]
        grads = ops.l1_multi_backward(terms, grad_out, ctx.needs_input_grad[2:])
        return (None, None) + tuple(grads)


def l1_terms(terms, n_slots):
    """terms: [(x, y, mask or None, weight, slot)] or [(x, y, mask, [(x_row0, y_row0, rows, weight, slot), ...])] -> vector [n_slots]:
    out[slot] = sum of weight * F.l1_loss(x[rows] * mask, y[rows] * mask) over the terms / segments routed to that slot."""
    xs, meta = [], []
    for t in terms:
        if len(t) == 5:
            x, y, m, w, slot = t
            segments = [(0, 0, x.shape[0], float(w), int(slot))]
        else:
            x, y, m, segments = t
        xs.append(x)
        meta.append((y, m, segments))
    return _L1Terms.apply(n_slots, meta, *xs)
