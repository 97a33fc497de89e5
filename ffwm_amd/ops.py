"""Tensor-level entry points of the HIP hot path: torch tensors in, C ABI underneath.

PyTorch is plumbing here (device memory, the current HIP stream); every function below is one
call into libffwm_hip.so through ``include/ffwm_hip.h``.  CPU tensors are refused, as the
reference's wrappers refuse them (/root/reference/models/external_function.py:37-38,84-85):
there is no CPU or eager fallback in this package.
"""
import ctypes

import torch

from . import _lib

_DT = {torch.float32: _lib.F32, torch.float64: _lib.F64}


def _dtype_code(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError("ffwm_amd ops support float32/float64 (AT_DISPATCH_FLOATING_TYPES), got %s" % t.dtype)


def _go_strides(grad_output):
    """(ctypes int64[4] or None, keep-alive): the element strides of a grad_output that is not contiguous -- handed to the
    *_backward_strided entry points, which read it the way the reference's kernels do (DIM3_INDEX with the tensor's strides,
    cuda/block_extractor/block_extractor_kernel.cu:8-15; the reference's Functions drop the result of .contiguous(),
    models/external_function.py:46-47).  Views with a negative stride or a stride-0 last dimension are copied instead."""
    if grad_output.is_contiguous():
        return grad_output, None
    st = grad_output.stride()
    if any(x < 0 for x in st) or st[3] == 0:
        return grad_output.contiguous(), None
    return grad_output, (ctypes.c_int64 * 4)(*st)


def _check(name, *tensors, strided_ok=None):
    ref = tensors[0]
    for t in tensors:
        if t is None:
            continue
        if t is strided_ok:
            if not t.is_cuda or t.device != ref.device or t.dtype != ref.dtype or t.dim() != 4:
                raise ValueError("%s: grad_output must be a 4-D tensor of the operands' device and dtype" % name)
            continue
        if not t.is_cuda:
            raise NotImplementedError("%s: ffwm_amd ops run on the GPU only (got a %s tensor)" % (name, t.device))
        if t.device != ref.device:
            raise ValueError("%s: tensors live on different devices (%s vs %s)" % (name, t.device, ref.device))
        if t.dtype != ref.dtype:
            raise TypeError("%s: mixed dtypes (%s vs %s)" % (name, t.dtype, ref.dtype))
        if t.dim() != 4:
            raise ValueError("%s: expected 4-D NCHW tensors, got %d-D" % (name, t.dim()))
        if not t.is_contiguous():
            raise ValueError("%s: tensors must be contiguous NCHW" % name)


def _ptr(t):
    return None if t is None else t.data_ptr()


class _on_device(object):
    """Launch on the tensors' device and its current stream (the reference has no device guard)."""

    __slots__ = ("dev", "prev")

    def __init__(self, t):
        self.dev = t.device.index
        self.prev = None

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.dev:
            self.prev = cur
            torch.cuda.set_device(self.dev)
        return torch.cuda.current_stream(self.dev).cuda_stream

    def __exit__(self, *exc):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)
        return False


# ---------------------------------------------------------------- block_extractor
def block_extractor_forward(source, flow_field, kernel_size, out=None):
    """-> out[B,C,k*Hf,k*Wf]; reference block_extractor_kernel.cu:21-85."""
    _check("block_extractor_forward", source, flow_field, out)
    B, C, Hs, Ws = source.shape
    Bf, two, Hf, Wf = flow_field.shape
    if two != 2:
        raise ValueError("block_extractor_forward: flow_field must have 2 channels")
    if Bf < B:
        raise ValueError("block_extractor_forward: flow_field batch %d < source batch %d" % (Bf, B))
    k = int(kernel_size)
    if out is None:
        out = source.new_empty((B, C, k * Hf, k * Wf))
    elif tuple(out.shape) != (B, C, k * Hf, k * Wf):
        raise ValueError("block_extractor_forward: output has the wrong shape")
    if out.numel() == 0:
        return out
    with _on_device(source) as stream:
        _lib.check(_lib.load().ffwm_block_extractor_forward(
            _ptr(source), _ptr(flow_field), _ptr(out), B, C, Hs, Ws, Hf, Wf, k, _dtype_code(source), stream),
            "ffwm_block_extractor_forward")
    return out


def block_extractor_backward(source, flow_field, grad_output, kernel_size, grad_source=None,
                             grad_flow_field=None):
    """Accumulates (+=) into the given, zero-filled gradient buffers; None skips one."""
    grad_output, gst = _go_strides(grad_output)
    _check("block_extractor_backward", source, flow_field, grad_output, grad_source, grad_flow_field, strided_ok=grad_output if gst is not None else None)
    B, C, Hs, Ws = source.shape
    _, _, Hf, Wf = flow_field.shape
    k = int(kernel_size)
    if tuple(grad_output.shape) != (B, C, k * Hf, k * Wf):
        raise ValueError("block_extractor_backward: grad_output has the wrong shape")
    if grad_output.numel() == 0:
        return grad_source, grad_flow_field
    with _on_device(source) as stream:
        if gst is None:
            _lib.check(_lib.load().ffwm_block_extractor_backward(
                _ptr(source), _ptr(flow_field), _ptr(grad_output), _ptr(grad_source), _ptr(grad_flow_field),
                B, C, Hs, Ws, Hf, Wf, k, _dtype_code(source), stream), "ffwm_block_extractor_backward")
        else:              # a non-contiguous grad_output is read through its strides (no copy): the per-element kernel
            _lib.check(_lib.load().ffwm_block_extractor_backward_strided(
                _ptr(source), _ptr(flow_field), _ptr(grad_output), gst, _ptr(grad_source), _ptr(grad_flow_field),
                B, C, Hs, Ws, Hf, Wf, k, _dtype_code(source), stream), "ffwm_block_extractor_backward_strided")
    return grad_source, grad_flow_field


# ---------------------------------------------------------------- block attention (fused consumer)
def block_attention_forward(source, flow_field, weights, kernel_size, out=None):
    """out[B,C,Hf,Wf] = avg_pool2d(block_extractor(source, flow) * local_attn_reshape(weights), k) without the
    k^2-fold expanded tensors; weights[B,k*k,Hf,Wf]."""
    _check("block_attention_forward", source, flow_field, weights, out)
    B, C, Hs, Ws = source.shape
    Bf, two, Hf, Wf = flow_field.shape
    k = int(kernel_size)
    if two != 2 or Bf < B:
        raise ValueError("block_attention_forward: flow_field must be [>=B, 2, Hf, Wf]")
    if tuple(weights.shape) != (B, k * k, Hf, Wf):
        raise ValueError("block_attention_forward: weights must be [B, k*k, Hf, Wf], got %s" % (tuple(weights.shape),))
    if out is None:
        out = source.new_empty((B, C, Hf, Wf))
    elif tuple(out.shape) != (B, C, Hf, Wf):
        raise ValueError("block_attention_forward: output has the wrong shape")
    if out.numel() == 0:
        return out
    with _on_device(source) as stream:
        _lib.check(_lib.load().ffwm_block_attention_forward(
            _ptr(source), _ptr(flow_field), _ptr(weights), _ptr(out), B, C, Hs, Ws, Hf, Wf, k, _dtype_code(source),
            stream), "ffwm_block_attention_forward")
    return out


def block_attention_backward(source, flow_field, weights, grad_output, kernel_size, grad_source=None,
                             grad_flow_field=None, grad_weights=None):
    """Accumulates (+=) into the given, zero-filled gradient buffers; None skips one."""
    _check("block_attention_backward", source, flow_field, weights, grad_output, grad_source, grad_flow_field,
           grad_weights)
    B, C, Hs, Ws = source.shape
    _, _, Hf, Wf = flow_field.shape
    k = int(kernel_size)
    if tuple(grad_output.shape) != (B, C, Hf, Wf) or tuple(weights.shape) != (B, k * k, Hf, Wf):
        raise ValueError("block_attention_backward: grad_output / weights have the wrong shape")
    if grad_output.numel() == 0:
        return grad_source, grad_flow_field, grad_weights
    with _on_device(source) as stream:
        _lib.check(_lib.load().ffwm_block_attention_backward(
            _ptr(source), _ptr(flow_field), _ptr(weights), _ptr(grad_output), _ptr(grad_source),
            _ptr(grad_flow_field), _ptr(grad_weights), B, C, Hs, Ws, Hf, Wf, k, _dtype_code(source), stream),
            "ffwm_block_attention_backward")
    return grad_source, grad_flow_field, grad_weights


# ---------------------------------------------------------------- local_attn_reshape
def local_attn_reshape_forward(inputs, kernel_size, out=None):
    """-> out[B,1,k*H,k*W]; reference local_attn_reshape_kernel.cu:21-61."""
    _check("local_attn_reshape_forward", inputs, out)
    B, C, H, W = inputs.shape
    k = int(kernel_size)
    if C != k * k:
        raise ValueError("local_attn_reshape_forward: need C == k*k (C=%d, k=%d)" % (C, k))
    if out is None:
        out = inputs.new_empty((B, 1, k * H, k * W))
    elif tuple(out.shape) != (B, 1, k * H, k * W):
        raise ValueError("local_attn_reshape_forward: output has the wrong shape")
    if out.numel() == 0:
        return out
    with _on_device(inputs) as stream:
        _lib.check(_lib.load().ffwm_local_attn_reshape_forward(
            _ptr(inputs), _ptr(out), B, H, W, k, _dtype_code(inputs), stream),
            "ffwm_local_attn_reshape_forward")
    return out


def local_attn_reshape_backward(grad_output, kernel_size, grad_inputs=None, accumulate=False):
    """grad_inputs[B,k*k,H,W]; accumulate=True is the reference's += into a zero-filled buffer."""
    grad_output, gst = _go_strides(grad_output)
    _check("local_attn_reshape_backward", grad_inputs if grad_inputs is not None else grad_output, grad_output, grad_inputs,
           strided_ok=grad_output if gst is not None else None)
    B, one, Ho, Wo = grad_output.shape
    k = int(kernel_size)
    if one != 1 or Ho % k or Wo % k:
        raise ValueError("local_attn_reshape_backward: grad_output must be [B,1,k*H,k*W]")
    H, W = Ho // k, Wo // k
    if grad_inputs is None:
        if accumulate:
            raise ValueError("local_attn_reshape_backward: accumulate=True needs a grad_inputs buffer")
        grad_inputs = grad_output.new_empty((B, k * k, H, W))
    elif tuple(grad_inputs.shape) != (B, k * k, H, W):
        raise ValueError("local_attn_reshape_backward: grad_inputs has the wrong shape")
    if grad_output.numel() == 0:
        return grad_inputs
    with _on_device(grad_output) as stream:
        if gst is None:
            _lib.check(_lib.load().ffwm_local_attn_reshape_backward(
                _ptr(grad_output), _ptr(grad_inputs), B, H, W, k, 1 if accumulate else 0,
                _dtype_code(grad_output), stream), "ffwm_local_attn_reshape_backward")
        else:
            _lib.check(_lib.load().ffwm_local_attn_reshape_backward_strided(
                _ptr(grad_output), gst, _ptr(grad_inputs), B, H, W, k, 1 if accumulate else 0,
                _dtype_code(grad_output), stream), "ffwm_local_attn_reshape_backward_strided")
    return grad_inputs


# ---------------------------------------------------------------- resample2d
def resample2d_forward(input1, input2, kernel_size=2, dilation=1, out=None):
    """-> out[B,C,H,W]; reference resample2d_kernel.cu:21-95."""
    _check("resample2d_forward", input1, input2, out)
    B1, C, Hi, Wi = input1.shape
    B, three, H, W = input2.shape
    if three != 3:
        raise ValueError("resample2d_forward: input2 must be [B,3,H,W] = (dx, dy, sigma)")
    if B1 < B:
        raise ValueError("resample2d_forward: input1 batch %d < input2 batch %d" % (B1, B))
    if out is None:
        out = input1.new_empty((B, C, H, W))
    elif tuple(out.shape) != (B, C, H, W):
        raise ValueError("resample2d_forward: output has the wrong shape")
    if out.numel() == 0:
        return out
    with _on_device(input1) as stream:
        _lib.check(_lib.load().ffwm_resample2d_forward(
            _ptr(input1), _ptr(input2), _ptr(out), B, C, Hi, Wi, H, W, int(kernel_size), int(dilation),
            _dtype_code(input1), stream), "ffwm_resample2d_forward")
    return out


def resample2d_backward(input1, input2, grad_output, kernel_size=2, dilation=1, grad_input1=None,
                        grad_input2=None, reference_quirk=True, overwrite_input1=False):
    """grad_input1 += (zero-fill it first) -- or, with overwrite_input1, grad_input1[:B] = (the buffer may be uninitialised: the owned-tile
    kernel stores every cell once, any other path clears the buffer itself) --, grad_input2 is overwritten; None skips one."""
    grad_output, gst = _go_strides(grad_output)
    _check("resample2d_backward", input1, input2, grad_output, grad_input1, grad_input2, strided_ok=grad_output if gst is not None else None)
    _, C, Hi, Wi = input1.shape
    B, _, H, W = input2.shape
    if tuple(grad_output.shape) != (B, C, H, W):
        raise ValueError("resample2d_backward: grad_output has the wrong shape")
    if grad_output.numel() == 0:
        # nothing flows back, but what the caller handed over uninitialised must still come back as zeros: grad_input1[:B] in
        # overwrite mode, grad_input2 always (it is written, never accumulated into)
        if overwrite_input1 and grad_input1 is not None and B > 0 and grad_input1[:B].numel() > 0:
            zero_fill(grad_input1[:B])
        if grad_input2 is not None and grad_input2.numel() > 0:
            zero_fill(grad_input2)
        return grad_input1, grad_input2
    flags = (1 if reference_quirk else 0) | (2 if overwrite_input1 else 0)
    with _on_device(input1) as stream:
        if gst is None:
            _lib.check(_lib.load().ffwm_resample2d_backward(
                _ptr(input1), _ptr(input2), _ptr(grad_output), _ptr(grad_input1), _ptr(grad_input2), B, C, Hi,
                Wi, H, W, int(kernel_size), int(dilation), flags, _dtype_code(input1), stream), "ffwm_resample2d_backward")
        else:
            _lib.check(_lib.load().ffwm_resample2d_backward_strided(
                _ptr(input1), _ptr(input2), _ptr(grad_output), gst, _ptr(grad_input1), _ptr(grad_input2), B, C, Hi,
                Wi, H, W, int(kernel_size), int(dilation), flags, _dtype_code(input1), stream), "ffwm_resample2d_backward_strided")
    return grad_input1, grad_input2


# ---------------------------------------------------------------- warp (WarpNet)
def warp_forward(feat, flow, flipcat=False, out=None):
    """grid_sample(bilinear, zeros, align_corners=False) [+ flip + cat]; base_networks.py:168-173,326-329."""
    _check("warp_forward", feat, flow, out)
    B, C, Hi, Wi = feat.shape
    Bf, two, H, W = flow.shape
    if two != 2 or Bf != B:
        raise ValueError("warp_forward: flow must be [B,2,H,W] with the features' batch size")
    Co = 2 * C if flipcat else C
    if out is None:
        out = feat.new_empty((B, Co, H, W))
    elif tuple(out.shape) != (B, Co, H, W):
        raise ValueError("warp_forward: output has the wrong shape")
    if out.numel() == 0:
        return out
    with _on_device(feat) as stream:
        _lib.check(_lib.load().ffwm_warp_forward(
            _ptr(feat), _ptr(flow), _ptr(out), B, C, Hi, Wi, H, W, 1 if flipcat else 0, _dtype_code(feat),
            stream), "ffwm_warp_forward")
    return out


def warp_backward(feat, flow, grad_output, flipcat=False, grad_feat=None, grad_flow=None, overwrite_feat=False):
    """Both gradients accumulate (+=) into zero-filled buffers; None skips one.  overwrite_feat=True: grad_feat may be UNINITIALISED --
    the library produces it whole (the owned-tile kernel stores instead of adding and the zero-fill is saved; every other path zero-fills
    it itself: flipcat bit 1 of ffwm_warp_backward)."""
    _check("warp_backward", feat, flow, grad_output, grad_feat, grad_flow)
    B, C, Hi, Wi = feat.shape
    _, _, H, W = flow.shape
    if tuple(grad_output.shape) != (B, 2 * C if flipcat else C, H, W):
        raise ValueError("warp_backward: grad_output has the wrong shape")
    if grad_output.numel() == 0:
        if overwrite_feat and grad_feat is not None and grad_feat.numel() > 0:
            zero_fill(grad_feat)                # the caller's buffer may be uninitialised: nothing flows back, so it is zero
        return grad_feat, grad_flow
    with _on_device(feat) as stream:
        _lib.check(_lib.load().ffwm_warp_backward(
            _ptr(feat), _ptr(flow), _ptr(grad_output), _ptr(grad_feat), _ptr(grad_flow), B, C, Hi, Wi, H, W,
            (1 if flipcat else 0) | (2 if overwrite_feat and grad_feat is not None else 0), _dtype_code(feat), stream), "ffwm_warp_backward")
    return grad_feat, grad_flow


class _WarpProblem(ctypes.Structure):          # include/ffwm_hip.h: ffwm_warp_problem
    _fields_ = [("feat", ctypes.c_void_p), ("flow", ctypes.c_void_p), ("output", ctypes.c_void_p),
                ("grad_output", ctypes.c_void_p), ("grad_feat", ctypes.c_void_p), ("grad_flow", ctypes.c_void_p),
                ("B", ctypes.c_int64), ("C", ctypes.c_int64), ("Hi", ctypes.c_int64), ("Wi", ctypes.c_int64),
                ("H", ctypes.c_int64), ("W", ctypes.c_int64)]


def _warp_table(feats, flows, outs=None, grad_outputs=None, grad_feats=None, grad_flows=None):
    n = len(feats)
    arr = (_WarpProblem * n)()
    for i in range(n):
        B, C, Hi, Wi = feats[i].shape
        Bf, two, H, W = flows[i].shape
        if two != 2 or Bf != B:
            raise ValueError("warp_multi: flow %d must be [B,2,H,W] with the feature's batch" % i)
        a = arr[i]
        a.feat, a.flow = _ptr(feats[i]), _ptr(flows[i])
        a.output = _ptr(outs[i]) if outs is not None else None
        a.grad_output = _ptr(grad_outputs[i]) if grad_outputs is not None else None
        a.grad_feat = _ptr(grad_feats[i]) if grad_feats is not None and grad_feats[i] is not None else None
        a.grad_flow = _ptr(grad_flows[i]) if grad_flows is not None and grad_flows[i] is not None else None
        a.B, a.C, a.Hi, a.Wi, a.H, a.W = B, C, Hi, Wi, H, W
    return arr


def warp_multi_forward(feats, flows, flipcat=False):
    """Several independent warps (lists of equal length) in one or two launches; -> list of outputs."""
    _check("warp_multi_forward", *(list(feats) + list(flows)))
    outs = [f.new_empty((f.size(0), (2 if flipcat else 1) * f.size(1), fl.size(2), fl.size(3))) for f, fl in zip(feats, flows)]
    arr = _warp_table(feats, flows, outs=outs)
    with _on_device(feats[0]) as stream:
        _lib.check(_lib.load().ffwm_warp_multi_forward(ctypes.cast(arr, ctypes.c_void_p), len(feats), 1 if flipcat else 0,
                                                       _dtype_code(feats[0]), stream), "ffwm_warp_multi_forward")
    return outs


def warp_multi_backward(feats, flows, grad_outputs, flipcat, grad_feats, grad_flows):
    """grad_feats[i] / grad_flows[i]: zero-filled tensors to accumulate into, or None."""
    _check("warp_multi_backward", *(list(feats) + list(flows) + list(grad_outputs)))
    arr = _warp_table(feats, flows, grad_outputs=grad_outputs, grad_feats=grad_feats, grad_flows=grad_flows)
    with _on_device(feats[0]) as stream:
        _lib.check(_lib.load().ffwm_warp_multi_backward(ctypes.cast(arr, ctypes.c_void_p), len(feats), 1 if flipcat else 0,
                                                        _dtype_code(feats[0]), stream), "ffwm_warp_multi_backward")


# ---------------------------------------------------------------- guided filter
def _gf_shapes(name, x, y):
    """(B, Cx, Cy, H, W) of a guided-filter call; c_x == 1 or c_x == c_y as the reference asserts (external_function.py:246-249)."""
    if x.size(0) != y.size(0) or x.shape[2:] != y.shape[2:] or x.size(1) not in (1, y.size(1)):
        raise ValueError("%s: x and y must agree in N, H, W, with c_x == 1 or c_x == c_y, got %s vs %s"
                         % (name, tuple(x.shape), tuple(y.shape)))
    return x.size(0), x.size(1), y.size(1), x.size(2), x.size(3)


def _gf_workspace(x, B, Cx, Cy, H, W, backward):
    n = _lib.load().ffwm_guided_filter_workspace_bytes(B * Cx, B * Cy, H, W, _dtype_code(x), 1 if backward else 0)
    _lib.check(min(n, 0), "ffwm_guided_filter_workspace_bytes")
    return x.new_empty(n // x.element_size())


_GF_FAST = 128      # H, W up to here with c_x == c_y: the four-launch kernels, no workspace forward


def guided_filter_forward(x, y, r, eps=1e-8):
    """-> (out, saved); GuidedFilter(r, eps)(x, y), reference external_function.py:239-277: x [B, 1 or C, H, W], y [B, C, H, W].
    saved is [5, B, C, H, W] for c_x == c_y and a flat buffer (2 B + 3 B C planes) for a one-channel guide."""
    _check("guided_filter_forward", x, y)
    B, Cx, Cy, H, W = _gf_shapes("guided_filter_forward", x, y)
    out = torch.empty_like(y)
    saved = x.new_empty((5, B, Cy, H, W)) if Cx == Cy else x.new_empty(((2 * Cx + 3 * Cy) * B * H * W,))
    if out.numel() == 0:
        return out, saved
    with _on_device(x) as stream:
        if Cx == Cy and H <= _GF_FAST and W <= _GF_FAST:
            _lib.check(_lib.load().ffwm_guided_filter_forward(
                _ptr(x), _ptr(y), _ptr(out), _ptr(saved), B * Cy, H, W, int(r), float(eps), _dtype_code(x), stream),
                "ffwm_guided_filter_forward")
        else:
            ws = _gf_workspace(x, B, Cx, Cy, H, W, False)
            _lib.check(_lib.load().ffwm_guided_filter_forward_general(
                _ptr(x), _ptr(y), _ptr(out), _ptr(saved), _ptr(ws), B * Cx, B * Cy, H, W, int(r), float(eps), _dtype_code(x),
                stream), "ffwm_guided_filter_forward_general")
    return out, saved


def guided_filter_backward_xy(x, y, saved, grad_output, r, want_x=True, want_y=True):
    """-> (grad_x, grad_y), None for the one that is not wanted (it is neither computed nor written).  grad_x of a one-channel
    guide is the sum over y's channels."""
    _check("guided_filter_backward", x, y, grad_output)
    B, Cx, Cy, H, W = _gf_shapes("guided_filter_backward", x, y)
    if grad_output.shape != y.shape:
        raise ValueError("guided_filter_backward: grad_output must have y's shape")
    if saved.dtype != x.dtype or saved.device != x.device or saved.numel() != (2 * Cx + 3 * Cy) * B * H * W:
        raise ValueError("guided_filter_backward: saved is not what guided_filter_forward returned for these tensors")
    gx = torch.empty_like(x) if want_x else None
    gy = torch.empty_like(y) if want_y else None
    if y.numel() == 0 or not (want_x or want_y):
        return gx, gy
    with _on_device(x) as stream:
        if Cx == Cy and H <= _GF_FAST and W <= _GF_FAST and not want_y:
            ws = x.new_empty((2, B, Cy, H, W))
            _lib.check(_lib.load().ffwm_guided_filter_backward(
                _ptr(x), _ptr(y), _ptr(saved), _ptr(grad_output), _ptr(gx), _ptr(ws), B * Cy, H, W, int(r), _dtype_code(x), stream),
                "ffwm_guided_filter_backward")
        else:
            ws = _gf_workspace(x, B, Cx, Cy, H, W, True)
            _lib.check(_lib.load().ffwm_guided_filter_backward_general(
                _ptr(x), _ptr(y), _ptr(saved), _ptr(grad_output), _ptr(gx), _ptr(gy), _ptr(ws), B * Cx, B * Cy, H, W, int(r),
                _dtype_code(x), stream), "ffwm_guided_filter_backward_general")
    return gx, gy


def guided_filter_backward(x, y, saved, grad_output, r):
    """-> grad_x alone (guided_filter_backward_xy for grad_y)."""
    return guided_filter_backward_xy(x, y, saved, grad_output, r, True, False)[0]


# ---------------------------------------------------------------- fused affine regularisation
def affine_regularization(flow, ktk, kernel_size, want_grad=True):
    """-> (loss, grad_flow or None): AffineRegularizationLoss(kz)(flow) of the reference (losses.py:200-219)
    and its gradient, one launch.  ktk = the module's K^T K matrix [kz^2, kz^2] in flow's dtype."""
    if flow.dim() != 4 or flow.size(1) != 2:
        raise ValueError("affine_regularization: flow must be [B,2,h,w]")
    if not flow.is_cuda:
        raise NotImplementedError("affine_regularization: ffwm_amd ops run on the GPU only (got a %s tensor)" % flow.device)
    flow = flow.contiguous()
    ktk = ktk.to(device=flow.device, dtype=flow.dtype).contiguous()
    B, _, h, w = flow.shape
    k = int(kernel_size)
    if ktk.numel() != k ** 4:
        raise ValueError("affine_regularization: ktk must hold kz^2 x kz^2 values")
    loss = torch.zeros((), device=flow.device, dtype=flow.dtype)
    grad = torch.zeros_like(flow) if want_grad else None
    scale = 1.0 / (B * (h - k + 1) * (w - k + 1))
    with _on_device(flow) as stream:
        _lib.check(_lib.load().ffwm_affine_regularization(
            _ptr(flow), _ptr(ktk), _ptr(loss), _ptr(grad), B, h, w, k, scale, _dtype_code(flow), stream),
            "ffwm_affine_regularization")
    return loss * scale, grad


# ---------------------------------------------------------------- correlation column maximum (MFMA)
CORR_PRECISIONS = ("fp32", "bf16x3")


def check_corr_precision(precision, who="correlation_colmax"):
    if precision not in CORR_PRECISIONS:
        raise ValueError("%s: precision must be one of %s, got %r" % (who, ", ".join(CORR_PRECISIONS), precision))
    return precision


def correlation_colmax(source, target, precision="fp32"):
    """torch.bmm(source[B,N,C], target[B,C,N]).max(dim=1)[0] without the [B,N,N] matrix (losses.py:347-353).
    precision "fp32": the fp32 MFMA kernel; "bf16x3": the bf16 MFMA kernel on hi/lo-split operands, three MFMAs per k-block
    (csrc/correlation.hip: error (2^-16 + 3 C roundings) sum |s t|; an infinite operand counts as a NaN)."""
    check_corr_precision(precision)
    if source.dim() != 3 or target.dim() != 3 or source.size(0) != target.size(0) or source.size(1) != target.size(2) \
            or source.size(2) != target.size(1):
        raise ValueError("correlation_colmax: need source [B,N,C] and target [B,C,N]")
    if not source.is_cuda:
        raise NotImplementedError("correlation_colmax: ffwm_amd ops run on the GPU only (got a %s tensor)" % source.device)
    if source.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError("correlation_colmax: float32 only")
    source, target = source.contiguous(), target.contiguous()
    B, N, C = source.shape
    out = source.new_empty((B, N))
    with _on_device(source) as stream:
        entry = "ffwm_correlation_colmax_split" if precision == "bf16x3" else "ffwm_correlation_colmax"
        _lib.check(getattr(_lib.load(), entry)(_ptr(source), _ptr(target), _ptr(out), B, N, C, _lib.F32, stream), entry)
    return out


# ---------------------------------------------------------------- fused sampling-correctness loss
def sampling_correctness(source, target, flow, corr_max, mask, eps, want_grad, want_map=False):
    """-> (out[2], grad_flow or None, loss_map or None): PerceptualCorrectness.calculate_loss of the reference (losses.py:341-371,
    bilinear branch) after the correlation maximum, one pass (csrc/sampling_correctness.hip).  source [B,C,Hi,Wi], target [B,C,H,W],
    flow [B,2,H,W], corr_max [B,H W], mask [B,H W] or None.  out[0] is the loss, out[1] the denominator of its mean;
    grad_flow = mask d(loss_map)/d(flow), to be scaled by grad_output / out[1]."""
    name = "sampling_correctness"
    _check(name, source, target, flow)
    B, C, Hi, Wi = source.shape
    H, W = target.shape[2:]
    if target.shape[:2] != (B, C) or tuple(flow.shape) != (B, 2, H, W):
        raise ValueError("%s: need source [B,C,Hi,Wi], target [B,C,H,W] and flow [B,2,H,W], got %s, %s, %s"
                         % (name, tuple(source.shape), tuple(target.shape), tuple(flow.shape)))
    for t, what in ((corr_max, "corr_max"), (mask, "mask")):
        if t is None:
            continue
        if not t.is_cuda or t.device != source.device:
            raise ValueError("%s: %s must live on the operands' device" % (name, what))
        if t.dtype != source.dtype:
            raise TypeError("%s: mixed dtypes (%s vs %s)" % (name, t.dtype, source.dtype))
        if t.numel() != B * H * W or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous [B, H W] tensor" % (name, what))
    if corr_max is None:
        raise ValueError("%s: corr_max is required" % name)
    code = _dtype_code(source)
    from .losses import _exp_minus_one
    e1 = _exp_minus_one(source.dtype)
    out = source.new_empty(2)
    grad = torch.empty_like(flow) if want_grad else None
    loss_map = source.new_empty((B, H * W)) if want_map else None
    if B * H * W == 0 or C == 0:
        # nothing to launch: the value the composition gives an empty grid (the mean of nothing is NaN; an empty mask sums to 0)
        zero = source.new_zeros(())
        out[0] = float("nan") if mask is None else (zero - e1) / (zero + eps)
        out[1] = 0.0 if mask is None else eps
        if grad is not None:
            grad.zero_()
        return out, grad, loss_map
    n = _lib.load().ffwm_sampling_correctness_workspace_bytes(B, H, W, code)
    _lib.check(min(n, 0), "ffwm_sampling_correctness_workspace_bytes")
    ws = torch.empty(n // 8, dtype=torch.float64, device=source.device)
    with _on_device(source) as stream:
        _lib.check(_lib.load().ffwm_sampling_correctness(
            _ptr(source), _ptr(target), _ptr(flow), _ptr(corr_max), _ptr(mask), _ptr(loss_map), _ptr(grad), _ptr(out), _ptr(ws),
            B, C, Hi, Wi, H, W, e1, float(eps), code, stream), "ffwm_sampling_correctness")
    return out, grad, loss_map


# ---------------------------------------------------------------- fused landmark loss
def landmark_loss(flows, lm_S, lm_F, gate, divisors, weights, want_grad, out_grads=None):
    """-> (out[n + 1], grads, skipped): LandmarkLoss on n = 1 .. 4 flow scales of one batch in one call (csrc/landmark_loss.hip).
    flows[i] [B,2,s,s]; lm_S, lm_F int64 [B,L,2] in (x, y) order; gate [B,L,2] in the flows' dtype; divisors[i] >= 1 the integer the
    landmarks are floor-divided by on scale i; weights[i] its weight.  out[0] = sum_i weights[i] * mse_i, out[1 + i] = mse_i.
    want_grad: a bool, or one per scale; grads[i] = weights[i] * d(mse_i)/d(flows[i]) (None where not wanted), every element
    written (out_grads[i], where given, is the destination: contiguous, of the flow's shape; nobody needs to zero-fill it).
    skipped: a device int32 scalar, the landmarks with an lm_F component outside the plane of one scale or more; they add nothing
    to the loss or the gradient of that scale and are never dereferenced."""
    name = "landmark_loss"
    flows = list(flows)
    n = len(flows)
    if not 1 <= n <= 4 or len(divisors) != n or len(weights) != n:
        raise ValueError("%s: need 1 .. 4 flows with one divisor and one weight each" % name)
    wants = [bool(want_grad)] * n if isinstance(want_grad, (bool, int)) else [bool(w) for w in want_grad]
    if len(wants) != n:
        raise ValueError("%s: want_grad must be a bool or one per scale" % name)
    B = flows[0].shape[0] if flows[0].dim() == 4 else -1
    for f in flows:
        if f.dim() != 4 or f.shape[0] != B or f.shape[1] != 2 or f.shape[2] != f.shape[3]:
            raise ValueError("%s: every flow must be a square [B,2,s,s] of one batch size, got %s" % (name, tuple(f.shape)))
    if lm_S.dim() != 3 or lm_S.shape[0] != B or lm_S.shape[2] != 2 or lm_F.shape != lm_S.shape or gate.shape != lm_S.shape:
        raise ValueError("%s: lm_S, lm_F and gate must all be [B,L,2] with the flows' B, got %s, %s, %s"
                         % (name, tuple(lm_S.shape), tuple(lm_F.shape), tuple(gate.shape)))
    L = lm_S.shape[1]
    if B == 0 or L == 0 or any(f.shape[2] == 0 for f in flows):
        raise ValueError("%s: B, L and the sides must be positive (the mean of nothing)" % name)
    divisors = [int(q) for q in divisors]
    if any(q < 1 for q in divisors):
        raise ValueError("%s: divisors must be integers >= 1" % name)
    _check(name, *flows)
    for t, what in ((lm_S, "lm_S"), (lm_F, "lm_F"), (gate, "gate")):
        if not t.is_cuda:
            raise NotImplementedError("%s: ffwm_amd ops run on the GPU only (got a %s tensor)" % (name, t.device))
        if t.device != flows[0].device:
            raise ValueError("%s: %s must live on the flows' device" % (name, what))
    if lm_S.dtype != torch.int64 or lm_F.dtype != torch.int64:
        raise TypeError("%s: lm_S and lm_F must be int64 tensors" % name)
    if gate.dtype != flows[0].dtype:
        raise TypeError("%s: gate must have the flows' dtype (%s vs %s)" % (name, gate.dtype, flows[0].dtype))
    lm_S, lm_F, gate = lm_S.contiguous(), lm_F.contiguous(), gate.contiguous()
    code = _dtype_code(flows[0])
    grads = []
    for i, f in enumerate(flows):
        g = None
        if wants[i]:
            g = out_grads[i] if out_grads is not None and out_grads[i] is not None else torch.empty_like(f)
            if g.shape != f.shape or g.dtype != f.dtype or g.device != f.device or not g.is_contiguous():
                raise ValueError("%s: a gradient destination must be a contiguous tensor of its flow's shape, dtype and device" % name)
        grads.append(g)
    out = flows[0].new_empty(n + 1)
    skipped = torch.empty((), dtype=torch.int32, device=flows[0].device)
    lib = _lib.load()
    sides = (ctypes.c_int64 * n)(*[f.shape[2] for f in flows])
    nbytes = lib.ffwm_landmark_loss_workspace_bytes(sides, n, B, L, code)
    _lib.check(min(nbytes, 0), "ffwm_landmark_loss_workspace_bytes")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=flows[0].device)
    fl = (ctypes.c_void_p * n)(*[_ptr(f) for f in flows])
    gr = (ctypes.c_void_p * n)(*[_ptr(g) for g in grads])
    with _on_device(flows[0]) as stream:
        _lib.check(lib.ffwm_landmark_loss(fl, gr, sides, (ctypes.c_int64 * n)(*divisors), (ctypes.c_double * n)(*[float(w) for w in weights]),
                                          n, _ptr(lm_S), _ptr(lm_F), _ptr(gate), _ptr(out), _ptr(skipped), _ptr(ws), B, L, code, stream),
                   "ffwm_landmark_loss")
    return out, grads, skipped


# ---------------------------------------------------------------- classifier loss (csrc/softmax_xent.hip)
def softmax_xent_chunk():
    """Elements of a row that one block reduces (the shapes around it are where the kernel takes another path)."""
    return _lib.load().ffwm_softmax_xent_chunk()


def softmax_xent(logits, target, want_grad=True, out_grad=None):
    """-> (out[3], row_loss[B], rank[B] int32, grad or None, skipped): nn.CrossEntropyLoss (mean) over logits [B, N] with int64
    targets [B], and the reference's accuracy(output, target, (1, 5)), in one call.  out = (mean loss, prec@1, prec@5 in percent);
    row_loss[b] = logsumexp(x_b) - x_b[t_b]; rank[b] = the elements above the target's logit plus the equal ones in front of it;
    grad = d(mean loss)/d(logits), every element written (out_grad, where given, is the destination: contiguous, of the logits'
    shape, dtype and device).  skipped: a device int32 scalar, the rows with a target outside [0, N): loss 0, gradient row 0, rank N."""
    name = "softmax_xent"
    if not (torch.is_tensor(logits) and torch.is_tensor(target)) or logits.dim() != 2 or target.dim() != 1 \
            or target.shape[0] != logits.shape[0]:
        raise ValueError("%s: logits [B, N] and target [B] expected" % name)
    for t in (logits, target):
        if not t.is_cuda:
            raise NotImplementedError("%s: ffwm_amd ops run on the GPU only (got a %s tensor)" % (name, t.device))
    if target.device != logits.device:
        raise ValueError("%s: target must live on the logits' device" % name)
    if target.dtype != torch.int64:
        raise TypeError("%s: target must be an int64 tensor" % name)
    if not logits.is_contiguous():
        raise ValueError("%s: logits must be contiguous" % name)
    B, N = logits.shape
    if B == 0 or N == 0:
        raise ValueError("%s: B and N must be positive (the mean of nothing)" % name)
    code = _dtype_code(logits)
    target = target.contiguous()
    grad = None
    if want_grad:
        grad = out_grad if out_grad is not None else torch.empty_like(logits)
        if grad.shape != logits.shape or grad.dtype != logits.dtype or grad.device != logits.device or not grad.is_contiguous():
            raise ValueError("%s: the gradient destination must be a contiguous tensor of the logits' shape, dtype and device" % name)
    lib = _lib.load()
    nbytes = lib.ffwm_softmax_xent_workspace_bytes(B, N, code)
    _lib.check(min(nbytes, 0), "ffwm_softmax_xent_workspace_bytes")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=logits.device)
    out = logits.new_empty(3)
    row_loss = logits.new_empty(B)
    rank = torch.empty(B, dtype=torch.int32, device=logits.device)
    skipped = torch.empty((), dtype=torch.int32, device=logits.device)
    with _on_device(logits) as stream:
        _lib.check(lib.ffwm_softmax_xent(_ptr(logits), _ptr(target), _ptr(out), _ptr(row_loss), _ptr(rank), _ptr(grad), _ptr(skipped),
                                         _ptr(ws), B, N, code, stream), "ffwm_softmax_xent")
    return out, row_loss, rank, grad, skipped


# ---------------------------------------------------------------- gradient health (csrc/grad_health.hip)
GRAD_HEALTH_CHUNK = 8192           # FFWM_GRAD_HEALTH_CHUNK of include/ffwm_hip.h (tests/test_grad_health_cpu.py holds the two together)
GRAD_HEALTH_MAX_SEGMENTS = 16


def grad_health_workspace_doubles(n, n_seg):
    """The doubles ffwm_grad_health wants as workspace for n elements in n_seg segments."""
    return _lib.load().ffwm_grad_health_workspace_bytes(n, n_seg) // 8


def grad_health(flat, seg_end, record=None, workspace=None):
    """-> record [n_seg, 4] float64 on the device: per segment of the flat float32 gradient array, over its FINITE elements, sum g^2
    and max |g|, then the count of non-finite elements and the element count.  seg_end: an int64 DEVICE tensor of ascending ends in
    elements (a list is copied to the device), the last one flat.numel(), every other one a multiple of 4; at most 16.  record and
    workspace (float64, grad_health_workspace_doubles(n, n_seg) elements) are made when not given; only they are written.  Squares and
    sums in double, no atomics, the same bits on every call (csrc/grad_health.hip states the order of summation)."""
    name = "grad_health"
    if not torch.is_tensor(flat) or flat.dim() != 1:
        raise ValueError("%s: a flat 1-D tensor expected" % name)
    if not flat.is_cuda:
        raise NotImplementedError("%s: ffwm_amd ops run on the GPU only (got a %s tensor)" % (name, flat.device))
    if flat.dtype != torch.float32 or not flat.is_contiguous() or flat.numel() == 0:
        raise ValueError("%s: a contiguous float32 tensor with at least one element expected" % name)
    if not torch.is_tensor(seg_end):
        seg_end = torch.tensor(list(seg_end), dtype=torch.int64, device=flat.device)
    if seg_end.dtype != torch.int64 or seg_end.dim() != 1 or seg_end.device != flat.device or not seg_end.is_contiguous():
        raise ValueError("%s: seg_end must be a contiguous 1-D int64 tensor on the gradients' device" % name)
    n, n_seg = flat.numel(), seg_end.numel()
    if not 1 <= n_seg <= GRAD_HEALTH_MAX_SEGMENTS:
        raise ValueError("%s: 1 .. %d segments, got %d" % (name, GRAD_HEALTH_MAX_SEGMENTS, n_seg))
    if record is None:
        record = torch.empty(n_seg, 4, dtype=torch.float64, device=flat.device)
    if workspace is None:
        workspace = torch.empty(grad_health_workspace_doubles(n, n_seg), dtype=torch.float64, device=flat.device)
    for what, t, least in (("record", record, 4 * n_seg), ("workspace", workspace, 0)):
        if t.dtype != torch.float64 or t.device != flat.device or not t.is_contiguous() or t.numel() < least:
            raise ValueError("%s: %s must be a contiguous float64 tensor on the gradients' device%s"
                             % (name, what, " with 4 values per segment" if least else ""))
    with _on_device(flat) as stream:
        _lib.check(_lib.load().ffwm_grad_health(_ptr(flat), n, _ptr(seg_end), n_seg, _ptr(workspace), workspace.numel() * 8, _ptr(record),
                                                _lib.F32, stream), "ffwm_grad_health")
    return record


# ---------------------------------------------------------------- conv weight gradient (MFMA)
def conv3x3_wgrad_supported(input, grad_output):
    """Shapes the MFMA weight-gradient kernel takes: float32 NCHW, W a multiple of 64, below 4 GiB."""
    return (input.dtype == torch.float32 and grad_output.dtype == torch.float32 and input.is_cuda
            and input.shape[3] % 64 == 0 and input.numel() * 4 < (1 << 32) - 64 and grad_output.numel() * 4 < (1 << 32) - 64)


def conv3x3_wgrad(input, grad_output, grad_weight=None, grad_bias=None):
    """grad_weight[K,C,3,3] of a 3x3 / stride 1 / pad 1 convolution (+= when given, zero-filled otherwise); a given
    (zero-filled) grad_bias[K] receives the bias gradient from the same pass."""
    _check("conv3x3_wgrad", input, grad_output, grad_weight)
    if grad_bias is not None and not (grad_bias.is_cuda and grad_bias.device == input.device and grad_bias.dtype == input.dtype
                                      and grad_bias.is_contiguous()):
        raise ValueError("conv3x3_wgrad: grad_bias must be a contiguous tensor on the input's device, same dtype")
    B, C, H, W = input.shape
    Bg, K, Hg, Wg = grad_output.shape
    if (Bg, Hg, Wg) != (B, H, W):
        raise ValueError("conv3x3_wgrad: grad_output %s does not match input %s" % (tuple(grad_output.shape), tuple(input.shape)))
    if grad_weight is None:
        grad_weight = input.new_zeros((K, C, 3, 3))
    elif tuple(grad_weight.shape) != (K, C, 3, 3):
        raise ValueError("conv3x3_wgrad: grad_weight has the wrong shape")
    if grad_bias is not None and tuple(grad_bias.shape) != (K,):
        raise ValueError("conv3x3_wgrad: grad_bias has the wrong shape")
    with _on_device(input) as stream:
        _lib.check(_lib.load().ffwm_conv3x3_wgrad(_ptr(input), _ptr(grad_output), _ptr(grad_weight), _ptr(grad_bias), B, C, K,
                                                  H, W, _dtype_code(input), stream), "ffwm_conv3x3_wgrad")
    return grad_weight


def conv2d_wgrad(rows, gathered, kernel, stride, pad, grad_weight=None):
    """grad_weight[K, C, k, k] of Conv2d (rows = grad_output, gathered = input) or [Ci, Co, 4, 4] of ConvTranspose2d(4, 2, 1)
    (rows = input, gathered = grad_output) on csrc/conv_bwd.hip; += into `grad_weight` when given, else a fresh tensor."""
    _check("conv2d_wgrad", rows, gathered, grad_weight)
    B, K, Ho, Wo = rows.shape
    Bg, C, H, W = gathered.shape
    if Bg != B:
        raise ValueError("conv2d_wgrad: batch sizes differ")
    if grad_weight is None:
        grad_weight = rows.new_zeros((K, C, kernel, kernel))
    elif tuple(grad_weight.shape) != (K, C, kernel, kernel):
        raise ValueError("conv2d_wgrad: grad_weight has the wrong shape")
    with _on_device(rows) as stream:
        _lib.check(_lib.load().ffwm_conv2d_wgrad(_ptr(rows), _ptr(gathered), _ptr(grad_weight), B, K, Ho, Wo, C, H, W, int(kernel),
                                                 int(stride), int(pad), _dtype_code(rows), stream), "ffwm_conv2d_wgrad")
    return grad_weight


def zero_fill(t):
    """Clear a contiguous CUDA tensor with the library's own kernel (ffwm_zero_fill; never a memset node: DESIGN 5.1)."""
    if not (t.is_cuda and t.is_contiguous()):
        raise ValueError("zero_fill: a contiguous CUDA tensor")
    with _on_device(t) as stream:
        _lib.check(_lib.load().ffwm_zero_fill(_ptr(t), t.numel() * t.element_size(), stream), "ffwm_zero_fill")
    return t


def conv2d_wgrad_tiled_ok(rows):
    """Shapes the tiled weight-gradient kernel takes: a plane of a multiple of 4 pixels, 16-byte aligned float32 rows."""
    return (rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 4 and (rows.shape[2] * rows.shape[3]) % 4 == 0
            and rows.data_ptr() % 16 == 0 and rows.numel() < (1 << 29))


def conv2d_wgrad_tiled(rows, gathered, kernel, stride, pad, want_bias=False, zeroed=None):
    """-> (grad_weight, grad_bias or None) of Conv2d (rows = grad_output, gathered = input: [K, C, k, k]; grad_bias = the row sums)
    or grad_weight [Ci, Co, 4, 4] of ConvTranspose2d(4, 2, 1) (rows = input, gathered = grad_output; no bias) on the tiled kernel of
    csrc/conv_bwd.hip.  Both results are slices of ONE buffer: a fresh one (the library clears it with one fill launch when it has
    to), or `zeroed` -- K C k k (+ K) ZERO floats the caller owns (a slice of the trainer's gradient arena): no fill launch at all."""
    _check("conv2d_wgrad_tiled", rows, gathered)
    B, K, Ho, Wo = rows.shape
    Bg, C, H, W = gathered.shape
    if Bg != B:
        raise ValueError("conv2d_wgrad_tiled: batch sizes differ")
    n = K * C * kernel * kernel
    total = n + (K if want_bias else 0)
    if zeroed is not None:
        if not (zeroed.is_cuda and zeroed.device == rows.device and zeroed.dtype == rows.dtype and zeroed.is_contiguous() and zeroed.numel() == total):
            raise ValueError("conv2d_wgrad_tiled: `zeroed` must be %d contiguous zero elements of the operands' device and dtype" % total)
        buf = zeroed.view(-1)
    else:
        buf = rows.new_empty((total,))
    gw = buf[:n].view(K, C, kernel, kernel)
    gb = buf[n:] if want_bias else None
    lib = _lib.load()
    with _on_device(rows) as stream:
        # (`prezeroed` is an ARGUMENT since ABI 5: rounds 4-5 toggled a process-global library option around the call -- ADVICE r5)
        _lib.check(lib.ffwm_conv2d_wgrad_tiled(_ptr(rows), _ptr(gathered), _ptr(gw), _ptr(gb), B, K, Ho, Wo, C, H, W, int(kernel),
                                               int(stride), int(pad), 1 if zeroed is not None else 0, _dtype_code(rows), stream),
                   "ffwm_conv2d_wgrad_tiled")
    return gw, gb


def conv3x3_winograd(x, weight, bias=None, data_gradient=False, act=0, slope=0.0, out=None, frozen=None, pre=None):
    """Conv2d(C, K, 3, 1, 1) forward (weight [K, C, 3, 3]) or its data gradient (x = grad_output [B, K_layer, H, W], weight =
    the layer's own [K_layer, C_layer, 3, 3]; returns [B, C_layer, H, W]) by fp32 Winograd F(2x2, 3x3) on the MFMA units
    (csrc/conv_winograd.hip).  act = 1 applies LeakyReLU(slope) after the bias (slope 0 = ReLU).  frozen: a dict OWNED BY THE
    LAYER (it must die with the weight tensor) in which the transformed weights of a frozen layer are kept between calls,
    keyed by direction, layout and the weight's version counter."""
    _check("conv3x3_winograd", x, weight, out)
    if bias is not None and (not bias.is_cuda or bias.dtype != x.dtype or not bias.is_contiguous()):
        raise ValueError("conv3x3_winograd: bias must be a contiguous tensor of the input's device and dtype")
    B, C, H, W = x.shape
    if data_gradient:
        if weight.shape[0] != C or tuple(weight.shape[2:]) != (3, 3):
            raise ValueError("conv3x3_winograd: weight %s does not belong to a grad_output with %d channels" % (tuple(weight.shape), C))
        K = weight.shape[1]
    else:
        if weight.shape[1] != C or tuple(weight.shape[2:]) != (3, 3):
            raise ValueError("conv3x3_winograd: weight %s does not fit an input with %d channels" % (tuple(weight.shape), C))
        K = weight.shape[0]
    if bias is not None and tuple(bias.shape) != (K,):
        raise ValueError("conv3x3_winograd: bias must have %d elements" % K)
    if out is None:
        out = x.new_empty((B, K, H, W))
    elif tuple(out.shape) != (B, K, H, W):
        raise ValueError("conv3x3_winograd: out has the wrong shape")
    lib = _lib.load()
    _sync_winograd_split_mode()
    mode = int(bool(data_gradient))
    ws = None
    if pre is not None:
        # transformed weights prepared beforehand for exactly this weight tensor, direction and width class (a dict the producer of
        # the weights attached to them: conv3x3_winograd_weights_multi)
        ws = pre.get((mode, W % 4 == 0))
        if ws is not None:
            mode |= 2
            frozen = None
    if ws is None and frozen is not None and frozen is not False:
        key = (mode, W % 4 == 0, weight._version, weight.data_ptr())
        ws = frozen.get(key)
        if ws is not None:
            mode |= 2
        else:
            for k in [k for k in frozen if k[2:] != key[2:]]:
                del frozen[k]         # transforms of an older version of the weights
    if ws is None:
        ws = x.new_empty((lib.ffwm_conv3x3_winograd_workspace_bytes(K, C) // 4,))
        if frozen is not None and frozen is not False:
            frozen[key] = ws
    with _on_device(x) as stream:
        _lib.check(lib.ffwm_conv3x3_winograd_forward(_ptr(x), _ptr(weight), _ptr(bias) if bias is not None else None, _ptr(out), _ptr(ws),
                                                     B, C, H, W, K, mode, int(act), float(slope), _dtype_code(x),
                                                     stream), "ffwm_conv3x3_winograd_forward")
    if frozen is not None and frozen is not False and not (mode & 2):
        # a transform that was just written into a layer's cache may be picked up by a call on ANOTHER stream (the trainer runs the
        # loss networks' passes on side streams): make it visible to every stream, once per frozen layer
        torch.cuda.current_stream(x.device).synchronize()
    return out


class _WinoWeightsItem(ctypes.Structure):
    _fields_ = [("weight", ctypes.c_void_p), ("workspace", ctypes.c_void_p), ("K", ctypes.c_int64), ("C", ctypes.c_int64),
                ("data_gradient", ctypes.c_int), ("width_multiple_of_4", ctypes.c_int)]


def conv3x3_winograd_weights_multi(items):
    """items: [(weight [Kl, Cl, 3, 3], data_gradient, width_multiple_of_4), ...] -> the transformed weights of every item (one
    tensor each, what conv3x3_winograd(..., pre=...) takes), all from ONE launch per 24 items (ffwm_conv3x3_winograd_weights_multi)."""
    if not items:
        return []
    lib = _lib.load()
    w0 = items[0][0]
    arr = (_WinoWeightsItem * len(items))()
    out = []
    for a, (w, dg, wm4) in zip(arr, items):
        if not (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 4 and tuple(w.shape[2:]) == (3, 3) and w.device == w0.device):
            raise ValueError("conv3x3_winograd_weights_multi: contiguous float32 [K, C, 3, 3] weights on one GPU")
        K, C = (w.shape[1], w.shape[0]) if dg else (w.shape[0], w.shape[1])
        ws = w.new_empty((lib.ffwm_conv3x3_winograd_workspace_bytes(K, C) // 4,))
        a.weight, a.workspace, a.K, a.C, a.data_gradient, a.width_multiple_of_4 = w.data_ptr(), ws.data_ptr(), K, C, int(bool(dg)), int(bool(wm4))
        out.append(ws)
    with _on_device(w0) as stream:
        _lib.check(lib.ffwm_conv3x3_winograd_weights_multi(ctypes.cast(arr, ctypes.c_void_p), len(items), _lib.F32, stream),
                   "ffwm_conv3x3_winograd_weights_multi")
    return out


_WINO_SPLIT_CAPPED = False
_WINO_SPLIT_BEFORE_CAP = 1


def _sync_winograd_split_mode():
    """torch.use_deterministic_algorithms(True) caps the Winograd kernel's reduction split at TWO pieces: two partial sums meet in a
    zero-filled output by float atomics, and a two-term sum does not depend on the order -- four terms do.  The library
    option conv_wino_split (1 = up to four pieces, the default; 2 = capped; 0 = never split) is RAISED to the cap while the switch is on
    and put back to what it was when it goes off; with the switch off a value set by hand is never touched (the first call
    used to overwrite a hand-set 2 with 1).  A hipGraph captured before the switch changed keeps the split it was captured with:
    re-capture (FFWMTrainer.release_graphs()) after changing the switch."""
    global _WINO_SPLIT_CAPPED, _WINO_SPLIT_BEFORE_CAP
    want = bool(torch.are_deterministic_algorithms_enabled())
    if want == _WINO_SPLIT_CAPPED:
        return
    if want:
        prev = _lib.set_option("conv_wino_split", 2)
        _WINO_SPLIT_BEFORE_CAP = prev
        if prev == 0:
            _lib.set_option("conv_wino_split", 0)          # never split: already deterministic
    else:
        _lib.set_option("conv_wino_split", _WINO_SPLIT_BEFORE_CAP)
    _WINO_SPLIT_CAPPED = want


def conv3x3_winograd_splits(B, C, H, W, K, act=0):
    """In how many pieces conv3x3_winograd will cut the reduction of this call (1, 2 or 4): ffwm_conv3x3_winograd_splits."""
    _sync_winograd_split_mode()
    return int(_lib.load().ffwm_conv3x3_winograd_splits(int(B), int(C), int(H), int(W), int(K), int(act)))


# ---------------------------------------------------------------- Winograd as 16 batched GEMMs (csrc/conv_winograd_gemm.hip)
WG_EPILOGUES = {"none": 0, "bias": 1, "relu": 2, "mfm": 3}


def conv3x3_wg_weights(weight, data_gradient=False):
    """U = G w G^T of a FROZEN Conv2d(C, K, 3, 1, 1) weight [K, C, 3, 3] for conv3x3_wg: the forward's, or (data_gradient) the
    data gradient's (the weight transposed and rotated).  One launch; made once per layer and direction."""
    if not (weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous() and weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3)):
        raise ValueError("conv3x3_wg_weights: a contiguous float32 [K, C, 3, 3] weight on the GPU")
    K, C = (weight.shape[1], weight.shape[0]) if data_gradient else (weight.shape[0], weight.shape[1])
    lib = _lib.load()
    U = weight.new_empty((lib.ffwm_conv3x3_wg_weights_bytes(K, C) // 4,))
    with _on_device(weight) as stream:
        _lib.check(lib.ffwm_conv3x3_wg_weights(_ptr(weight), _ptr(U), K, C, int(bool(data_gradient)), _lib.F32, stream), "ffwm_conv3x3_wg_weights")
    return U


def conv3x3_wg(x, U, bias, epilogue, relu_mask=None, out=None, K=None, tile=0):
    """Conv2d(C, K, 3, 1, 1) of x [B, C, H, W] with the transformed weights U of conv3x3_wg_weights, as input transform, 16 MFMA
    GEMMs and output transform.  epilogue: "none", "bias", "relu" (bias + ReLU) or "mfm" (bias + max-feature-map: [B, K / 2, H, W]).
    relu_mask: a tensor of x's shape; x is read as aten::threshold_backward(x, relu_mask, 0) (the data gradient behind a ReLU).
    K: the output channels before the epilogue (default: bias.numel()).  tile (tests): 64 / 128 fixes the GEMM tile."""
    _check("conv3x3_wg", x, relu_mask, out)
    for t in (U, bias):
        if t is not None and (t.device != x.device or t.dtype != x.dtype or not t.is_contiguous()):
            raise ValueError("conv3x3_wg: U and bias must be contiguous tensors of the input's device and dtype")
    if x.dtype != torch.float32:
        raise TypeError("conv3x3_wg: float32 only")
    B, C, H, W = x.shape
    if K is None:
        if bias is None:
            raise ValueError("conv3x3_wg: K is needed when there is no bias")
        K = bias.numel()
    lib = _lib.load()
    if U.numel() * 4 != lib.ffwm_conv3x3_wg_weights_bytes(K, C):
        raise ValueError("conv3x3_wg: U does not belong to a layer with %d input and %d output channels" % (C, K))
    if bias is not None and (not bias.is_contiguous() or bias.numel() != K):
        raise ValueError("conv3x3_wg: bias must be a contiguous vector of %d elements" % K)
    if relu_mask is not None and (relu_mask.shape != x.shape or not relu_mask.is_contiguous()):
        raise ValueError("conv3x3_wg: relu_mask must be contiguous and of x's shape")
    epi = WG_EPILOGUES[epilogue]
    if epi == 3 and K % 2:
        raise ValueError("conv3x3_wg: the mfm epilogue needs an even K")
    shape = (B, K // 2 if epi == 3 else K, H, W)
    if out is None:
        out = x.new_empty(shape)
    elif tuple(out.shape) != shape:
        raise ValueError("conv3x3_wg: out has the wrong shape")
    ws = x.new_empty((lib.ffwm_conv3x3_wg_workspace_bytes(B, C, H, W, K) // 4,))
    with _on_device(x) as stream:
        _lib.check(lib.ffwm_conv3x3_wg_forward_tiled(_ptr(x), _ptr(U), _ptr(bias), _ptr(out), _ptr(ws), B, C, H, W, K, epi,
                                                     _ptr(relu_mask), int(tile), _dtype_code(x), stream), "ffwm_conv3x3_wg_forward")
    return out


def conv3x3_wg_tile(B, C, H, W, K):
    """The GEMM tile (64 or 128) the plan of conv3x3_wg takes for this call on the current device: ffwm_conv3x3_wg_tile."""
    return int(_lib.load().ffwm_conv3x3_wg_tile(int(B), int(C), int(H), int(W), int(K)))


# ---------------------------------------------------------------- the same route on the bf16 MFMA (csrc/conv_winograd_gemm_split.hip)
WG_SPLIT_EPILOGUES = {"none": 0, "bias": 1, "lrelu": 2}


def conv3x3_wg_split_weights(weight, data_gradient=False):
    """U = G w G^T of a FROZEN Conv2d(C, K, 3, 1, 1) weight [K, C, 3, 3], every entry split in two bf16 terms, for conv3x3_wg_split /
    conv3x3_wg_split_frozen: the forward's, or (data_gradient) the data gradient's -- the weight read transposed and rotated, bit for
    bit the forward's U of weight.transpose(0, 1).flip(2, 3).  One launch; made once per layer and direction.  A float32 tensor that
    holds the bf16 halves (ffwm_conv3x3_wg_split_weights_bytes)."""
    if not (weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous() and weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3)):
        raise ValueError("conv3x3_wg_split_weights: a contiguous float32 [K, C, 3, 3] weight on the GPU")
    K, C = weight.shape[0], weight.shape[1]
    lib = _lib.load()
    if data_gradient:
        U = weight.new_empty((lib.ffwm_conv3x3_wg_split_weights_bytes(C, K) // 4,))
        with _on_device(weight) as stream:
            _lib.check(lib.ffwm_conv3x3_wg_split_weights_dgrad(_ptr(weight), _ptr(U), K, C, _lib.F32, stream),
                       "ffwm_conv3x3_wg_split_weights_dgrad")
        return U
    U = weight.new_empty((lib.ffwm_conv3x3_wg_split_weights_bytes(K, C) // 4,))
    with _on_device(weight) as stream:
        _lib.check(lib.ffwm_conv3x3_wg_split_weights(_ptr(weight), _ptr(U), K, C, _lib.F32, stream), "ffwm_conv3x3_wg_split_weights")
    return U


def conv3x3_wg_split(x, U, bias, epilogue, slope=0.2, out=None, K=None, tile=0, workspace=None):
    """Conv2d(C, K, 3, 1, 1) of float32 x [B, C, H, W] with the split transformed weights U of conv3x3_wg_split_weights: input
    transform + split, 16 GEMMs on the bf16 MFMA (lo hi + hi lo + hi hi per product), output transform.  epilogue: "none", "bias" or
    "lrelu" (bias + LeakyReLU(slope)).  K: the output channels (default: bias.numel()).  tile (tests): 64 / 128 fixes the GEMM tile.
    workspace: a float32 tensor of at least ffwm_conv3x3_wg_split_workspace_bytes (an arena slice), else allocated.  Error bound and
    the non-finite contract: include/ffwm_hip.h."""
    _check("conv3x3_wg_split", x, out)
    for t in (U, bias, workspace):
        if t is not None and (t.device != x.device or t.dtype != x.dtype or not t.is_contiguous()):
            raise ValueError("conv3x3_wg_split: U, bias and workspace must be contiguous tensors of the input's device and dtype")
    if x.dtype != torch.float32:
        raise TypeError("conv3x3_wg_split: float32 only")
    B, C, H, W = x.shape
    if K is None:
        if bias is None:
            raise ValueError("conv3x3_wg_split: K is needed when there is no bias")
        K = bias.numel()
    lib = _lib.load()
    if U.numel() * 4 != lib.ffwm_conv3x3_wg_split_weights_bytes(K, C):
        raise ValueError("conv3x3_wg_split: U does not belong to a layer with %d input and %d output channels" % (C, K))
    epi = WG_SPLIT_EPILOGUES[epilogue]
    if epi and bias is None:
        raise ValueError("conv3x3_wg_split: the %s epilogue needs a bias" % epilogue)
    if bias is not None and bias.numel() != K:
        raise ValueError("conv3x3_wg_split: bias must be a contiguous vector of %d elements" % K)
    shape = (B, K, H, W)
    if out is None:
        out = x.new_empty(shape)
    elif tuple(out.shape) != shape:
        raise ValueError("conv3x3_wg_split: out has the wrong shape")
    need = lib.ffwm_conv3x3_wg_split_workspace_bytes(B, C, H, W, K) // 4
    if workspace is None:
        workspace = x.new_empty((need,))
    elif workspace.numel() < need:
        raise ValueError("conv3x3_wg_split: the workspace is too small")
    with _on_device(x) as stream:
        _lib.check(lib.ffwm_conv3x3_wg_split_forward(_ptr(x), _ptr(U), _ptr(bias), _ptr(out), _ptr(workspace), B, C, H, W, K, epi,
                                                     float(slope), int(tile), _dtype_code(x), stream), "ffwm_conv3x3_wg_split_forward")
    return out


def conv3x3_wg_split_frozen(x, U, bias, epilogue, relu_mask=None, out=None, K=None, tile=0, workspace=None):
    """conv3x3_wg_split for the frozen loss networks of the train step, with the epilogue names of conv3x3_wg: "none", "bias", "relu"
    (bias + ReLU) or "mfm" (bias + max-feature-map: [B, K / 2, H, W]).  relu_mask: a tensor of x's shape; x is read as
    aten::threshold_backward(x, relu_mask, 0) (the data gradient behind a ReLU; U of conv3x3_wg_split_weights(w, data_gradient=True)).
    K: the output channels before the epilogue (default: bias.numel()).  tile (tests): 64 / 128 fixes the GEMM tile.  workspace: a
    float32 tensor of at least ffwm_conv3x3_wg_split_workspace_bytes, else allocated."""
    _check("conv3x3_wg_split_frozen", x, relu_mask, out)
    for t in (U, bias, workspace):
        if t is not None and (t.device != x.device or t.dtype != x.dtype or not t.is_contiguous()):
            raise ValueError("conv3x3_wg_split_frozen: U, bias and workspace must be contiguous tensors of the input's device and dtype")
    if x.dtype != torch.float32:
        raise TypeError("conv3x3_wg_split_frozen: float32 only")
    B, C, H, W = x.shape
    if K is None:
        if bias is None:
            raise ValueError("conv3x3_wg_split_frozen: K is needed when there is no bias")
        K = bias.numel()
    lib = _lib.load()
    if U.numel() * 4 != lib.ffwm_conv3x3_wg_split_weights_bytes(K, C):
        raise ValueError("conv3x3_wg_split_frozen: U does not belong to a layer with %d input and %d output channels" % (C, K))
    epi = WG_EPILOGUES[epilogue]
    if epi and bias is None:
        raise ValueError("conv3x3_wg_split_frozen: the %s epilogue needs a bias" % epilogue)
    if bias is not None and bias.numel() != K:
        raise ValueError("conv3x3_wg_split_frozen: bias must be a contiguous vector of %d elements" % K)
    if relu_mask is not None and (relu_mask.shape != x.shape or not relu_mask.is_contiguous()):
        raise ValueError("conv3x3_wg_split_frozen: relu_mask must be contiguous and of x's shape")
    if epi == 3 and K % 2:
        raise ValueError("conv3x3_wg_split_frozen: the mfm epilogue needs an even K")
    shape = (B, K // 2 if epi == 3 else K, H, W)
    if out is None:
        out = x.new_empty(shape)
    elif tuple(out.shape) != shape:
        raise ValueError("conv3x3_wg_split_frozen: out has the wrong shape")
    need = lib.ffwm_conv3x3_wg_split_workspace_bytes(B, C, H, W, K) // 4
    if workspace is None:
        workspace = x.new_empty((need,))
    elif workspace.numel() < need:
        raise ValueError("conv3x3_wg_split_frozen: the workspace is too small")
    with _on_device(x) as stream:
        _lib.check(lib.ffwm_conv3x3_wg_split_apply(_ptr(x), _ptr(U), _ptr(bias), _ptr(out), _ptr(workspace), B, C, H, W, K, epi,
                                                   _ptr(relu_mask), int(tile), _dtype_code(x), stream), "ffwm_conv3x3_wg_split_apply")
    return out


def conv3x3_wg_split_tile(B, C, H, W, K):
    """The GEMM tile (64 or 128) the plan of conv3x3_wg_split takes for this call on the current device."""
    return int(_lib.load().ffwm_conv3x3_wg_split_tile(int(B), int(C), int(H), int(W), int(K)))


def conv3x3_wg_split_workspace_floats(B, C, H, W, K):
    """The workspace of conv3x3_wg_split in float32 elements (ffwm_conv3x3_wg_split_workspace_bytes / 4); no device is touched."""
    return int(_lib.load().ffwm_conv3x3_wg_split_workspace_bytes(int(B), int(C), int(H), int(W), int(K))) // 4


# ---------------------------------------------------------------- LightCNN max-feature-map
def _mfm_dims(x):
    if x.dim() < 2 or x.shape[1] % 2:
        raise ValueError("mfm: need [B, 2C, ...], got %s" % (tuple(x.shape),))
    hw = 1
    for d in x.shape[2:]:
        hw *= d
    return x.shape[0], x.shape[1] // 2, hw


def _bias_ok(x, bias, n):
    if bias is None:
        return
    if not (bias.is_cuda and bias.dtype == x.dtype and bias.is_contiguous() and bias.numel() == n):
        raise ValueError("bias must be a contiguous float32 GPU vector of %d elements" % n)


# ---------------------------------------------------------------- residual-block tails / warp-attention gate
_ACT_CODES = {"lrelu": 1, "sigmoid": 3}


def _same_f32(name, *ts):
    t0 = ts[0]
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == t0.shape and t.device == t0.device):
            raise NotImplementedError("%s: contiguous float32 GPU tensors of one shape only" % name)


def add_act_forward(a, b, act, negative_slope=0.2):
    """act(a + b): the tail of ResidualBlock.forward (base_networks.py:207-233) as one pass; act in {"lrelu", "sigmoid"}."""
    _same_f32("add_act_forward", a, b)
    y = torch.empty_like(a)
    if y.numel():
        with _on_device(a) as stream:
            _lib.check(_lib.load().ffwm_add_act_forward(_ptr(a), _ptr(b), _ptr(y), a.numel(), _ACT_CODES[act], float(negative_slope),
                                                        _lib.F32, stream), "ffwm_add_act_forward")
    return y


def add_act_backward(y, grad_y, act, negative_slope=0.2):
    """grad_y * act'(a + b) from y = act(a + b): the gradient of a and of b."""
    _same_f32("add_act_backward", y, grad_y)
    dz = torch.empty_like(y)
    if dz.numel():
        with _on_device(y) as stream:
            _lib.check(_lib.load().ffwm_add_act_backward(_ptr(y), _ptr(grad_y), _ptr(dz), y.numel(), _ACT_CODES[act],
                                                         float(negative_slope), _lib.F32, stream), "ffwm_add_act_backward")
    return dz


def sigmoid_gate_forward(a, b, x):
    """-> (y, att): att = sigmoid(a + b), y = x * att (FFWM.forward's `skip * att_i(skip)`, base_networks.py:330-333)."""
    _same_f32("sigmoid_gate_forward", a, b, x)
    att, y = torch.empty_like(a), torch.empty_like(a)
    if y.numel():
        with _on_device(a) as stream:
            _lib.check(_lib.load().ffwm_sigmoid_gate_forward(_ptr(a), _ptr(b), _ptr(x), _ptr(att), _ptr(y), a.numel(), _lib.F32, stream),
                       "ffwm_sigmoid_gate_forward")
    return y, att


def sigmoid_gate_backward(x, att, grad_y):
    """-> (grad_z, grad_x): grad_z = the gradient of a and of b."""
    _same_f32("sigmoid_gate_backward", x, att, grad_y)
    dz, dx = torch.empty_like(x), torch.empty_like(x)
    if dz.numel():
        with _on_device(x) as stream:
            _lib.check(_lib.load().ffwm_sigmoid_gate_backward(_ptr(x), _ptr(att), _ptr(grad_y), _ptr(dz), _ptr(dx), x.numel(), _lib.F32,
                                                              stream), "ffwm_sigmoid_gate_backward")
    return dz, dx


# ---------------------------------------------------------------- netG eval forward (csrc/netg_eval.hip)
def _f32_in(name, *ts):
    t0 = ts[0]
    for t in ts:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == t0.device):
            raise NotImplementedError("%s: contiguous float32 tensors on one GPU only" % name)


def _dest_view(name, out, shape, like):
    """out: None (a fresh contiguous tensor) or a destination view -- [B, C, H, W] of `shape` whose samples are contiguous (a
    channel slice of a concatenation buffer); -> (tensor, batch stride)."""
    if out is None:
        out = like.new_empty(shape)
    B, C, H, W = shape
    if not (out.is_cuda and out.dtype == torch.float32 and out.device == like.device and tuple(out.shape) == tuple(shape)
            and out.stride(3) == 1 and out.stride(2) == W and out.stride(1) == H * W and out.stride(0) >= C * H * W):
        raise ValueError("%s: the destination must be a float32 [%d, %d, %d, %d] view with contiguous samples" % ((name,) + tuple(shape)))
    return out, out.stride(0)


def shuffle_bias_act(h, bias, slope=0.2, out=None):
    """lrelu(pixel_shuffle(h, 2) + bias[k]) of h [B, 4K, H, W] (base_networks.py:261-272 with the BatchNorm folded) in one pass,
    into `out` (a destination view [B, K, 2H, 2W]) or a fresh tensor."""
    _f32_in("shuffle_bias_act", h, bias)
    B, C4, H, W = h.shape
    if C4 % 4 or (bias is not None and bias.numel() != C4 // 4):
        raise ValueError("shuffle_bias_act: h must have 4K channels and bias K elements")
    K = C4 // 4
    out, obs = _dest_view("shuffle_bias_act", out, (B, K, 2 * H, 2 * W), h)
    with _on_device(h) as stream:
        _lib.check(_lib.load().ffwm_shuffle_bias_act_forward(_ptr(h), _ptr(bias), _ptr(out), B, K, H, W, obs, float(slope), _lib.F32, stream),
                   "ffwm_shuffle_bias_act_forward")
    return out


def image_head(x, weight, bias, out=None):
    """sigmoid(conv2d(x, weight [3, C, 3, 3], bias, stride 1, padding 1)): netG's rec0 / rec1 / rec2 as one direct kernel."""
    _f32_in("image_head", x, weight, bias)
    B, C, H, W = x.shape
    if tuple(weight.shape) != (3, C, 3, 3) or (bias is not None and bias.numel() != 3):
        raise ValueError("image_head: weight [3, %d, 3, 3] and bias [3] expected" % C)
    out, obs = _dest_view("image_head", out, (B, 3, H, W), x)
    with _on_device(x) as stream:
        _lib.check(_lib.load().ffwm_image_head_forward(_ptr(x), _ptr(weight), _ptr(bias), _ptr(out), B, C, H, W, obs, _lib.F32, stream),
                   "ffwm_image_head_forward")
    return out


def upsample2x_bilinear(x, out=None):
    """F.interpolate(x, scale_factor=2, mode="bilinear") (align_corners=False) into `out` (a destination view) or a fresh tensor."""
    _f32_in("upsample2x_bilinear", x)
    B, C, H, W = x.shape
    out, obs = _dest_view("upsample2x_bilinear", out, (B, C, 2 * H, 2 * W), x)
    with _on_device(x) as stream:
        _lib.check(_lib.load().ffwm_upsample2x_bilinear_forward(_ptr(x), _ptr(out), B, C, H, W, obs, _lib.F32, stream),
                   "ffwm_upsample2x_bilinear_forward")
    return out


def sigmoid_gate_forward_strided(a, b, x, out=None, want_att=True):
    """-> (y, att or None): sigmoid_gate_forward with y written into `out` (a destination view); want_att=False skips att."""
    _same_f32("sigmoid_gate_forward_strided", a, b, x)
    if a.dim() != 4:
        raise ValueError("sigmoid_gate_forward_strided: 4-D tensors expected")
    B, C, H, W = a.shape
    out, obs = _dest_view("sigmoid_gate_forward_strided", out, (B, C, H, W), a)
    att = torch.empty_like(a) if want_att else None
    with _on_device(a) as stream:
        _lib.check(_lib.load().ffwm_sigmoid_gate_forward_strided(_ptr(a), _ptr(b), _ptr(x), _ptr(att), _ptr(out), B, C, H * W, obs, _lib.F32,
                                                                 stream), "ffwm_sigmoid_gate_forward_strided")
    return out, att


def mfm_forward(x, bias=None):
    """max(x[:, :C] + bias[:C], x[:, C:] + bias[C:]) of a contiguous float32 [B, 2C, ...] tensor."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
        raise NotImplementedError("mfm_forward: contiguous float32 GPU tensors only")
    B, C, HW = _mfm_dims(x)
    _bias_ok(x, bias, 2 * C)
    y = x.new_empty((B, C) + tuple(x.shape[2:]))
    if y.numel():
        with _on_device(x) as stream:
            _lib.check(_lib.load().ffwm_mfm_forward(_ptr(x), _ptr(bias), _ptr(y), B, C, HW, _lib.F32, stream), "ffwm_mfm_forward")
    return y


def mfm_backward(x, grad_y, bias=None):
    if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and grad_y.is_contiguous() and grad_y.dtype == x.dtype):
        raise NotImplementedError("mfm_backward: contiguous float32 GPU tensors only")
    B, C, HW = _mfm_dims(x)
    _bias_ok(x, bias, 2 * C)
    dx = torch.empty_like(x)
    if dx.numel():
        with _on_device(x) as stream:
            _lib.check(_lib.load().ffwm_mfm_backward(_ptr(x), _ptr(bias), _ptr(grad_y), _ptr(dx), B, C, HW, _lib.F32, stream),
                       "ffwm_mfm_backward")
    return dx


def bias_relu_forward(h, bias, out=None):
    """relu(h + bias[None, :, None, None]) of a contiguous float32 [B, C, ...] tensor; out may be h itself."""
    if not (h.is_cuda and h.dtype == torch.float32 and h.is_contiguous()):
        raise NotImplementedError("bias_relu_forward: contiguous float32 GPU tensors only")
    B, C = h.shape[0], h.shape[1]
    HW = h.numel() // max(B * C, 1)
    _bias_ok(h, bias, C)
    y = torch.empty_like(h) if out is None else out
    if y.numel():
        with _on_device(h) as stream:
            _lib.check(_lib.load().ffwm_bias_relu_forward(_ptr(h), _ptr(bias), _ptr(y), B, C, HW, _lib.F32, stream),
                       "ffwm_bias_relu_forward")
    return y


# ---------------------------------------------------------------- identity evaluation (csrc/lightcnn_eval.hip)
def mfm_tail(h, bias, residual=None, pool=False, out=None):
    """pool(max(h[:, :C] + bias[:C], h[:, C:] + bias[C:]) + residual) of a contiguous float32 h [B, 2C, H, W] in one pass: the tail of a
    LightCNN layer behind its convolution without bias.  bias [2C] or None, residual [B, C, H, W] or None, pool = MaxPool2d(2, 2,
    ceil_mode=True).  out: a contiguous destination of the result's shape (a batch slice of a wider buffer, say)."""
    _f32_in("mfm_tail", h, bias, residual, out)
    if h.dim() != 4 or h.shape[1] % 2:
        raise ValueError("mfm_tail: need [B, 2C, H, W], got %s" % (tuple(h.shape),))
    B, C, H, W = h.shape[0], h.shape[1] // 2, h.shape[2], h.shape[3]
    _bias_ok(h, bias, 2 * C)
    if residual is not None and tuple(residual.shape) != (B, C, H, W):
        raise ValueError("mfm_tail: the residual must be [%d, %d, %d, %d]" % (B, C, H, W))
    shape = (B, C, (H + 1) // 2, (W + 1) // 2) if pool else (B, C, H, W)
    if out is None:
        out = h.new_empty(shape)
    elif tuple(out.shape) != shape:
        raise ValueError("mfm_tail: the destination must be %s" % (shape,))
    if out.numel():
        with _on_device(h) as stream:
            _lib.check(_lib.load().ffwm_mfm_tail_forward(_ptr(h), _ptr(bias), _ptr(residual), _ptr(out), B, C, H, W, int(bool(pool)),
                                                         _lib.F32, stream), "ffwm_mfm_tail_forward")
    return out


def identity_input(img, crop=False, out=None):
    """The identity network's input [B, 1, H, W] from img [B, Cin, H, W] in one launch: the channel mean, or with crop=True (128 x 128
    only) the reference's mean -> WarpNet(build_grid(B, 98)) -> F.interpolate(., (128, 128), mode="bilinear") (models/losses.py:85-112)."""
    _f32_in("identity_input", img, out)
    if img.dim() != 4 or img.shape[1] < 1:
        raise ValueError("identity_input: need [B, Cin, H, W], got %s" % (tuple(img.shape),))
    B, Cin, H, W = img.shape
    if crop and (H, W) != (128, 128):
        raise ValueError("identity_input: the centre-face crop is defined for 128 x 128 images only")
    if out is None:
        out = img.new_empty((B, 1, H, W))
    elif tuple(out.shape) != (B, 1, H, W):
        raise ValueError("identity_input: the destination must be [%d, 1, %d, %d]" % (B, H, W))
    if out.numel():
        with _on_device(img) as stream:
            _lib.check(_lib.load().ffwm_identity_input(_ptr(img), _ptr(out), B, Cin, H, W, int(bool(crop)), _lib.F32, stream),
                       "ffwm_identity_input")
    return out


def identity_input_backward(grad_out, cin, crop=False, out=None):
    """The adjoint of identity_input in one launch: grad_out [B, 1, H, W] -> d/d(img) [B, cin, H, W], overwritten (no zero-fill; `out`:
    a contiguous destination of that shape).  crop=False: grad_out / cin in every channel; crop=True (128 x 128 only): the transposed
    crop, a gather in a fixed order without atomics -- exactly 0 outside rows 27 .. 126 and columns 14 .. 113."""
    _f32_in("identity_input_backward", grad_out, out)
    cin = int(cin)
    if grad_out.dim() != 4 or grad_out.shape[1] != 1 or cin < 1:
        raise ValueError("identity_input_backward: need grad_out [B, 1, H, W] and cin >= 1, got %s, %d" % (tuple(grad_out.shape), cin))
    B, _, H, W = grad_out.shape
    if crop and (H, W) != (128, 128):
        raise ValueError("identity_input_backward: the centre-face crop is defined for 128 x 128 images only")
    if out is None:
        out = grad_out.new_empty((B, cin, H, W))
    elif tuple(out.shape) != (B, cin, H, W):
        raise ValueError("identity_input_backward: the destination must be [%d, %d, %d, %d]" % (B, cin, H, W))
    if out.numel():
        with _on_device(grad_out) as stream:
            _lib.check(_lib.load().ffwm_identity_input_backward(_ptr(grad_out), _ptr(out), B, cin, H, W, int(bool(crop)), _lib.F32, stream),
                       "ffwm_identity_input_backward")
    return out


def cosine_topk(probe, gallery, k):
    """-> (values [B, k] float32 descending, indices [B, k] int32): the k largest torch.cosine_similarity(gallery, probe[b]) per probe row;
    equal similarities: the lower gallery index first; NaN ranks above everything (topk's rule).  1 <= k <= min(G, 32), D <= 1024."""
    _f32_in("cosine_topk", probe, gallery)
    if probe.dim() != 2 or gallery.dim() != 2 or probe.shape[1] != gallery.shape[1]:
        raise ValueError("cosine_topk: probe [B, D] and gallery [G, D] expected")
    (B, D), G, k = probe.shape, gallery.shape[0], int(k)
    if not (1 <= k <= min(G, 32)) or not (1 <= D <= 1024) or B < 1:
        raise ValueError("cosine_topk: 1 <= k <= min(G, 32), 1 <= D <= 1024 and B >= 1 expected (B %d, G %d, D %d, k %d)" % (B, G, D, k))
    lib = _lib.load()
    need = lib.ffwm_cosine_topk_workspace_bytes(B, G, D, k)
    if need <= 0:
        raise ValueError("cosine_topk: the library refuses B %d, G %d, D %d, k %d" % (B, G, D, k))
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=probe.device)
    values = probe.new_empty((B, k))
    indices = torch.empty((B, k), dtype=torch.int32, device=probe.device)
    with _on_device(probe) as stream:
        _lib.check(lib.ffwm_cosine_topk(_ptr(probe), _ptr(gallery), _ptr(values), _ptr(indices), B, G, D, k, _ptr(ws), ws.numel() * 4,
                                        _lib.F32, stream), "ffwm_cosine_topk")
    return values, indices


# ---------------------------------------------------------------- fused L1 terms (csrc/l1_loss.hip)
class _L1Problem(ctypes.Structure):            # include/ffwm_hip.h: ffwm_l1_problem
    _fields_ = [("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("grad_x", ctypes.c_void_p),
                ("n", ctypes.c_int64), ("chw", ctypes.c_int64), ("hw", ctypes.c_int64), ("scale", ctypes.c_double),
                ("slot", ctypes.c_int)]


def _l1_table(terms, grads=None):
    """terms: [(x, y, mask or None, segments)], segments = [(x_row0, y_row0, rows, scale, slot)]: rows x_row0 .. x_row0 + rows of x
    against rows y_row0 .. of y (and of the mask, indexed like x).  One kernel problem per segment."""
    segs = []
    for i, (x, y, m, segments) in enumerate(terms):
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous() and y.dtype == x.dtype
                and y.shape[1:] == x.shape[1:]):
            raise ValueError("l1_multi: term %d needs contiguous float32 GPU tensors with equal trailing shapes" % i)
        row = x.numel() // max(x.shape[0], 1)
        if m is not None:
            if not (m.is_contiguous() and m.dtype == x.dtype and m.dim() == x.dim() and m.shape[0] == x.shape[0]
                    and m.shape[2:] == x.shape[2:] and m.shape[1] in (1, x.shape[1])):
                raise ValueError("l1_multi: term %d: the mask must be [B, 1 or C, ...] over x" % i)
            mrow = m.numel() // m.shape[0]
        for (x0, y0, rows, scale, slot) in segments:
            if x0 < 0 or y0 < 0 or x0 + rows > x.shape[0] or y0 + rows > y.shape[0]:
                raise ValueError("l1_multi: term %d: segment outside the tensors" % i)
            segs.append((x.data_ptr() + 4 * x0 * row, y.data_ptr() + 4 * y0 * row, None if m is None else m.data_ptr() + 4 * x0 * mrow,
                         None if grads is None or grads[i] is None else grads[i].data_ptr() + 4 * x0 * row,
                         rows * row, row if m is not None else 1, mrow if m is not None else 1, float(scale), int(slot)))
    arr = (_L1Problem * len(segs))()
    for a, sg in zip(arr, segs):
        a.x, a.y, a.mask, a.grad_x, a.n, a.chw, a.hw, a.scale, a.slot = sg
    return arr, len(segs)


def l1_multi_forward(terms, n_slots):
    """terms as in _l1_table -> out[n_slots] with out[slot] = sum over the segments of scale * sum |x m - y m| (one launch)."""
    out = torch.zeros(n_slots, device=terms[0][0].device, dtype=torch.float32)
    arr, n = _l1_table(terms)
    with _on_device(terms[0][0]) as stream:
        _lib.check(_lib.load().ffwm_l1_multi(ctypes.cast(arr, ctypes.c_void_p), n, _ptr(out), None, n_slots, _lib.F32, stream),
                   "ffwm_l1_multi")
    return out


def l1_multi_backward(terms, grad_out, need):
    """-> [grad_x or None per term]: grad_out[slot] * scale * sign(x m - y m) * m (one launch for all terms)."""
    sel = [i for i, nd in enumerate(need) if nd]
    if not sel:
        return [None] * len(terms)
    # rows no segment covers get no gradient: such a tensor starts from zeros
    grads = []
    for i in sel:
        x, segments = terms[i][0], terms[i][3]
        # the kernel WRITES a segment's rows (it does not accumulate): segments of one tensor must not overlap; rows none of them covers
        # get no gradient, so unless the segments tile the tensor exactly it starts from zeros
        spans = sorted((s0, s0 + r) for (s0, _, r, _, _) in segments)
        for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
            if b0 < a1:
                raise ValueError("l1_multi: term %d: segments [%d, %d) and [%d, %d) overlap (a row would keep only one gradient)"
                                 % (i, a0, a1, b0, b1))
        covered = bool(spans) and spans[0][0] == 0 and spans[-1][1] == x.shape[0] and all(a1 == b0 for (_, a1), (b0, _) in zip(spans, spans[1:]))
        grads.append(torch.empty_like(x) if covered else torch.zeros_like(x))
    arr, n = _l1_table([terms[i] for i in sel], grads)
    go = grad_out.contiguous()
    with _on_device(go) as stream:
        _lib.check(_lib.load().ffwm_l1_multi(ctypes.cast(arr, ctypes.c_void_p), n, None, _ptr(go), go.numel(), _lib.F32, stream),
                   "ffwm_l1_multi")
    out = [None] * len(terms)
    for i, g in zip(sel, grads):
        out[i] = g
    return out


# ---------------------------------------------------------------- device-resident face dataset
_FACE_TABLES = (("pairs", torch.int32), ("index", torch.int32), ("masks", torch.uint8), ("pair_lm", torch.int32), ("lm", torch.int32),
                ("lm_flip", torch.int32), ("gate", torch.float32))


def face_batch(images, pairs, index, masks=None, pair_lm=None, lm=None, lm_flip=None, gate=None, out=None):
    """One batch of the reference's FaceDataset from a device-resident store in ONE launch (csrc/face_batch.hip): images uint8
    [N, H, W, 3], pairs int32 [P, 2], index int32 [B] ON THE DEVICE -> {"img_S", "img_F": float32 [B, 3, H, W], "invalid": int32 [B]}
    (a test batch, index in [0, P)); with masks uint8 [N, H, W], pair_lm int32 [P, 3], lm / lm_flip int32 [K, L, 2] and gate float32
    [KG, L] a training batch (index in [0, 2 P), >= P flipped): also "mask_S", "mask_F" [B, 1, H, W], "lm_S", "lm_F" int64 [B, L, 2],
    "gate" [B, L, 1].  `out`: a dict of destinations of those shapes, written in place (a missing one is allocated).  No host-device
    copy and no synchronisation: an index out of range gives zeros and invalid[b] = 1, to be read when the caller chooses."""
    name = "face_batch"
    train = masks is not None
    tables = {"pairs": pairs, "index": index, "masks": masks, "pair_lm": pair_lm, "lm": lm, "lm_flip": lm_flip, "gate": gate}
    (N, H, W, P, K, KG, L, B), res = _face_batch_plan(name, images, tables, train, out)
    if B:
        with _on_device(images) as stream:
            _lib.check(_lib.load().ffwm_face_batch(
                _ptr(images), _ptr(masks), _ptr(pairs), _ptr(pair_lm), _ptr(lm), _ptr(lm_flip), _ptr(gate), _ptr(index),
                _ptr(res["img_S"]), _ptr(res["img_F"]), _ptr(res.get("mask_S")), _ptr(res.get("mask_F")), _ptr(res.get("lm_S")),
                _ptr(res.get("lm_F")), _ptr(res.get("gate")), _ptr(res["invalid"]), N, H, W, P, K, KG, L, B, int(train), stream),
                "ffwm_face_batch")
    return res


def _face_batch_plan(name, images, tables, train, out):
    """The checks of face_batch / face_batch_aug on the store's tables -> ((N, H, W, P, K, KG, L, B), the destinations)."""
    pairs, index, masks, pair_lm, lm, lm_flip, gate = (tables[k] for k, _ in _FACE_TABLES)
    if train and any(v is None for v in tables.values()):
        raise ValueError("%s: a training batch needs masks, pair_lm, lm, lm_flip and gate" % name)
    if not images.is_cuda:
        raise NotImplementedError("%s: ffwm_amd ops run on the GPU only (got a %s tensor); FaceStore.host_batch is the CPU path"
                                  % (name, images.device))
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise ValueError("%s: images must be contiguous uint8 [N, H, W, 3]" % name)
    for key, dt in _FACE_TABLES:
        t = tables[key]
        if train or key in ("pairs", "index"):
            if t.dtype != dt or t.device != images.device or not t.is_contiguous():
                raise ValueError("%s: %s must be a contiguous %s tensor on %s" % (name, key, dt, images.device))
    N, H, W, _ = images.shape
    if pairs.dim() != 2 or pairs.shape[1] != 2 or index.dim() != 1:
        raise ValueError("%s: pairs must be [P, 2] and index [B]" % name)
    P, B = pairs.shape[0], index.shape[0]
    K = KG = L = 0
    if train:
        if tuple(masks.shape) != (N, H, W):
            raise ValueError("%s: masks must be [%d, %d, %d]" % (name, N, H, W))
        if lm.dim() != 3 or lm.shape[2] != 2 or lm_flip.shape != lm.shape or gate.dim() != 2 or gate.shape[1] != lm.shape[1] \
                or tuple(pair_lm.shape) != (P, 3):
            raise ValueError("%s: need lm / lm_flip [K, L, 2], gate [KG, L] and pair_lm [P, 3]" % name)
        K, L, KG = lm.shape[0], lm.shape[1], gate.shape[0]
    shapes = {"img_S": ((B, 3, H, W), torch.float32), "img_F": ((B, 3, H, W), torch.float32), "invalid": ((B,), torch.int32)}
    if train:
        shapes.update({"mask_S": ((B, 1, H, W), torch.float32), "mask_F": ((B, 1, H, W), torch.float32),
                       "lm_S": ((B, L, 2), torch.int64), "lm_F": ((B, L, 2), torch.int64), "gate": ((B, L, 1), torch.float32)})
    res = {}
    for key, (shape, dt) in shapes.items():
        t = None if out is None else out.get(key)
        if t is None:
            t = torch.empty(shape, dtype=dt, device=images.device)
        elif tuple(t.shape) != shape or t.dtype != dt or t.device != images.device or not t.is_contiguous():
            raise ValueError("%s: the destination %s must be a contiguous %s tensor of shape %s on %s" % (name, key, dt, shape, images.device))
        res[key] = t
    return (N, H, W, P, K, KG, L, B), res


def face_batch_aug(images, pairs, index, masks, pair_lm, lm, lm_flip, gate, lm_raw, lm_raw_flip, slot, xtab, ytab, cs, load_size,
                   out=None):
    """face_batch's training batch with the S side rotated by a whole angle per sample, in ONE launch (ffwm_face_batch_aug in
    csrc/face_batch.hip: the rotation of the reference's --aug, stated as cv2.warpAffine's fixed-point bilinear path -- see
    ffwm_amd/data.py; no OpenCV was at hand to confirm its bytes).  Beside face_batch's arguments: lm_raw / lm_raw_flip float32
    [K, L, 2], slot int32 [B] ON THE DEVICE (the angle slot of every sample), xtab int32 [A, 2, W], ytab int32 [A, 2, H] and cs
    float32 [A, 2] (data.FaceRotation makes them), A <= 64.  img_S, mask_S and lm_S change; an index or a slot out of range gives
    zeros and invalid[b] = 1."""
    name = "face_batch_aug"
    tables = {"pairs": pairs, "index": index, "masks": masks, "pair_lm": pair_lm, "lm": lm, "lm_flip": lm_flip, "gate": gate}
    (N, H, W, P, K, KG, L, B), res = _face_batch_plan(name, images, tables, True, out)
    if not torch.is_tensor(xtab) or xtab.dim() != 3:
        raise ValueError("%s: xtab must be an int32 tensor [A, 2, %d]" % (name, W))
    for key, t, dt, shape in (("lm_raw", lm_raw, torch.float32, (K, L, 2)), ("lm_raw_flip", lm_raw_flip, torch.float32, (K, L, 2)),
                              ("slot", slot, torch.int32, (B,)), ("xtab", xtab, torch.int32, (xtab.shape[0], 2, W)),
                              ("ytab", ytab, torch.int32, (xtab.shape[0], 2, H)), ("cs", cs, torch.float32, (xtab.shape[0], 2))):
        if t.dtype != dt or t.device != images.device or not t.is_contiguous() or tuple(t.shape) != shape:
            raise ValueError("%s: %s must be a contiguous %s tensor of shape %s on %s" % (name, key, dt, shape, images.device))
    A = xtab.shape[0]
    if not 1 <= A <= 64 or load_size < 1:
        raise ValueError("%s: 1 to 64 angle slots and a positive load_size" % name)
    if B:
        with _on_device(images) as stream:
            _lib.check(_lib.load().ffwm_face_batch_aug(
                _ptr(images), _ptr(masks), _ptr(pairs), _ptr(pair_lm), _ptr(lm), _ptr(lm_flip), _ptr(gate), _ptr(index), _ptr(lm_raw),
                _ptr(lm_raw_flip), _ptr(slot), _ptr(xtab), _ptr(ytab), _ptr(cs), _ptr(res["img_S"]), _ptr(res["img_F"]),
                _ptr(res["mask_S"]), _ptr(res["mask_F"]), _ptr(res["lm_S"]), _ptr(res["lm_F"]), _ptr(res["gate"]), _ptr(res["invalid"]),
                N, H, W, P, K, KG, L, B, A, int(load_size), 1, stream), "ffwm_face_batch_aug")
    return res


# ---------------------------------------------------------------- LightCNN fine-tuning batches
def identity_batch(images, targets, index, matrix=None, flip=None, crop=False, out_side=128, out=None):
    """One batch of the reference's lightcnn ImgDataset from a device-resident store in ONE launch (csrc/identity_batch.hip): images
    uint8 [N, H, W, 3], targets int64 [N], index int32 [B] ON THE DEVICE -> {"img": float32 [B, 1, H, W] ([B, 1, out_side, out_side]
    with `crop`), "target": int64 [B], "invalid": int32 [B]}.  With matrix float64 [B, 6] and flip uint8 [B] a training batch (PIL's
    bicubic rotation under those inverse-map matrices, then the mirror); without them a test batch (byte / 255 and the channel mean).
    `out`: a dict of destinations of those shapes, written in place (a missing one is allocated).  No host-device copy and no
    synchronisation: an index out of range or a matrix that is not finite gives zeros, target 0 and invalid[b] = 1."""
    name = "identity_batch"
    augment = matrix is not None or flip is not None
    if augment and (matrix is None or flip is None):
        raise ValueError("%s: an augmented batch needs both matrix and flip" % name)
    if not images.is_cuda:
        raise NotImplementedError("%s: ffwm_amd ops run on the GPU only (got a %s tensor); IdentityStore.host_batch is the CPU path"
                                  % (name, images.device))
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3 or not images.is_contiguous():
        raise ValueError("%s: images must be contiguous uint8 [N, H, W, 3]" % name)
    tables = (("targets", targets, torch.int64), ("index", index, torch.int32)) + (
        (("matrix", matrix, torch.float64), ("flip", flip, torch.uint8)) if augment else ())
    for key, t, dt in tables:
        if t.dtype != dt or t.device != images.device or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %s tensor on %s" % (name, key, dt, images.device))
    N, H, W, _ = images.shape
    if tuple(targets.shape) != (N,) or index.dim() != 1:
        raise ValueError("%s: targets must be [%d] and index [B]" % (name, N))
    B = index.shape[0]
    if augment and (tuple(matrix.shape) != (B, 6) or tuple(flip.shape) != (B,)):
        raise ValueError("%s: matrix must be [%d, 6] and flip [%d]" % (name, B, B))
    crop, out_side = bool(crop), int(out_side)
    if crop and (H <= 30 or W <= 30 or out_side < 1):
        raise ValueError("%s: crop takes [28:-2, 15:-15] of the plane (H and W must exceed 30) and a positive out_side" % name)
    side = (out_side, out_side) if crop else (H, W)
    shapes = {"img": ((B, 1) + side, torch.float32), "target": ((B,), torch.int64), "invalid": ((B,), torch.int32)}
    res = {}
    for key, (shape, dt) in shapes.items():
        t = None if out is None else out.get(key)
        if t is None:
            t = torch.empty(shape, dtype=dt, device=images.device)
        elif tuple(t.shape) != shape or t.dtype != dt or t.device != images.device or not t.is_contiguous():
            raise ValueError("%s: the destination %s must be a contiguous %s tensor of shape %s on %s" % (name, key, dt, shape, images.device))
        res[key] = t
    if B:
        with _on_device(images) as stream:
            _lib.check(_lib.load().ffwm_identity_batch(
                _ptr(images), _ptr(targets), _ptr(index), _ptr(matrix) if augment else None, _ptr(flip) if augment else None,
                _ptr(res["img"]), _ptr(res["target"]), _ptr(res["invalid"]), N, H, W, B, out_side, int(augment), int(crop), stream),
                "ffwm_identity_batch")
    return res


# ---------------------------------------------------------------- result images (csrc/visuals.hip)
class _VisualItem(ctypes.Structure):           # include/ffwm_hip.h: ffwm_visual_item
    _fields_ = [("src", ctypes.c_void_p), ("palette", ctypes.c_void_p), ("out", ctypes.c_void_p), ("kind", ctypes.c_int),
                ("B", ctypes.c_int64), ("C", ctypes.c_int64), ("H", ctypes.c_int64), ("W", ctypes.c_int64)]


def visuals(items):
    """items: up to 16 tuples (tensor [B, C, H, W], kind, palette or None) with kind 0 image / 1 mask / 2 flow / 3 palette (uint8
    [256, 3] RGB on the device) -> a list of uint8 [B, H, W, 3] RGB sheets, one per item, written by ONE call (two launches with a
    flow item, else one) as the reference's tensor2im / tensor2mask / tensor2flow / tensor2att write them on the host.  The sheets are
    views of one allocation (16-byte aligned each), so they cross to the host in one copy.  Tensors are taken through
    .float().contiguous(), as the reference calls .float()."""
    name = "visuals"
    if not items:
        return []
    if len(items) > 16:
        raise ValueError("%s: at most 16 items per call, got %d" % (name, len(items)))
    srcs, pals, offsets, total = [], [], [], 0
    dev = items[0][0].device
    for i, (t, kind, pal) in enumerate(items):
        if not t.is_cuda:
            raise NotImplementedError("%s: ffwm_amd ops run on the GPU only (got a %s tensor); ffwm_amd.visuals.render is the CPU path"
                                      % (name, t.device))
        if t.device != dev:
            raise ValueError("%s: tensors live on different devices (%s vs %s)" % (name, t.device, dev))
        if t.dim() != 4 or t.numel() == 0:
            raise ValueError("%s: item %d: expected a non-empty 4-D NCHW tensor, got shape %s" % (name, i, tuple(t.shape)))
        if kind == 3:
            if pal is None:
                raise ValueError("%s: item %d: a palette item needs its uint8 [256, 3] palette" % (name, i))
            if not (pal.is_cuda and pal.device == dev and pal.dtype == torch.uint8 and tuple(pal.shape) == (256, 3)):
                raise ValueError("%s: item %d: the palette must be a uint8 [256, 3] tensor on %s" % (name, i, dev))
            pal = pal.contiguous()
        else:
            pal = None
        srcs.append(t.detach().float().contiguous())
        pals.append(pal)
        offsets.append(total)
        B, _, H, W = t.shape
        total += (3 * B * H * W + 15) // 16 * 16
    sheet = torch.empty(total, dtype=torch.uint8, device=dev)
    arr = (_VisualItem * len(items))()
    outs = []
    for a, s, pal, off, (_, kind, _) in zip(arr, srcs, pals, offsets, items):
        B, C, H, W = s.shape
        out = sheet[off:off + 3 * B * H * W].view(B, H, W, 3)
        a.src, a.palette, a.out, a.kind, a.B, a.C, a.H, a.W = s.data_ptr(), _ptr(pal), out.data_ptr(), int(kind), B, C, H, W
        outs.append(out)
    lib = _lib.load()
    table = ctypes.cast(arr, ctypes.c_void_p)
    nbytes = lib.ffwm_visuals_workspace_bytes(table, len(items))
    if nbytes < 0:
        _lib.check(int(nbytes), "ffwm_visuals_workspace_bytes")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev) if nbytes else None
    with _on_device(srcs[0]) as stream:
        _lib.check(lib.ffwm_visuals(table, len(items), _ptr(ws), nbytes, _lib.F32, stream), "ffwm_visuals")
    return outs
