"""The reference's result images: util/util.py (tensor2im / tensor2mask / tensor2flow / tensor2att), util/flow_util.py (flow2img) and the
routing and file names of util/visualizer.py (display_test_results, display_current_results), for whole batches.

    from ffwm_amd import ResultWriter
    from ffwm_amd.visuals import from_result
    w = ResultWriter("checkpoints/ffwm/test/multipie")
    r = frontalizer(img_S)
    w.save_test(from_result(r, img_S, img_F, extra=("flow_F128",)), prefixes)          # <prefix>_<label>.png per image and label

CUDA tensors are rendered by ONE call into csrc/visuals.hip (ops.visuals): uint8 [B, H, W, 3] sheets on the device, one
device-to-host copy of the bytes instead of one float32 `.cpu()` per label and image.  CPU tensors go through the numpy restatements
below, which are also what the tests hold the kernel to.  Both follow the same stated arithmetic (include/ffwm_hip.h):

  * to_u8: ONE rule for every float -> byte conversion: truncate toward zero to int32, keep the low 8 bits; NaN, +-inf and
    |t| >= 2^31 give 0.  On [0, 256) that is numpy's astype(uint8), which the reference uses; outside it numpy's cast is undefined.
  * a flow is coloured in float32 up to and including u / maxrad and in float64 from there on, as the reference is under NumPy 2
    (finfo(float).eps is a float64 scalar and promotes the float32 array).

The library ships NO colour map for tensor2att: the reference's is cv2.COLORMAP_JET, OpenCV's table, and a table typed from memory
would be uncertified bytes (the position data.py takes on aug=True).  Pass `palette`, a uint8 [256, 3] RGB table.
"""
import collections
import os

import numpy as np

IMAGE, MASK, FLOW, PALETTE = 0, 1, 2, 3
MAX_ITEMS = 16                   # items of one ffwm_visuals call (csrc/visuals.hip: kVisMax)
FLOW_REDUCTION_BLOCK = 1024      # threads of the one workgroup that reduces a flow image's maximum (csrc/visuals.hip: kFlowBlock);
FLOW_REDUCTION_PASS = 4096       # cells it covers per pass where a plane takes float4 loads (H*W % 4 == 0), else FLOW_REDUCTION_BLOCK
PIXELS_PER_BLOCK = 1024          # pixels a workgroup of the colouring pass owns (kVisPerBlock = kBlock * kVisPix)

PALETTE_HINT = ("tensor2att needs a palette (uint8 [256, 3], RGB): the library ships no JET table.  Where OpenCV exists, "
                "cv2.applyColorMap(np.arange(256, dtype=np.uint8).reshape(256, 1), cv2.COLORMAP_JET)[:, 0, ::-1] is the reference's")


# ------------------------------------------------------------------------------------------------ host restatements
def to_u8(t):
    """The stated float -> byte rule (module docstring), elementwise on a float32 or float64 array."""
    t = np.asarray(t)
    with np.errstate(invalid="ignore"):
        ok = np.abs(t) < 2147483648.0                       # False for NaN and +-inf
        i = np.trunc(np.where(ok, t, 0)).astype(np.int64)
    return (i & 255).astype(np.uint8)


def color_wheel():
    """flow_util.make_color_wheel: the 55 Middlebury colours [55, 3] (float64 holding integers): segments RY 15, YG 6, GC 4, CB 11,
    BM 13, MR 6, one channel at 255, one ramping by floor(255 i / n), up or down."""
    wheel = np.zeros((55, 3))
    col = 0
    for n, full, ramp, falls in ((15, 0, 1, False), (6, 1, 0, True), (4, 1, 2, False), (11, 2, 1, True), (13, 2, 0, False),
                                 (6, 0, 2, True)):
        r = np.floor(255 * np.arange(n) / n)
        wheel[col:col + n, full] = 255
        wheel[col:col + n, ramp] = 255 - r if falls else r
        col += n
    return wheel


def _sample(x, idx):
    """image idx of a [B, C, H, W] torch tensor or numpy array as float32 numpy [C, H, W] (`tensor[idx].cpu().float().numpy()`)."""
    if isinstance(x, np.ndarray):
        return np.asarray(x[idx], dtype=np.float32)
    return x.detach()[idx].cpu().float().numpy()


def tensor2im(input_image, idx=0):
    """util.tensor2im: [H, W, 3] uint8 of image idx; a 1-channel image is (x - 0.5) * 2 on three channels, then * 255."""
    x = _sample(input_image, idx)
    if x.shape[0] == 1:
        x = np.tile((x - np.float32(0.5)) * np.float32(2), (3, 1, 1))
    return to_u8(np.transpose(x, (1, 2, 0)) * np.float32(255.0))


def tensor2mask(input_image, idx=0):
    """util.tensor2mask: x * 255, a 1-channel mask tiled to three channels."""
    x = _sample(input_image, idx)
    if x.shape[0] == 1:
        x = np.tile(x, (3, 1, 1))
    return to_u8(np.transpose(x, (1, 2, 0)) * np.float32(255.0))


def tensor2att(input_image, palette, idx=0):
    """util.tensor2att with the colour map as an argument: palette[u8(x[0] * 255)], palette uint8 [256, 3] in RGB."""
    if palette is None:
        raise ValueError(PALETTE_HINT)
    pal = palette if isinstance(palette, np.ndarray) else palette.detach().cpu().numpy()
    if pal.shape != (256, 3) or pal.dtype != np.uint8:
        raise ValueError("palette must be uint8 [256, 3], got %s %s" % (pal.dtype, pal.shape))
    x = _sample(input_image, idx)
    return pal[to_u8(x[0] * np.float32(255.0))]


def _nudge(a, ulps):
    for _ in range(abs(int(ulps))):
        a = np.nextafter(a, np.inf if ulps > 0 else -np.inf)
    return a


def tensor2flow(flow, idx=0, atan2_ulps=0):
    """util.tensor2flow + flow_util.flow2img: the sampling grid [B, 2, H, W] in [-1, 1] as a Middlebury colour image [H, W, 3].
    Both axes scale with H, as in the reference.  atan2_ulps moves arctan2's result by that many float64 ulps (tests: which pixels
    an atan2 of another libm could colour differently)."""
    f = _sample(flow, idx)
    if f.shape[0] != 2:
        raise ValueError("a flow has 2 channels, got %d" % f.shape[0])
    H, W = f.shape[1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.clip((f + np.float32(1)) * np.float32(H / 2), np.float32(0), np.float32(H - 1))          # NaN passes, as torch.clamp
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
        u, v = g[0] - xx, g[1] - yy
        rad = np.sqrt(u * u + v * v)
        m = np.max(rad)                                      # NaN if any cell is
        maxrad = m if m > -1 else np.float32(-1)             # Python's max(-1, nan) is -1
        eps = np.finfo(np.float64).eps
        ud, vd = (u / maxrad).astype(np.float64) + eps, (v / maxrad).astype(np.float64) + eps          # float32 division, float64 after
        nan = np.isnan(ud) | np.isnan(vd)
        ud, vd = np.where(nan, 0.0, ud), np.where(nan, 0.0, vd)
        radd = np.sqrt(ud * ud + vd * vd)
        a = _nudge(np.arctan2(-vd, -ud), atan2_ulps) / np.pi
        fk = (a + 1) / 2 * 54 + 1
        k0 = np.floor(fk)
        frac = fk - k0
        k0 = k0.astype(np.int64)
        i0, i1 = (k0 - 1) % 55, k0 % 55                      # k1 = k0 + 1 with 56 -> 1; numpy's wheel[k - 1] wraps k = 0 the same way
        wheel = color_wheel()
        img = np.zeros((H, W, 3), np.uint8)
        for ch in range(3):
            col = (1 - frac) * (wheel[i0, ch] / 255) + frac * (wheel[i1, ch] / 255)
            col = np.where(radd <= 1, 1 - radd * (1 - col), col * 0.75)
            img[:, :, ch] = to_u8(np.floor(255 * col))
        img[nan] = 0
    return img


# ------------------------------------------------------------------------------------------------ routing
def kind_of(label, test=True):
    """The converter util/visualizer.py picks for a label: display_test_results (test=True) asks 'att', then 'mask', then 'flow' in
    the label, else image; display_current_results (test=False) knows 'mask' and image only."""
    if test:
        if "att" in label:
            return PALETTE
        if "mask" in label:
            return MASK
        if "flow" in label:
            return FLOW
        return IMAGE
    return MASK if "mask" in label else IMAGE


def _host_render(x, kind, palette):
    fn = {IMAGE: tensor2im, MASK: tensor2mask, FLOW: tensor2flow}.get(kind)
    imgs = [tensor2att(x, palette, idx=i) if kind == PALETTE else fn(x, idx=i) for i in range(x.shape[0])]
    return np.stack(imgs)


def render(visuals, test=True, palette=None):
    """visuals: OrderedDict label -> [B, C, H, W] tensor  ->  OrderedDict label -> uint8 [B, H, W, 3] (RGB), each on its tensor's
    device.  The CUDA tensors of the call take one ops.visuals call per 16 labels; CPU tensors go through the restatements."""
    import torch
    kinds = collections.OrderedDict((label, kind_of(label, test)) for label in visuals)
    if palette is None and PALETTE in kinds.values():
        raise ValueError(PALETTE_HINT)
    out = collections.OrderedDict((label, None) for label in visuals)
    dev = [label for label, x in visuals.items() if x.is_cuda]
    for i in range(0, len(dev), MAX_ITEMS):
        from . import ops
        chunk = dev[i:i + MAX_ITEMS]
        items = []
        for label in chunk:
            pal = None
            if kinds[label] == PALETTE:
                pal = palette if torch.is_tensor(palette) else torch.from_numpy(np.ascontiguousarray(palette))
                pal = pal.to(visuals[label].device)
            items.append((visuals[label], kinds[label], pal))
        for label, sheet in zip(chunk, ops.visuals(items)):
            out[label] = sheet
    for label, x in visuals.items():
        if not x.is_cuda:
            out[label] = torch.from_numpy(_host_render(x, kinds[label], palette))
    return out


def to_host(rendered):
    """render()'s result as numpy arrays.  The sheets of one ops.visuals call are views of one allocation: it crosses once."""
    bases, out = {}, collections.OrderedDict()
    for label, t in rendered.items():
        base = t._base if t.is_cuda and t._base is not None else None
        if base is None:
            out[label] = t.cpu().numpy()
            continue
        key = (base.data_ptr(), base.numel())
        if key not in bases:
            bases[key] = base.cpu().numpy()
        off = t.storage_offset() - base.storage_offset()
        out[label] = bases[key][off:off + t.numel()].reshape(tuple(t.shape))
    return out


# ------------------------------------------------------------------------------------------------ files
class ResultWriter(object):
    """The image files of the reference's Visualizer: save_test is display_test_results for every image of a batch
    (`<test_dir>/<prefix>_<label>.png`), save_train display_current_results (`<img_dir>/epoch%.3d_<label>.png`, image 0).  PNGs through
    PIL in RGB; the reference's cv2.imwrite of the RGB -> BGR converted array decodes to the same pixels."""

    def __init__(self, test_dir, img_dir=None, palette=None):
        self.test_dir = test_dir
        self.img_dir = img_dir if img_dir is not None else test_dir
        self.palette = palette

    @staticmethod
    def _save(array, path):
        from PIL import Image
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        Image.fromarray(np.ascontiguousarray(array)).save(path)

    def save_test(self, visuals, prefixes):
        """One render, one copy of the sheet, one file per image and label -> the paths written.  prefixes: one per image of the
        batch (the reference's os.path.splitext(name)[0]); None skips that image (not in visual_list)."""
        host = to_host(render(visuals, test=True, palette=self.palette))
        paths = []
        for label, sheet in host.items():
            if len(prefixes) != sheet.shape[0]:
                raise ValueError("%s has %d images, %d prefixes were given" % (label, sheet.shape[0], len(prefixes)))
        for idx, prefix in enumerate(prefixes):
            if prefix is None:
                continue
            for label, sheet in host.items():
                paths.append(os.path.join(self.test_dir, "%s_%s.png" % (prefix, label)))
                self._save(sheet[idx], paths[-1])
        return paths

    def save_train(self, visuals, epoch):
        """display_current_results: image 0 of every visual as epoch%.3d_<label>.png ('mask' labels as masks, the rest as images)."""
        first = collections.OrderedDict((label, x[:1]) for label, x in visuals.items())
        host = to_host(render(first, test=False))
        paths = []
        for label, sheet in host.items():
            paths.append(os.path.join(self.img_dir, "epoch%.3d_%s.png" % (epoch, label)))
            self._save(sheet[0], paths[-1])
        return paths


# ------------------------------------------------------------------------------------------------ the reference's visual_names
def from_result(r, img_S, img_F=None, extra=()):
    """The visuals of test_ffwm.py (visual_names = img_S, img_F, fake_F128) from a FrontalizerResult; extra: any of 'img_S_warp',
    'att', 'flow_F128' (r.flows[0]).  img_F is left out when the caller has no ground truth."""
    v = collections.OrderedDict()
    v["img_S"] = img_S
    if img_F is not None:
        v["img_F"] = img_F
    v["fake_F128"] = r.fake_F128
    for name in extra:
        if name == "flow_F128":
            v[name] = r.flows[0]
        elif name in ("img_S_warp", "att"):
            v[name] = getattr(r, name)
        else:
            raise ValueError("from_result: no visual named %r" % (name,))
    return v


def train_visuals(trainer, b):
    """The eight training visuals of models/ffwm_model.py:208 from a batch and what FFWMTrainer keeps, detached, after a step."""
    return collections.OrderedDict([
        ("img_S", b["img_S"]), ("img_F", b["img_F"]), ("img_S_warp", trainer.img_S_warp), ("fake_F32", trainer.fake32),
        ("fake_F64", trainer.fake64), ("fake_F128", trainer.fake128), ("img_S_rec", trainer.img_S_rec),
        ("img_GF128", trainer.img_GF128)])
