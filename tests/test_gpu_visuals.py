"""Result images on the GPU (csrc/visuals.hip through ops.visuals and ffwm_amd.visuals.render) against the numpy restatements of
ffwm_amd/visuals.py, which tests/test_visuals_cpu.py holds to the reference's own bytes.

IMAGE, MASK and PALETTE items are float32 arithmetic with one rounding per operation: bit-equal.  A FLOW item passes through a
float64 atan2, and the device's is another libm's than numpy's: a pixel is compared exactly where moving arctan2's result by +-4 ulp
changes none of its bytes (decided, tests/visual_cases.py: undecided), and within 1 level elsewhere.  The +-4 ulp window supposes the
device's double atan2 good to a couple of ulp; a mismatch on a decided pixel is a finding, not a reason to widen it."""
import collections
import ctypes

import numpy as np
import pytest
import torch

import visual_cases as cases
from ffwm_amd import _lib, graphs, ops
from ffwm_amd import visuals as V

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64


def _host(kind, x, palette=None):
    if kind == V.PALETTE:
        return np.stack([V.tensor2att(x, palette, idx=i) for i in range(x.shape[0])])
    fn = {V.IMAGE: V.tensor2im, V.MASK: V.tensor2mask, V.FLOW: V.tensor2flow}[kind]
    return np.stack([fn(x, idx=i) for i in range(x.shape[0])])


@pytest.fixture(scope="module")
def flow_refs():
    """name -> [(restated image, undecided mask)] per image: computed once, shared, never written."""
    refs = collections.OrderedDict()
    for name, f in cases.flow_cases().items():
        refs[name] = [cases.undecided(f, i)[:2] for i in range(f.shape[0])]
    return refs


def _call_with_guards(rows):
    """rows: [(array, kind, palette or None)] -> the outputs of ONE ffwm_visuals call whose destinations sit in one buffer with GUARD
    bytes of 0xA5 in front of, between and behind them; asserts that no guard byte changed."""
    srcs = [torch.from_numpy(x).to(DEV) for x, _, _ in rows]
    pals = [None if p is None else torch.from_numpy(p).to(DEV) for _, _, p in rows]
    offs, total = [], GUARD
    for x, _, _ in rows:
        offs.append(total)
        total += (3 * x.shape[0] * x.shape[2] * x.shape[3] + 3) // 4 * 4 + GUARD
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device=DEV)
    arr = (ops._VisualItem * len(rows))()
    for a, s, p, off, (x, kind, _) in zip(arr, srcs, pals, offs, rows):
        a.src, a.palette, a.out, a.kind = s.data_ptr(), None if p is None else p.data_ptr(), buf.data_ptr() + off, kind
        a.B, a.C, a.H, a.W = x.shape
    lib = _lib.load()
    table = ctypes.cast(arr, ctypes.c_void_p)
    nbytes = lib.ffwm_visuals_workspace_bytes(table, len(rows))
    assert nbytes == 4 * sum(x.shape[0] for x, kind, _ in rows if kind == V.FLOW)
    ws = torch.full((max(nbytes // 4, 1) + 2,), float("nan"), device=DEV)
    _lib.check(lib.ffwm_visuals(table, len(rows), ws.data_ptr() if nbytes else None, nbytes, _lib.F32,
                                torch.cuda.current_stream().cuda_stream), "ffwm_visuals")
    host = buf.cpu().numpy()
    assert torch.isnan(ws[nbytes // 4:]).all(), "the workspace was written past one float per flow image"
    written = np.zeros(total, bool)
    outs = []
    for off, (x, _, _) in zip(offs, rows):
        n = 3 * x.shape[0] * x.shape[2] * x.shape[3]
        written[off:off + n] = True
        outs.append(host[off:off + n].reshape(x.shape[0], x.shape[2], x.shape[3], 3))
    assert (host[~written] == 0xA5).all(), "bytes outside the outputs were written"
    return outs


def _assert_flow(name, got, refs):
    for i, (ref, und) in enumerate(refs):
        diff = np.abs(got[i].astype(np.int32) - ref.astype(np.int32)).max(axis=2)
        bad = int((diff[~und] != 0).sum())
        print("%s[%d]: %d of %d pixels differ (largest step %d), %d undecided, %d decided pixels differ"
              % (name, i, int((diff != 0).sum()), diff.size, int(diff.max()), int(und.sum()), bad))
        assert bad == 0, (name, i, bad)
        assert (diff[und] <= 1).all(), (name, i, int(diff[und].max()))


@pytest.mark.parametrize("kind", [V.IMAGE, V.MASK])
def test_image_and_mask_items_are_bit_equal(kind):
    for name, x in cases.image_cases().items():
        got, = _call_with_guards([(x, kind, None)])
        assert (got == _host(kind, x)).all(), name


def test_palette_item_is_bit_equal():
    x, pal = cases.palette_case()
    got, = _call_with_guards([(x, V.PALETTE, pal)])
    assert (got == _host(V.PALETTE, x, pal)).all()
    s = cases.image_cases()["special_1x3x4x4"]                  # C = 3: only channel 0 is looked at; NaN, inf and 300 index the table
    got, = _call_with_guards([(s, V.PALETTE, pal)])
    assert (got == _host(V.PALETTE, s, pal)).all()


def test_mixed_table_in_one_call(flow_refs):
    """Items of different sizes and kinds in one call: fake_F32 beside fake_F128, an odd-sized mask, a flow and a palette item."""
    x, pal = cases.palette_case()
    rows = [(a, kind, None) for _, kind, a in cases.mixed_table()]
    rows += [(cases.flow_cases()["odd_2x5x7"], V.FLOW, None), (x, V.PALETTE, pal), (cases.flow_cases()["uniform_20"], V.FLOW, None)]
    outs = _call_with_guards(rows)
    for got, (a, kind, p) in zip(outs, rows):
        if kind != V.FLOW:
            assert (got == _host(kind, a, p)).all()
    _assert_flow("odd_2x5x7", outs[3], flow_refs["odd_2x5x7"])
    _assert_flow("uniform_20", outs[5], flow_refs["uniform_20"])


def test_flow_items_match_on_every_decided_pixel(flow_refs):
    for name, f in cases.flow_cases().items():
        got, = _call_with_guards([(f, V.FLOW, None)])
        _assert_flow(name, got, flow_refs[name])
    got, = _call_with_guards([(cases.flow_cases()["identity_8"], V.FLOW, None)])
    assert not got.any()                                         # no motion: black


def _device_items():
    x, pal = cases.palette_case()
    return [(torch.from_numpy(cases.image_cases()["rgb_2x3x5x7"]).to(DEV), V.IMAGE, None),
            (torch.from_numpy(cases.flow_cases()["uniform_20"]).to(DEV), V.FLOW, None),
            (torch.from_numpy(x).to(DEV), V.PALETTE, torch.from_numpy(pal).to(DEV)),
            (torch.from_numpy(cases.image_cases()["gray_2x1x5x7"]).to(DEV), V.MASK, None)]


def test_two_calls_give_identical_bytes():
    items = _device_items()
    a, b = ops.visuals(items), ops.visuals(items)
    assert len(a) == len(b) == 4 and a[0]._base is a[3]._base and all(t.data_ptr() % 16 == 0 for t in a)
    for s, t, (x, _, _) in zip(a, b, items):
        assert s.dtype == torch.uint8 and tuple(s.shape) == (x.shape[0], x.shape[2], x.shape[3], 3) and torch.equal(s, t)
    with pytest.raises(ValueError):
        ops.visuals(items * 5)
    with pytest.raises(ValueError):
        ops.visuals([(items[2][0], V.PALETTE, None)])
    with pytest.raises(_lib.FFWMError):
        ops.visuals([(items[1][0], V.IMAGE, None)])              # C = 2 is not an image


def test_captured_call_follows_its_input_buffers(flow_refs):
    items = _device_items()
    graphs.warm_up(lambda: ops.visuals(items), 2, sync=True)
    g, outs = graphs.capture(lambda: ops.visuals(items))
    new_img = np.ascontiguousarray(cases.image_cases()["rgb_2x3x5x7"][::-1] * np.float32(0.5))
    new_flow = cases.flow_cases()["uniform_20"][:, ::-1].copy() * np.float32(0.25)
    items[0][0].copy_(torch.from_numpy(new_img))                 # in place: the graph was captured on these addresses
    items[1][0].copy_(torch.from_numpy(new_flow))
    g.replay()
    torch.cuda.synchronize()
    assert (outs[0].cpu().numpy() == _host(V.IMAGE, new_img)).all()
    ref, und, _ = cases.undecided(new_flow, 0)
    _assert_flow("replayed uniform_20", outs[1].cpu().numpy(), [(ref, und)])
    assert (outs[3].cpu().numpy() == _host(V.MASK, cases.image_cases()["gray_2x1x5x7"])).all()


def test_render_on_cuda_tensors_equals_render_on_their_cpu_copies(flow_refs):
    x, pal = cases.palette_case()
    v = collections.OrderedDict()
    v["img_S"] = torch.from_numpy(cases.image_cases()["rgb_2x3x5x7"])
    v["mask_S"] = torch.from_numpy(cases.image_cases()["gray_2x1x5x7"])
    v["flow_F128"] = torch.from_numpy(cases.flow_cases()["two_scales_2x8"])
    v["att"] = torch.from_numpy(x)
    v["fake_F128"] = torch.from_numpy(cases.mixed_table()[1][2])
    on_cpu = V.render(v, palette=pal)
    on_gpu = V.render(collections.OrderedDict((k, t.to(DEV)) for k, t in v.items()), palette=pal)
    assert list(on_gpu) == list(v) and all(t.is_cuda for t in on_gpu.values())
    host = V.to_host(on_gpu)
    for label in v:
        if label == "flow_F128":
            assert (on_cpu[label].numpy() == np.stack([r for r, _ in flow_refs["two_scales_2x8"]])).all()
            _assert_flow(label, host[label], flow_refs["two_scales_2x8"])
        else:
            assert (host[label] == on_cpu[label].numpy()).all(), label
        assert (host[label] == on_gpu[label].cpu().numpy()).all()      # the one copy of the sheet holds what the views hold
    # half-precision input goes through .float(), as the reference's .cpu().float() does
    h = v["img_S"].to(DEV).half()
    assert (V.render({"img_S": h})["img_S"].cpu().numpy() == V.render({"img_S": h.cpu()})["img_S"].numpy()).all()
