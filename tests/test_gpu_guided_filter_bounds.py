"""The guided-filter kernels (csrc/guided_filter.hip) against the per-element float64 bounds, the exact windows and the small
contracts of tests/guided_filter_bounds.py, on every route: the four-launch kernels, the general kernels with column chunks of 32, 64
and 128 rows, a window longer than a row chunk, a one-channel guide.  Every test checks by launch name that the route it claims ran.

What is asserted, per case of gb.CASES:
  bounds   float32 with u = 2^-24 on the families uniform, planes, image, offset; float64 with u64 = 2^-53 on planes and image: the
           saved planes mean_x, mean_y, A, var_x + eps, mean_A and the output against the float64 closed form, element by element;
           grad_x, grad_y against the closed-form backward of the kernel's OWN saved planes.
  exact    integer inputs: mean_x, mean_y == float32(S) / float32(N), bit for bit.
and once each: a NaN stays in the planes it can reach; the workspace's contents do not matter; the general entry points hand a fast
shape to the four-launch kernels.

Worst error / bound seen on an MI355X (SAFETY = 4; printed as GFBOUND lines by every test): GPU_RATIOS below.
"""
import contextlib

import pytest
import torch

import guided_filter_bounds as gb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "f64": torch.float64}
RUNS = [(name, fam, "f32") for name in gb.CASES for fam in gb.FAMILIES] + [(name, fam, "f64") for name in gb.CASES for fam in ("planes", "image")]
SCOPES = {("fwd", "fast"): "guided_filter_fwd", ("fwd", "general"): "guided_filter_fwd_general",
          ("bwd", "fast"): "guided_filter_bwd", ("bwd", "general"): "guided_filter_bwd_general"}
# the largest error / bound per route over all cases and families, recorded from the GFBOUND lines of a run on an MI355X (a record,
# not a threshold: the assertion is error / bound <= 1).  The worst plane is mean_x / mean_y forward and grad_y backward on every route.
GPU_RATIOS = {
    # route:           (forward f32, backward f32, forward f64, backward f64)
    "fast":            (0.0485, 0.0023, 0.0307, 0.0021),
    "general/rc=32":   (0.0165, 0.0036, 0.0078, 0.0029),
    "general/rc=64":   (0.0246, 0.0037, 0.0164, 0.0040),
    "general/rc=128":  (0.0265, 0.0035, 0.0143, 0.0038),
}


@contextlib.contextmanager
def _profiled():
    """Profile what runs inside; yields the set the launch names (without their size suffix) are collected into."""
    from ffwm_amd import _lib
    names = set()
    _lib.prof_reset()
    _lib.prof_enable(True)
    try:
        yield names
        torch.cuda.synchronize()
        names.update(k.split("@")[0] for k in _lib.prof_collect())
    finally:
        _lib.prof_enable(False)


def _gf_names(names):
    return {n for n in names if n.startswith("guided_filter")}


def _shape(case):
    B, Cx, Cy, H, W, r, want_y = case
    return B, Cx, Cy, H, W, r, want_y, B * Cx, B * Cy


def _hip(case, x, y, g, dtype):
    """One forward and backward through ffwm_amd.ops.  -> planes (dict, on the CPU, flat), grads (dict), launch names."""
    from ffwm_amd import ops
    B, Cx, Cy, H, W, r, want_y, Px, Py = _shape(case)
    xd, yd, gd = x.to(DEV, dtype).view(B, Cx, H, W), y.to(DEV, dtype).view(B, Cy, H, W), g.to(DEV, dtype).view(B, Cy, H, W)
    with _profiled() as names:
        out, saved = ops.guided_filter_forward(xd, yd, r)
        gx, gy = ops.guided_filter_backward_xy(xd, yd, saved, gd, r, True, want_y)
    planes = gb.split_saved(saved.cpu(), Px, Py, H, W)
    planes["out"] = out.cpu().view(Py, H, W)
    grads = {"grad_x": gx.cpu().view(Px, H, W), "grad_y": None if gy is None else gy.cpu().view(Py, H, W)}
    return planes, grads, _gf_names(names)


def _assert_route(name, names):
    _, fwd, bwd, _ = gb.CASES[name]
    assert names == {SCOPES["fwd", fwd], SCOPES["bwd", bwd]}, (name, sorted(names))


@pytest.mark.parametrize("name,family,prec", RUNS, ids=["-".join(r) for r in RUNS])
def test_every_plane_within_its_bound(name, family, prec):
    case = gb.CASES[name][0]
    dtype = DT[prec]
    x, y, g = (t.to(dtype) for t in gb.inputs(name, family))
    fp, bp = gb.plans(case)
    planes, grads, names = _hip(case, x, y, g, dtype)
    _assert_route(name, names)
    fwd = gb.ForwardBound(fp, x, y)
    saved = {k: planes[k] for k in ("mean_x", "mean_y", "A", "ve", "mean_A")}
    bwd = gb.BackwardBound(bp, x, y, g, saved)
    ratios = fwd.ratios(planes)
    ratios.update(bwd.ratios(grads))
    print("GFBOUND gpu %s fwd=%s bwd=%s %s %s: %s" % (name, fp, bp, family, prec, " ".join("%s %.3g" % kv for kv in ratios.items())))
    assert len(ratios) == (8 if case[6] else 7)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, "error / bound above 1: %s" % bad


@pytest.mark.parametrize("name", list(gb.CASES))
def test_integer_windows_are_exact(name):
    case = gb.CASES[name][0]
    x, y, g = gb.inputs(name, "integers")
    fp, _ = gb.plans(case)
    mx, my = gb.exact_means(x, y, case[5], fp.kind == "fast")
    planes, _, names = _hip(case, x, y, g, torch.float32)
    _assert_route(name, names)
    for key, ref in (("mean_x", mx), ("mean_y", my)):
        same = planes[key] == ref
        assert bool(same.all()), "%s: %d of %d values differ, first at %s" % (key, int((~same).sum()), same.numel(),
                                                                               tuple(int(i) for i in (~same).nonzero()[0]))


# ------------------------------------------------------------------------------------------------ non-finite containment
NAN_CASES = ["fast_ragged", "guide1_long_lines"]


def _near(H, W, i0, j0, d):
    i, j = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    return ((i - i0).abs() <= d) & ((j - j0).abs() <= d)


def _same(a, b):
    return torch.equal(a, b)


@pytest.mark.parametrize("name", NAN_CASES)
def test_a_nan_in_x_stays_in_its_guide(name):
    case = gb.CASES[name][0]
    B, Cx, Cy, H, W, r, want_y, Px, Py = _shape(case)
    cdiv = Py // Px
    x, y, g = gb.inputs(name, "uniform")
    clean_p, clean_g, _ = _hip(case, x, y, g, torch.float32)
    i0, j0 = H // 2, W // 3
    xn = x.clone()
    xn[0, i0, j0] = float("nan")
    planes, grads, names = _hip(case, xn, y, g, torch.float32)
    _assert_route(name, names)
    for key, per_x in (("mean_x", True), ("ve", True), ("mean_y", False), ("A", False), ("mean_A", False), ("out", False)):
        first = 1 if per_x else cdiv                       # the planes of guide 0 come first
        assert _same(planes[key][first:], clean_p[key][first:]), key
    assert _same(planes["mean_y"], clean_p["mean_y"])      # y's own mean does not see x at all
    assert _same(grads["grad_x"][1:], clean_g["grad_x"][1:])
    if want_y:
        assert _same(grads["grad_y"][cdiv:], clean_g["grad_y"][cdiv:])
    near_r, near_2r = _near(H, W, i0, j0, r), _near(H, W, i0, j0, 2 * r)
    assert not torch.isfinite(planes["mean_x"][0][near_r]).any() and not torch.isfinite(planes["ve"][0][near_r]).any()
    for c in range(cdiv):
        assert not torch.isfinite(planes["A"][c][near_r]).any()
        assert not torch.isfinite(planes["out"][c][near_2r]).any() and not torch.isfinite(planes["mean_A"][c][near_2r]).any()
        if want_y:
            assert not torch.isfinite(grads["grad_y"][c][near_2r]).any()
    assert not torch.isfinite(grads["grad_x"][0][near_2r]).any()


@pytest.mark.parametrize("name", NAN_CASES)
def test_a_nan_in_y_and_grad_output_stays_in_its_plane(name):
    case = gb.CASES[name][0]
    B, Cx, Cy, H, W, r, want_y, Px, Py = _shape(case)
    cdiv = Py // Px
    x, y, g = gb.inputs(name, "uniform")
    clean_p, clean_g, _ = _hip(case, x, y, g, torch.float32)
    q = 1
    i0, j0 = H // 3, W // 2
    yn, gn = y.clone(), g.clone()
    yn[q, i0, j0] = float("nan")
    gn[q, i0 + 1, j0 - 1] = float("nan")
    planes, grads, names = _hip(case, x, yn, gn, torch.float32)
    _assert_route(name, names)
    others = [p for p in range(Py) if p != q]
    for key in ("mean_x", "ve"):
        assert _same(planes[key], clean_p[key]), key
    for key in ("mean_y", "A", "mean_A", "out"):
        assert _same(planes[key][others], clean_p[key][others]), key
    guide = q // cdiv
    other_x = [p for p in range(Px) if p != guide]
    assert _same(grads["grad_x"][other_x], clean_g["grad_x"][other_x])
    if want_y:
        assert _same(grads["grad_y"][others], clean_g["grad_y"][others])
    near_r, near_2r = _near(H, W, i0, j0, r), _near(H, W, i0, j0, 2 * r)
    assert not torch.isfinite(planes["mean_y"][q][near_r]).any() and not torch.isfinite(planes["A"][q][near_r]).any()
    assert not torch.isfinite(planes["out"][q][near_2r]).any()
    g_2r = _near(H, W, i0 + 1, j0 - 1, 2 * r)
    assert not torch.isfinite(grads["grad_x"][guide][g_2r]).any()
    if want_y:
        assert not torch.isfinite(grads["grad_y"][q][g_2r]).any()


# ------------------------------------------------------------------------------------------------ the C ABI
def _abi(case, family="uniform"):
    from ffwm_amd import _lib
    B, Cx, Cy, H, W, r, want_y, Px, Py = _shape(case)
    return _lib, _lib.load(), torch.cuda.current_stream(torch.device(DEV)).cuda_stream, (Px, Py, H, W, r)


def _fwd_general(lib, L, stream, dims, x, y, ws):
    Px, Py, H, W, r = dims
    out, saved = torch.empty_like(y), x.new_empty((2 * Px + 3 * Py) * H * W)
    L.check(lib.ffwm_guided_filter_forward_general(x.data_ptr(), y.data_ptr(), out.data_ptr(), saved.data_ptr(),
                                                   None if ws is None else ws.data_ptr(), Px, Py, H, W, r, gb.EPS, L.F32, stream),
            "ffwm_guided_filter_forward_general")
    return out, saved


def _bwd_general(lib, L, stream, dims, x, y, saved, g, ws, want_y):
    Px, Py, H, W, r = dims
    gx, gy = torch.empty_like(x), (torch.empty_like(y) if want_y else None)
    L.check(lib.ffwm_guided_filter_backward_general(x.data_ptr(), y.data_ptr(), saved.data_ptr(), g.data_ptr(), gx.data_ptr(),
                                                    None if gy is None else gy.data_ptr(), ws.data_ptr(), Px, Py, H, W, r, L.F32, stream),
            "ffwm_guided_filter_backward_general")
    return gx, gy


def test_workspace_contents_do_not_matter():
    name = "guide1_long_lines"
    case = gb.CASES[name][0]
    L, lib, stream, dims = _abi(case)
    Px, Py, H, W, r = dims
    x, y, g = (t.to(DEV) for t in gb.inputs(name, "uniform"))
    nbytes = lib.ffwm_guided_filter_workspace_bytes(Px, Py, H, W, L.F32, 1)
    assert nbytes == 4 * (Px + Py) * H * W * 4
    results = []
    with _profiled() as names:
        for fill in (float("nan"), 0.0):
            ws = torch.full((nbytes // 4,), fill, device=DEV)
            out, saved = _fwd_general(lib, L, stream, dims, x, y, ws)
            ws.fill_(fill)
            gx, gy = _bwd_general(lib, L, stream, dims, x, y, saved, g, ws, True)
            results.append((out, saved, gx, gy))
    assert _gf_names(names) == {"guided_filter_fwd_general", "guided_filter_bwd_general"}
    for a, b, what in zip(results[0], results[1], ("out", "saved", "grad_x", "grad_y")):
        assert torch.isfinite(a).all(), what
        assert torch.equal(a, b), what


def test_general_entry_points_hand_a_fast_shape_to_the_four_launch_kernels():
    name = "fast_ragged"
    case = gb.CASES[name][0]
    L, lib, stream, dims = _abi(case)
    Px, Py, H, W, r = dims
    x, y, g = (t.to(DEV) for t in gb.inputs(name, "uniform"))
    assert lib.ffwm_guided_filter_workspace_bytes(Px, Py, H, W, L.F32, 0) == 0
    out, saved = torch.empty_like(y), x.new_empty((5 * Py * H * W,))
    gx = torch.empty_like(x)
    ws = torch.full((lib.ffwm_guided_filter_workspace_bytes(Px, Py, H, W, L.F32, 1) // 4,), float("nan"), device=DEV)
    with _profiled() as names:
        L.check(lib.ffwm_guided_filter_forward(x.data_ptr(), y.data_ptr(), out.data_ptr(), saved.data_ptr(), Py, H, W, r, gb.EPS, L.F32,
                                               stream), "ffwm_guided_filter_forward")
        out_g, saved_g = _fwd_general(lib, L, stream, dims, x, y, None)           # NULL workspace allowed
        L.check(lib.ffwm_guided_filter_backward(x.data_ptr(), y.data_ptr(), saved.data_ptr(), g.data_ptr(), gx.data_ptr(), ws.data_ptr(),
                                                Py, H, W, r, L.F32, stream), "ffwm_guided_filter_backward")
        ws.fill_(float("nan"))
        gx_g, _ = _bwd_general(lib, L, stream, dims, x, y, saved, g, ws, False)   # grad_y = NULL
    assert _gf_names(names) == {"guided_filter_fwd", "guided_filter_bwd"}, sorted(names)
    assert torch.equal(out_g, out) and torch.equal(saved_g, saved) and torch.equal(gx_g, gx)
    assert torch.isfinite(out).all() and torch.isfinite(gx).all()
    with _profiled() as names:
        gx_y, gy = _bwd_general(lib, L, stream, dims, x, y, saved, g, ws, True)
    assert _gf_names(names) == {"guided_filter_bwd_general"}, sorted(names)
    # the general kernels from the four-launch kernels' saved planes: the same gradient within the backward's own bound
    bp = gb.Plan("general", r, gb.col_rows(Py, H, W))
    planes = gb.split_saved(saved.cpu(), Px, Py, H, W)
    ratios = gb.BackwardBound(bp, x.cpu(), y.cpu(), g.cpu(), planes).ratios({"grad_x": gx_y.cpu(), "grad_y": gy.cpu()})
    assert max(ratios.values()) <= 1.0, ratios
