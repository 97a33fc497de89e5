"""The yardstick of tests/correctness_bounds.py, checked without a GPU: the torch composition of the sampling-correctness loss
(losses.PerceptualCorrectness.calculate_loss over tests/torch_refs.warp, in the call's own dtype) meets every bound of every case,
so the bounds and the inputs are satisfiable by the reference alone; the conditions raise on inputs that break them; and the C ABI
exports the new entry points and checks their arguments before any launch."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import correctness_bounds as cb
import torch_refs


def _composition(case):
    """-> (loss, flow.grad, loss_map) of the composition on the CPU."""
    from ffwm_amd import losses
    B, C, Hi, Wi, H, W = case.dims
    pc = losses.PerceptualCorrectness(None, torch_refs.warp)
    pc.target_vgg, pc.source_vgg = {"x": case.target}, {"x": case.source}
    flow = case.flow.clone().requires_grad_(True)
    mask = None if case.mask is None else case.mask.reshape(B, 1, H, W)
    loss = pc.calculate_loss(flow, "x", mask, use_bilinear_sampling=True)
    loss.backward()
    with torch.no_grad():
        sample = torch_refs.warp(case.source, case.flow).reshape(B, C, -1)
        loss_map = torch.exp(-F.cosine_similarity(sample, case.target.reshape(B, C, -1)) / (case.corr_max + case.eps))
    return loss.detach(), flow.grad, loss_map


@pytest.mark.parametrize("spec", cb.cases(), ids=cb.case_id)
def test_torch_composition_meets_every_bound(spec):
    case = cb.build(spec)
    bound = cb.Bound(case, float_sums=True)
    loss, grad, loss_map = _composition(case)
    bound.check(loss_map=loss_map, what="composition")
    bound.check_module(loss, grad, what="composition")


def test_every_family_and_mask_is_covered_and_the_routes_are_what_the_shapes_are_for():
    specs = cb.cases()
    assert {s[1] for s in specs} == set(cb.FAMILIES) and {s[2] for s in specs} == set(cb.MASKS)
    want = {"c3": 1, "c64": 4, "c70_ragged": 4, "c256": 4, "c5_f64": 1, "c20_trips": 1, "c31": 1, "c32": 4, "c32_1024_blocks": 1}
    assert {n: cb.lane_slices(s) for n, s in cb.SHAPES.items()} == want


def test_outside_family_is_exactly_one_and_zero_in_the_reference():
    case = cb.make_case(cb.SHAPES["c3"], "outside", "none")
    bound = cb.Bound(case)
    assert bool(bound.outside.all())
    assert bool((bound.ref_map == 1).all()) and bool((bound.ref_grad == 0).all())


def test_all_zero_mask_gives_the_references_quotient():
    case = cb.make_case(cb.SHAPES["c3"], "random", "zero")
    bound = cb.Bound(case)
    assert bound.ref_out0 == (0.0 - case.e1) / (0.0 + case.eps) and bound.ref_out1 == case.eps


def test_conditions_raise_on_bad_inputs():
    shape = cb.SHAPES["c3"]
    B, C, Hi, Wi, H, W = shape
    case = cb.make_case(shape, "random")
    case.flow[0, 0, 2, 3] = (2 * 2.0 + 1) / Wi - 1              # px = 2 exactly: on the kink of the bilinear interpolant
    with pytest.raises(ValueError, match="fractional"):
        cb.Bound(case)
    case = cb.make_case(shape, "random")
    case.source.zero_()                                          # in range, but S = 0: neither outside nor sqrt(S) >= 1e-4
    case.corr_max = torch.full_like(case.corr_max, 0.5)
    with pytest.raises(ValueError, match="neither"):
        cb.Bound(case)
    case = cb.make_case(shape, "random")
    case.corr_max[0, 0] = 0.1
    with pytest.raises(ValueError, match="corr_max"):
        cb.Bound(case)


def test_a_wrong_output_misses_the_bound():
    case = cb.make_case(cb.SHAPES["c3"], "random", "binary")
    bound = cb.Bound(case)
    loss, grad, loss_map = _composition(case)
    wrong = loss_map.clone()
    wrong[0, 5] *= 1 + 2.0 ** -12
    with pytest.raises(AssertionError):
        bound.check(loss_map=wrong, verbose=False)
    with pytest.raises(AssertionError):
        bound.check_module(loss, grad * (1 + 2.0 ** -10), verbose=False)


# ------------------------------------------------------------------------------------------------ the C ABI, no device touched
@pytest.fixture(scope="module")
def hiplib():
    from ffwm_amd import build, _lib
    build.build()
    return _lib.load()


NEW = ("ffwm_sampling_correctness", "ffwm_sampling_correctness_workspace_bytes")


def test_library_exports_the_new_symbols(hiplib):
    from ffwm_amd import _lib
    for n in NEW:
        assert hasattr(hiplib, n) and n in _lib.EXPORTS
    assert hiplib.ffwm_sampling_correctness_workspace_bytes.restype is ctypes.c_int64
    assert hiplib.ffwm_abi_version() == 5


def test_workspace_query(hiplib):
    ws = hiplib.ffwm_sampling_correctness_workspace_bytes
    for (B, H, W) in ((1, 1, 1), (2, 5, 7), (6, 128, 128)):
        for dtype in (0, 1):
            assert ws(B, H, W, dtype) == 16 * B * ((H * W + 15) // 16)           # two doubles per 16-pixel block
    assert ws(0, 4, 4, 0) == -1 and ws(1, 0, 4, 0) == -1 and ws(1, 4, -1, 0) == -1
    assert ws(1, 4, 4, 7) == -2 and b"dtype" in hiplib.ffwm_last_error()
    assert ws(1, 1 << 15, 1 << 15, 0) == -3


def test_argument_errors_are_reported_before_launch(hiplib):
    fn = hiplib.ffwm_sampling_correctness
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(source=p, target=p, flow=p, cm=p, mask=None, lmap=None, grad=None, out=p, ws=p, dims=(1, 2, 4, 4, 4, 4), dtype=0):
        return fn(source, target, flow, cm, mask, lmap, grad, out, ws, *dims, 0.36787944117144233, 1e-8, dtype, None)
    for missing in ("source", "target", "flow", "cm", "out"):
        assert call(**{missing: None}) == -1 and b"NULL" in hiplib.ffwm_last_error()
    assert call(ws=None) == -1 and b"workspace" in hiplib.ffwm_last_error()
    assert call(dtype=5) == -2 and b"dtype" in hiplib.ffwm_last_error()
    for bad in ((0, 2, 4, 4, 4, 4), (1, 0, 4, 4, 4, 4), (1, 2, 0, 4, 4, 4), (1, 2, 4, 4, 4, 0)):
        assert call(dims=bad) == -1
    assert call(dims=(1, 2, 1 << 15, 1 << 15, 4, 4)) == -3
    assert call(dims=(1, 2, 4, 4, 1 << 14, 1 << 14)) == -3
    assert call(dims=(1, 1 << 20, 64, 64, 4, 4)) == -3 and b"4 GiB" in hiplib.ffwm_last_error()
    assert call(dims=(1, 1 << 19, 64, 64, 4, 4), dtype=1) == -3


def test_op_wrapper_refuses_cpu_tensors_and_bad_shapes():
    from ffwm_amd import ops
    case = cb.make_case(cb.SHAPES["c3"], "random")
    with pytest.raises(NotImplementedError):
        ops.sampling_correctness(case.source, case.target, case.flow, case.corr_max, None, 1e-8, True)


def test_fused_switch_defaults_off_and_falls_back_to_the_composition_on_the_cpu():
    from ffwm_amd import losses
    assert losses.PerceptualCorrectness(None, torch_refs.warp).fused is False
    case = cb.make_case(cb.SHAPES["c3"], "random", "binary")
    B, C, Hi, Wi, H, W = case.dims
    got = []
    for fused in (False, True):
        pc = losses.PerceptualCorrectness(None, torch_refs.warp, fused=fused)
        pc.target_vgg, pc.source_vgg = {"x": case.target}, {"x": case.source}
        got.append(pc.calculate_loss(case.flow, "x", case.mask.reshape(B, 1, H, W), use_bilinear_sampling=True))
    assert torch.equal(got[0], got[1])
