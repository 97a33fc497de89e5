"""tests/bn_bounds.py judged without a GPU.  Two fp32 stand-ins -- ATen's CPU kernels (native_batch_norm + leaky_relu / sigmoid and
their backward functions) and a torch restatement of the kernel's own arithmetic (double sums, x sc + sh) -- meet every bound with
SAFETY = 1 on every shape, configuration and family of the GPU matrix, and the exact family bit for bit: the reference alone stays
inside its conditions (among them: zero elements within the fp32 margin of the activation's kink, asserted by BackwardBound).  Eight
mutants of the restatement each miss a bound somewhere in the matrix.  bn_route is checked at its thresholds."""
import pytest
import torch

import bn_bounds as bb


def _aten_forward(case):
    rm = None if case.run_mean is None else case.run_mean.clone()
    rv = None if case.run_var is None else case.run_var.clone()
    out, save_mean, save_invstd = torch.native_batch_norm(case.x, case.gamma, case.beta, rm, rv, True, case.momentum, case.eps)
    if case.res is not None:
        out = out + (case.res + case.rbias.view(1, -1, 1, 1))
    y = torch.sigmoid(out) if case.act == 1 else torch.nn.functional.leaky_relu(out, case.slope)
    return y, save_mean, save_invstd, rm, rv


def _aten_backward(bc):
    C = bc.x.shape[1]
    if bc.variant == "plain":
        ga = bc.gamma if bc.gamma is not None else torch.ones(C)
        be = bc.beta if bc.beta is not None else torch.zeros(C)
        pre = (bc.x - bc.save_mean.view(1, -1, 1, 1)) * bc.save_invstd.view(1, -1, 1, 1) * ga.view(1, -1, 1, 1) + be.view(1, -1, 1, 1)
        g = torch.ops.aten.leaky_relu_backward(bc.dy, pre, bc.slope, False)
    elif bc.act == 1:
        g = torch.ops.aten.sigmoid_backward(bc.dy, bc.y)
    else:
        g = torch.ops.aten.leaky_relu_backward(bc.dy, bc.y, bc.slope, True)
    dx, dw, db = torch.ops.aten.native_batch_norm_backward(g, bc.x, bc.gamma, None, None, bc.save_mean, bc.save_invstd, True, bc.eps, [True, True, True])
    if dw is None or bc.gamma is None:
        xhat = (bc.x - bc.save_mean.view(1, -1, 1, 1)) * bc.save_invstd.view(1, -1, 1, 1)
        dw = (g.double() * xhat.double()).sum((0, 2, 3)).float()
    return dx, dw, db, (g if bc.variant == "res" else None)


def _both_directions(case, route, forward, backward, safety, exact_dx=False, verbose=False, float_sums=False):
    """Forward stand-in against ForwardBound; then the backward stand-in on the reference's own float statistics and output."""
    fb = bb.ForwardBound(case, route, safety)
    fb.check(*forward(case), verbose=verbose)
    bc = bb.backward_inputs(case, fb.mean.float(), fb.invstd.float(), fb.ref.float() if case.variant == "res" else None)
    bwd = bb.BackwardBound(bc, route, safety, float_sums=float_sums)
    if not case.exact and case.variant == "plain":
        assert bwd.ambiguous == 0
    bwd.check(*backward(bc), exact_dx=exact_dx, verbose=verbose)


@pytest.mark.parametrize("spec", bb.mixed_cases(), ids=bb.case_id)
def test_standins_meet_every_bound_without_the_safety_factor(spec):
    case, route = bb.build_mixed(spec, huge_exp=30)              # (ATen's fp32 sums of squares overflow at 2^60)
    _both_directions(case, route, _aten_forward, _aten_backward, 1.0, float_sums=True)
    case, route = bb.build_mixed(spec)
    _both_directions(case, route, lambda c: bb.emulate_forward(c, route), lambda c: bb.emulate_backward(c, route), 1.0)


@pytest.mark.parametrize("spec", bb.exact_cases(), ids=lambda s: "-".join(str(v) for v in s))
def test_standins_meet_the_exact_family_bit_for_bit(spec):
    case, route = bb.build_exact(spec)
    _both_directions(case, route, lambda c: bb.emulate_forward(c, route), lambda c: bb.emulate_backward(c, route), 1.0, exact_dx=spec[-1])
    _both_directions(case, route, _aten_forward, _aten_backward, 1.0, exact_dx=False)


def test_exact_family_refuses_what_it_cannot_prove():
    with pytest.raises(ValueError):
        bb.make_exact_case((3, 37, 5, 7))                          # 105 values per channel cannot be balanced
    with pytest.raises(ValueError):
        bb.require_exact(torch.tensor([1.0 / 3.0], dtype=torch.float64))
    case, route = bb.build_exact(("wave_rounds_ragged", "plain", 0.25, 0.5, False))       # n = 2044: mean(g) = k / 2044 is no float
    fb = bb.ForwardBound(case, route)
    bwd = bb.BackwardBound(bb.backward_inputs(case, fb.mean.float(), fb.invstd.float()), route)
    with pytest.raises(ValueError):
        bwd.require_exact_dx()


def test_ill_conditioned_statistics_are_refused():
    """mean = 2^20 std: the double sums' own error would exceed one float rounding of the output."""
    case, route = bb.build_mixed(("block_ragged2", "plain", "a", 0, False))
    case.x[:, 0] = torch.randn(case.x[:, 0].shape) * 2.0 ** -12 + 2.0 ** 14
    with pytest.raises(ValueError):
        bb.ForwardBound(case, route)


# ------------------------------------------------------------------------------------------------ mutants
def _fails(case, route, mutant):
    try:
        _both_directions(case, route, lambda c: bb.emulate_forward(c, route, mutant), lambda c: bb.emulate_backward(c, route, mutant), bb.SAFETY)
    except AssertionError as e:
        return str(e)
    return None


MUTANT_CASES = {
    "fp32_variance": [("block_ragged1", "plain", "a", 0, False), ("split_s2", "plain", "a", 0, False)],
    "first_slice_only": [("split_s2", "plain", "a", 0, False), ("split_s32", "res_lrelu", "a", 0, False)],
    "ragged_group_skipped": [("block_ragged1", "plain", "a", 0, False), ("wave_rounds_ragged", "plain", "a", 0, False), ("split_odd_float4", "plain", "a", 0, False)],
    "biased_running_var": [("split_s2", "plain", "b", 0, False), ("block_scalar", "res_lrelu", "a", 0, False), ("wave_n2", "plain", "b", 0, False)],
    "rbias_dropped": [("wave_scalar_dead11", "res_lrelu", "a", 0, False), ("block_2048", "res_sigmoid", "a", 0, False)],
    "mask_from_x": [("wave_scalar_dead11", "plain", "a", 0, False), ("split_s3", "plain", "b", 0, False)],
    "uncentred_dgamma": [("block_scalar", "plain", "a", 0, False), ("block_scalar", "res_lrelu", "a", 0, False)],
    "dead_subgroup_store": [("wave_scalar_dead11", "plain", "a", 0, False), ("wave_1030", "res_lrelu", "a", 0, False)],
}


@pytest.mark.parametrize("mutant", bb.MUTANTS)
def test_every_mutant_misses_a_bound(mutant):
    """... at the FULL bound (SAFETY = 4), on every case listed for it, while the unmutated restatement passes the same cases."""
    for spec in MUTANT_CASES[mutant]:
        case, route = bb.build_mixed(spec)
        assert _fails(case, route, None) is None, spec
        why = _fails(case, route, mutant)
        assert why is not None, "%s passed %s" % (mutant, bb.case_id(spec))
        print(mutant, bb.case_id(spec), "->", why[:200])


def test_mutants_that_need_a_route_are_harmless_elsewhere():
    """The mutants are restatements of real slips, not noise: without slices / a ragged row / dead sub-groups they change nothing."""
    case, route = bb.make_case((1, 3, 64, 64)), bb.bn_route(1, 3, 64 * 64, False)          # one slice, 1024 float4: no ragged row, no dead
    assert (route.kind, route.all4 % route.threads, route.dead) == ("block", 0, 0)
    for mutant in ("first_slice_only", "ragged_group_skipped", "dead_subgroup_store"):
        assert _fails(case, route, mutant) is None, mutant


def test_fp32_variance_is_rejected_at_a_mean_of_256_std_by_a_wide_margin():
    case, route = bb.build_mixed(("block_ragged1", "plain", "a", 0, False))
    fb = bb.ForwardBound(case, route)
    _, _, invstd, _, _ = bb.emulate_forward(case, route, "fp32_variance")
    c = case.families.index("offset")
    ratio = float((invstd[c].double() - fb.invstd[c]).abs() / fb.invstd_bound[c])
    assert ratio > 100, ratio
    _, _, good, _, _ = bb.emulate_forward(case, route)
    assert float((good[c].double() - fb.invstd[c]).abs() / fb.invstd_bound[c]) <= 1


# ------------------------------------------------------------------------------------------------ the route
def test_route_thresholds():
    r = bb.bn_route
    assert r(1, 3, 2047, False).kind == "wave" and r(1, 3, 2047, False).threads == 64 and not r(1, 3, 2047, False).vec
    assert r(1, 3, 2048, False).kind == "block" and r(1, 3, 2048, False).threads == 1024 and r(1, 3, 2048, False).vec
    assert r(1, 3, 2047, True).S == 1 and r(1, 3, 2048, True).S == 1
    # HW % 4: no split without the float4 path, however large
    assert r(3, 2, 128 * 128 + 1, True).kind == "block" and r(3, 2, 128 * 128 + 2, True).S == 1 and r(3, 2, 128 * 128 + 4, True).S == 3
    # B HW / 16384 = 1, 2, 32
    assert r(1, 1, 16384, True).kind == "block" and r(1, 1, 32764, True).S == 1
    assert r(1, 1, 32768, True).S == 2 and r(2, 1, 16384, True).S == 2 and r(1, 1, 49148, True).S == 2
    assert r(2, 1, 512 * 512, True).S == 32 and r(4, 1, 512 * 512, True).S == 32 and r(1, 1, 31 * 16384, True).S == 31
    # C against ceil(1024 / C)
    big = (8, 512 * 512)
    assert [r(big[0], C, big[1], True).S for C in (1, 32, 33, 64, 100, 341, 342, 511, 512, 513, 1024)] == [32, 32, 32, 16, 11, 4, 3, 3, 2, 2, 1]
    assert r(8, 1025, 512 * 512, True).kind == "block"
    assert r(2, 3, 128 * 128, False).S == 1                                              # no scratch, no split


def test_route_slices_and_chains():
    r = bb.bn_route(3, 4, 108 * 104, True)
    assert r.kind == "split" and r.slices == [(0, 4212), (4212, 8424)] and r.hw4 == 2808      # the boundary lies inside plane 1
    r = bb.bn_route(1, 2, 12 * 2731, True)
    assert r.slices == [(0, 4097), (4097, 8193)]                                             # an odd float4 count, unequal slices
    assert r.L_fwd == 16 * 2 and r.L_bwd == 8 * 3 and r.P == 64 + 16 + 2
    r = bb.bn_route(3, 37, 35, False)
    assert (r.kind, r.path, r.dead, r.blocks, r.L_fwd, r.P) == ("wave", "scalar", 11, 3, 3, 64)
    r = bb.bn_route(8, 1030, 4, False)
    assert (r.kind, r.path, r.dead, r.all4, r.L_fwd) == ("wave", "float4", 10, 8, 16)
    r = bb.bn_route(5, 2, 64 * 68, False)
    assert (r.kind, r.path, r.all4, r.L_fwd, r.L_bwd, r.P) == ("block", "float4", 5440, 32, 24, 80)
    for name in bb.SHAPES:
        route = bb.route_of(name)
        assert sum(t - f for f, t in route.slices) == route.all4 and all(t > f for f, t in route.slices) or not route.vec
    assert bb.scratch_doubles(3) == 8 and bb.scratch_doubles(4) == 10


def test_every_family_and_sign_of_gamma_reaches_every_shape():
    seen = {}
    for spec in bb.mixed_cases():
        case_families = seen.setdefault(spec[0], set())
        C = bb.SHAPES[spec[0]][0][1]
        case_families.update(bb.FAMILIES[(c + spec[3]) % 5] for c in range(C))
    assert all(v == set(bb.FAMILIES) for v in seen.values()), seen
    case, _ = bb.build_mixed(("wave_scalar_dead11", "plain", "a", 0, False))
    g, b = case.gamma, case.beta
    assert bool((g > 0).any()) and bool((g < 0).any()) and bool(((g == 0) & (b == 0)).any()) and bool(((g == 0) & (b != 0)).any())
