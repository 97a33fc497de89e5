"""The guided-filter bounds of tests/guided_filter_bounds.py judged without a GPU: the restated route picks the chunk heights the
case table claims; the closed-form backward is autograd's; the fp32 stand-ins (the cumsum restatement of ffwm_amd.nets.GuidedFilter,
the sliding-window emulation, the cumsum-difference emulation of the four-launch kernels) meet every bound with SAFETY = 1 and the
integer family bit for bit; every mutant of the emulation misses an assertion at the full SAFETY = 4; the conditions raise on inputs
built to violate them.  rc is handed to the emulation, so the shapes here are smaller than the GPU ones."""
import pytest
import torch

import guided_filter_bounds as gb

# (B, Cx, Cy, H, W, r, want_y), rc for the emulation (None: the fast route)
SMALL = {
    "fast": ((1, 2, 2, 37, 61, 5, False), None),
    "general_two_row_chunks": ((1, 2, 2, 70, 300, 9, True), 32),
    "general_guide1": ((2, 1, 3, 40, 70, 4, True), 16),
    "general_window_over_chunks": ((1, 1, 1, 50, 75, 20, True), 8),
}


def _plans(name):
    case, rc = SMALL[name]
    if rc is None:
        return case, gb.Plan("fast", case[5]), gb.Plan("fast", case[5])
    return case, gb.Plan("general", case[5], rc), gb.Plan("general", case[5], rc)


def _nets_box(r):
    from ffwm_amd import nets
    gf = nets.GuidedFilter(r)
    return lambda v: gf.box(v.unsqueeze(0))[0]


def _run(name, family, dtype, mutant=None, safety=gb.SAFETY, box=None):
    """-> ({plane: error / bound} of the forward and the backward, the stand-in's planes)."""
    case, fp, bp = _plans(name)
    x, y, g = (t.to(dtype) for t in gb.flat(case, gb.make_inputs(case, family)))
    if box is None:
        fwd = gb.emulate_forward(fp, x, y, mutant=mutant)
    else:
        fwd = gb.forward_formulas(box, x, y, case[5], gb.EPS)
    ratios = gb.ForwardBound(fp, x, y, safety=safety).ratios(fwd)
    saved = {k: fwd[k] for k in ("mean_x", "mean_y", "A", "ve", "mean_A")}
    if mutant in (None, "gvar_sign"):            # a backward from wrong saved planes has no reference to meet
        bwd = gb.emulate_backward(bp, x, y, g, saved, mutant=mutant) if box is None else gb.backward_formulas(box, x, y, g, saved, case[5])
        ratios.update(gb.BackwardBound(bp, x, y, g, saved, safety=safety).ratios(bwd))
    return ratios, fwd


def test_the_restated_route_gives_every_case_of_the_table_its_chunk_height():
    seen = set()
    for name, (case, fwd, bwd, rc) in gb.CASES.items():
        B, Cx, Cy, H, W, r, want_y = case
        assert gb.col_rows(B * Cy, H, W) == rc, name
        fp, bp = gb.plans(case)
        assert (fp.kind, bp.kind) == (fwd, bwd), name
        assert H > 2 * r + 1 and W > 2 * r + 1
        if bwd == "general":
            seen.add(rc)
    assert seen == {32, 64, 128}
    assert gb.col_rows(24, 512, 512) == 64 and gb.col_rows(3, 512, 512) == 32 and gb.col_rows(192, 130, 65) == 64
    assert gb.col_rows(256, 130, 65) == 128 and gb.col_rows(255, 130, 65) == 64
    assert gb.route(3, 3, 128, 128, False) == "fast" and gb.route(3, 3, 128, 128, True) == "general"
    assert gb.route(3, 3, 129, 128, False) == "general" and gb.route(1, 3, 64, 64, False) == "general"
    # the properties the note column of the table promises
    assert 2 * gb.CASES["general_long_window"][0][5] + 1 > gb.ROW_CHUNK
    assert 130 % 64 == 2 and 130 % 128 == 2 and 65 % 64 == 1 and 260 % gb.ROW_CHUNK == 4 and 33 % 32 == 1


@pytest.mark.parametrize("name", ["fast", "general_guide1"])
def test_closed_form_is_autograd_of_the_restatement(name):
    from ffwm_amd import nets
    case = SMALL[name][0]
    B, Cx, Cy, H, W, r, _ = case
    x4, y4, g4 = (t.double() for t in gb.make_inputs(case, "uniform"))
    xr, yr = x4.clone().requires_grad_(True), y4.clone().requires_grad_(True)
    out = nets.GuidedFilter(r)(xr, yr)
    out.backward(g4)
    x, y, g = gb.flat(case, (x4, y4, g4))
    fwd = gb.forward_formulas(lambda v: gb.box64(v, r), x, y, r, gb.EPS)
    bwd = gb.backward_formulas(lambda v: gb.box64(v, r), x, y, g, fwd, r)
    for got, ref in ((fwd["out"], out.detach()), (bwd["grad_x"], xr.grad), (bwd["grad_y"], yr.grad)):
        ref = ref.reshape(got.shape)
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", gb.FAMILIES)
@pytest.mark.parametrize("name", sorted(SMALL))
def test_emulation_meets_every_bound_at_safety_1(name, family, dtype):
    ratios, _ = _run(name, family, dtype, safety=1.0)
    print("GFBOUND cpu %s %s: %s" % (name, family, " ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
    assert len(ratios) == 8 and max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("family", gb.FAMILIES)
def test_float32_restatement_meets_the_fast_bounds_at_safety_1(family):
    """ffwm_amd.nets.GuidedFilter's box (full-length cumsums) in float32, on the route whose bound is a cumsum's."""
    ratios, _ = _run("fast", family, torch.float32, safety=1.0, box=_nets_box(SMALL["fast"][0][5]))
    assert len(ratios) == 8 and max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("name", sorted(SMALL))
def test_integer_family_is_exact_in_the_emulation(name):
    case, fp, _ = _plans(name)
    x, y, _ = gb.flat(case, gb.make_inputs(case, "integers"))
    mx, my = gb.exact_means(x, y, case[5], fp.kind == "fast")
    fwd = gb.emulate_forward(fp, x, y)
    assert torch.equal(fwd["mean_x"], mx) and torch.equal(fwd["mean_y"], my)
    if fp.kind == "fast":
        box = _nets_box(case[5])
        n = gb.box_count(case[3], case[4], case[5], torch.float32)
        assert torch.equal(box(x) / n, mx) and torch.equal(box(y) / n, my)


def _misses(name, mutant):
    """The assertions a mutant misses: bounds at SAFETY = 4 in float32 and float64, and the exact integer means."""
    missed = []
    for dtype in (torch.float32, torch.float64):
        ratios, _ = _run(name, "uniform", dtype, mutant=mutant)
        missed += ["%s/%s" % (k, str(dtype)[-7:]) for k, v in ratios.items() if not v <= 1.0]
    case, fp, _ = _plans(name)
    x, y, _ = gb.flat(case, gb.make_inputs(case, "integers"))
    mx, my = gb.exact_means(x, y, case[5], fp.kind == "fast")
    fwd = gb.emulate_forward(fp, x, y, mutant=mutant)
    missed += [k for k, ref in (("mean_x/exact", mx), ("mean_y/exact", my)) if not torch.equal(fwd[k.split("/")[0]], ref)]
    return missed


def test_the_unmutated_emulation_misses_nothing():
    for name in ("general_guide1", "fast"):
        assert _misses(name, None) == []


@pytest.mark.parametrize("mutant,name,expect", [
    ("hi_off_by_one", "general_guide1", "mean_x/exact"),
    ("hi_off_by_one", "fast", "mean_x/exact"),
    ("seed_short", "general_guide1", "mean_x/exact"),
    ("unclipped_n", "general_guide1", "mean_y/exact"),
    ("eps_dropped", "general_guide1", "ve/float64"),
    ("guide_plane_mod", "general_guide1", "A/float32"),
    ("gvar_sign", "general_guide1", "grad_x/float32"),
])
def test_mutants_miss_an_assertion(mutant, name, expect):
    missed = _misses(name, mutant)
    print("GFBOUND mutant %s on %s misses: %s" % (mutant, name, " ".join(missed)))
    assert expect in missed, missed


def test_seed_short_is_seen_by_the_bounds_too():
    ratios, _ = _run("general_window_over_chunks", "uniform", torch.float32, mutant="seed_short")
    assert ratios["mean_x"] > 1.0 and ratios["out"] > 1.0


def test_drift_of_a_sum_that_is_never_reseeded():
    """A dense patch on a long line: past the patch the kernel's sums are exactly zero (a chunk reseeds from zeros), and the bound
    there is zero; a running sum that is never reseeded keeps its rounding residue."""
    H, W, r, rc = 600, 8, 3, 32
    gen = torch.Generator().manual_seed(5)
    v = torch.zeros(1, H, W)
    v[:, 20:60] = torch.rand(1, 40, W, generator=gen) * 100
    plan = gb.Plan("general", r, rc)
    ref = gb.box64(v.double(), r)
    bound = gb.box_err(plan, v.double().abs(), 0.0, gb.SAFETY * gb.U32)
    assert float(bound[:, 128:].max()) == 0.0 and float(bound[:, 20:60].min()) > 0.0
    good = gb.emu_box(plan, v)
    assert gb.worst_ratio(good, ref, bound) <= 1.0 and float(good[:, 128:].abs().max()) == 0.0
    drift = gb.emu_box(plan, v, mutant="no_reseed")
    assert float(drift[:, 128:].abs().max()) > 0.0, "no residue: the mutant does not drift on this input"
    assert gb.worst_ratio(drift, ref, bound) > 1.0


def test_the_conditions_raise():
    gen = torch.Generator().manual_seed(3)
    big = torch.floor(torch.rand(1, 64, 64, generator=gen) * 4096)
    with pytest.raises(ValueError, match="2\\^24"):
        gb.require_exact(big, big, 8, False)
    with pytest.raises(ValueError, match="integer"):
        gb.require_exact(big + 0.5, big, 8, False)
    line = torch.full((1, 128, 128), 45.0)                 # every window below 2^24, the fast route's cumsum not
    gb.require_exact(line, line, 40, False)
    with pytest.raises(ValueError, match="2\\^24"):
        gb.require_exact(line, line, 40, True)
    x = 1000.0 + 1e-3 * torch.rand(1, 40, 40, generator=gen)
    y = torch.rand(1, 40, 40, generator=gen)
    with pytest.raises(ValueError, match="first-order"):
        gb.ForwardBound(gb.Plan("general", 4, 32), x, y)
    gb.ForwardBound(gb.Plan("general", 4, 32), x - 1000.0 + torch.rand(1, 40, 40, generator=gen), y)


def test_every_gpu_case_meets_the_ve_condition_on_the_reference_alone():
    """The families' amplitudes (module docstring of guided_filter_bounds) against the largest case of each route."""
    for name in ("fast_full_line", "fast_odd_strip", "general_rc128", "general_rc128_guide1"):
        for family in ("image", "offset"):
            assert gb.forward_bound(name, family, torch.float32).ve_condition <= 1.0
