"""The per-pixel yardstick of tests/gather_bounds.py, checked on the CPU at the shapes of tests/test_gpu_gather_bounds.py:

  * every float64 restatement (the source of `mag`) reproduces the float64 oracle to 64 u64 mag (measured: <= 17);
  * the float32 oracle -- the reference's own arithmetic, one running sum over taps x C terms -- meets every bound at
    rho / SAFETY, on every family, grid family and operator;
  * seven mutants of a float32 stand-in fail it, among them one the suite's global bound ``tol (1 + max|ref|)`` accepts.

Worst error / bound of the float32 oracle at rho / SAFETY (the bound is a worst-case one over n = taps x C terms, so the
reference sits far inside it where n is large; where kappa leads -- warp on sizes that are no power of two -- it sits closest):

    operator / output             worst ratio   where
    resample2d d_input2           0.15          C = 5, ks 2, group_mags
    block extractor d_flow        0.055         k = 2, C = 3, masked
    block attention d_flow        0.032         C = 6, group_mags
    block attention d_weights     0.18          C = 6, feat_mags
    warp d_flow                   0.58          in [1, 3, 96, 130] -> grid 80 x 129, border grid, masked (kappa leads)
"""
import pytest
import torch

import gather_bounds as gb
import scatter_bounds as sb

U64 = 2.0 ** -53


def _restated(bound, what):
    q = (bound.signed - bound.ref).abs() / (64 * U64 * bound.mag + gb.FLOOR)
    assert float(q.max()) <= 1.0, "%s: restatement off the float64 oracle by %.3g x 64 u64 mag" % (what, float(q.max()))


def _as_f32(bound):
    """The bound of a float32 implementation of the same case (the float64 cases carry u64 in kappa)."""
    scale = sb.unit_roundoff(torch.float32) / sb.unit_roundoff(bound.dtype)
    return gb.Bound(bound.ref, bound.mag, bound.kappa * scale, bound.units, torch.float32, bound.signed)


def _f32(*ts):
    """Float32 COPIES: the cached cases stay as they were built."""
    return [t.to(torch.float32, copy=True).contiguous() for t in ts]


# ------------------------------------------------------------------------------------------------ restatement + reference
@pytest.mark.parametrize("kind", gb.FAMILIES)
@pytest.mark.parametrize("name", list(gb.RS_CASES))
def test_resample2d_restatement_and_reference(oracle, name, kind):
    in1, in2, go, bound = gb.rs_case(name, kind)
    ks, dil = gb.RS_CASES[name][2:4]
    _restated(bound, "resample2d %s %s" % (name, kind))
    _, got = oracle.resample2d_backward(*_f32(in1, in2, go), ks, dil)
    _as_f32(bound).check(got, bound.units / gb.SAFETY, "fp32 oracle, resample2d %s %s" % (name, kind))


@pytest.mark.parametrize("kind", gb.FAMILIES)
@pytest.mark.parametrize("name", list(gb.BE_CASES))
def test_block_extractor_restatement_and_reference(oracle, name, kind):
    src, flow, go, k, bound = gb.be_case(name, kind)
    _restated(bound, "block extractor %s %s" % (name, kind))
    _, got = oracle.block_extractor_backward(*_f32(src, flow, go), k)
    _as_f32(bound).check(got, bound.units / gb.SAFETY, "fp32 oracle, block extractor %s %s" % (name, kind))


@pytest.mark.parametrize("kind", gb.FAMILIES)
@pytest.mark.parametrize("name", list(gb.BA_CASES))
def test_block_attention_restatement_and_reference(oracle, name, kind):
    src, flow, w, go, flow_bound, weights_bound = gb.ba_case(name, kind)
    _restated(flow_bound, "block attention %s %s" % (name, kind))
    s32, f32 = _f32(src, flow)
    _, gf = oracle.block_extractor_backward(s32, f32, sb.attention_extractor_grad(w, go, 3).float(), 3)
    gpool = (go.float() / 9).repeat_interleave(3, 2).repeat_interleave(3, 3)
    gw = oracle.local_attn_reshape_backward((gpool * oracle.block_extractor_forward(s32, f32, 3)).sum(1, keepdim=True).contiguous(), 3)
    _as_f32(flow_bound).check(gf, flow_bound.units / gb.SAFETY, "fp32 oracle, block attention d_flow %s %s" % (name, kind))
    _as_f32(weights_bound).check(gw, weights_bound.units / gb.SAFETY, "fp32 oracle, block attention d_weights %s %s" % (name, kind))


WARP_ROWS = [(name,) + row for name in gb.WARP_CASES for row in gb.warp_matrix(name)]


@pytest.mark.parametrize("name,grid_kind,kind,flipcat", WARP_ROWS)
def test_warp_restatement_and_reference(oracle, name, grid_kind, kind, flipcat):
    feat, grid, go, bound = gb.warp_case(name, grid_kind, kind, flipcat)
    what = "warp %s %s %s flipcat %d" % (name, grid_kind, kind, flipcat)
    _restated(bound, what)
    _, got = oracle.warp_backward(*_f32(feat, grid, go), flipcat)
    _as_f32(bound).check(got, bound.units / gb.SAFETY, "fp32 oracle, " + what)
    if grid_kind == "outside":         # bands of pixels with four invalid corners: exactly 0, and the bound leaves them no slack
        dead = bound.mag == 0
        assert int(dead.sum()) > 0 and float((bound.mag + bound.kappa)[dead].max()) == 0.0 and float(got[dead].abs().max()) == 0.0


def test_interior_grid_keeps_every_corner_inside_and_outside_grid_has_dead_bands():
    """What the grid families are for: `interior` gives whole waves whole rows (the pair-load arm of the multi-problem kernel),
    `outside` pixels without a valid corner, and every sample is an odd multiple of 2^-9 (2^-9 from the nearest cell edge)."""
    Hi, Wi = 64, 192
    for kind in gb.WARP_GRIDS:
        grid = gb.warp_grid(kind, 2, (Hi, Wi), (Hi, Wi), 161).double()
        ix, iy = ((grid[:, 0] + 1) * Wi - 1) / 2, ((grid[:, 1] + 1) * Hi - 1) / 2
        for v in (ix, iy):
            n = torch.round(v * 512)                         # (the float32 grid moves a sample by ~1e-5 px where the size is no power of two)
            assert float((v * 512 - n).abs().max()) < 1e-2 and bool((n.long() % 2 == 1).all())
        inside = (ix > 0) & (ix < Wi - 1) & (iy > 0) & (iy < Hi - 1)
        dead = (ix < -1) | (ix > Wi) | (iy < -1) | (iy > Hi)
        assert bool(inside.all()) == (kind == "interior")
        assert (int(dead.sum()) > 1000) == (kind == "outside")


LDS_CASES = ("b2c5_64", "ragged_w", "grids", "slabs", "c2_66", "natural")     # what test_gpu_gather_bounds.py sends to the LDS kernel


def test_warp_lds_cases_leave_lds_only_under_zoom25():
    """The profiler scope cannot tell the LDS arm of warp_bwd_flow_lds_kernel from its direct-gather arm, so the inputs are
    proven here: under zoom25 some tiles' boxes exceed 128 x 32 cells (direct gathers) while others of the same launch stay in
    LDS; every other grid of the LDS cases -- zoom 1.8 too: 16 rows span at most 30 cells -- keeps every tile in LDS."""
    for name in LDS_CASES:
        (B, C, Hi, Wi), grid_hw, _ = gb.WARP_CASES[name]
        for grid_kind in sorted({row[0] for row in gb.warp_matrix(name)}):
            boxes = gb.warp_lds_boxes(gb.warp_grid(grid_kind, B, (Hi, Wi), grid_hw or (Hi, Wi), 161), (Hi, Wi))
            direct = sum(1 for bw, bh in boxes if bw > 128 or bh > 32)
            if grid_kind == "zoom25":
                assert 0 < direct < sum(1 for bw, bh in boxes if bw > 0), (name, boxes)
            else:
                assert direct == 0 and max(bw for bw, _ in boxes) > 0, (name, grid_kind, boxes)


def test_warp_pixel_kernel_slabs():
    """Which loops of warp_bwd_body a case runs follows from its slab: [4, 20, 256, 256] keeps 5 channels per block (1024 tiles:
    20 -> 10 gives 2048 blocks, 10 -> 5 gives 4096) -- one four-channel trip, pair loads in the multi launch, and one channel for
    the tail loop; every other pixel-kernel case is cut down to one channel per block and runs the tail loop alone."""
    def slab(name):
        (B, C, Hi, Wi), grid_hw, _ = gb.WARP_CASES[name]
        return gb.warp_pixel_slab(B, C, *(grid_hw or (Hi, Wi)))
    assert slab("slab5") == 5
    assert [slab(n) for n in ("multi_wide", "multi_crop", "small", "ragged", "crop")] == [1] * 5


# ------------------------------------------------------------------------------------------------ mutants
def _rejected(bound, fake, what):
    ratio, wrong = bound.ratio(fake)
    assert ratio > 1.0 or wrong > 0, "%s: the bound accepts the mutant (error / bound = %.3g)" % (what, ratio)
    return ratio


def test_mutant_1_last_channel_of_a_ragged_group_dropped(oracle):
    in1, in2, go, bound = gb.rs_case("lds_c6", "signed")
    i32, f32, g32 = _f32(in1, in2, go)
    bound.check(oracle.resample2d_backward(i32, f32, g32, 4, 1)[1], what="the stand-in itself")
    g32[:, 5] = 0
    _rejected(bound, oracle.resample2d_backward(i32, f32, g32, 4, 1)[1], "C = 6, channel 5 dropped")


def test_mutant_2_second_half_of_the_quotient_rule_omitted(oracle):
    in1, in2, go, bound = gb.rs_case("lds_c6", "signed")
    first, second = gb.resample2d_restatement(in1, in2, go, 4, 1, halves=True)
    bound.check((first - second).float(), what="the stand-in itself")
    _rejected(bound, first.float(), "sumgrad S / sum^2 omitted")


def test_mutant_3_sigma_gradient_divided_by_sigma_squared(oracle):
    in1, in2, go, bound = gb.rs_case("lds_store", "signed")
    fake = bound.signed.clone()
    fake[:, 2] *= in2[:, 2].double()                     # / sigma^2 instead of / sigma^3, in both halves
    _rejected(bound, fake.float(), "d/dsigma over sigma^2")
    assert bound.ratio(torch.cat((fake[:, :2], bound.signed[:, 2:]), 1).float())[0] <= 1.0       # d/dx, d/dy are untouched


def test_mutant_4_channel_slabs_overwrite_instead_of_add(oracle):
    feat, grid, go, bound = gb.warp_case("slabs", "border", "signed", False)
    f32, gr32, g32 = _f32(feat, grid, go)
    bound.check(oracle.warp_backward(f32, gr32, g32)[1], what="the stand-in itself")
    g32[:, :32] = 0                                       # 40 channels in slabs of 8: what the last slab stores survives
    _rejected(bound, oracle.warp_backward(f32, gr32, g32)[1], "warp, last slab only")
    in1, in2, go, bound = gb.rs_case("lds_slabs", "signed")
    i32, f32, g32 = _f32(in1, in2, go)
    g32[:, :16] = 0
    _rejected(bound, oracle.resample2d_backward(i32, f32, g32, 4, 1)[1], "resample2d, last slab only")


def test_mutant_5_flipcat_half_added_unmirrored(oracle):
    feat, grid, go, bound = gb.warp_case("ragged_w", "border", "signed", True)
    f32, gr32, g32 = _f32(feat, grid, go)
    C = feat.shape[1]
    bound.check(oracle.warp_backward(f32, gr32, (g32[:, :C] + g32[:, C:].flip(3)).contiguous())[1], what="the stand-in itself")
    _rejected(bound, oracle.warp_backward(f32, gr32, (g32[:, :C] + g32[:, C:]).contiguous())[1], "flipped half un-mirrored")


def test_mutant_6_corner_sign_flipped_where_a_tap_was_padded_or_clamped(oracle):
    feat, grid, go, bound = gb.warp_case("ragged_w", "border", "signed", False)
    fake, _, _ = gb.warp_restatement(feat, grid, go, False, flip_padded=True)
    changed = fake != bound.signed
    assert 0 < int(changed.sum()) < fake.numel() // 8      # border pixels only
    _rejected(bound, fake.float(), "warp: sign of corner 0 on padded pixels")
    assert bound.ratio(torch.where(changed, bound.signed, fake).float())[0] <= 1.0
    src, flow, go, k, bound = gb.be_case("grids", "signed")
    fake, _ = gb.block_extractor_restatement(src, flow, go, k, flip_clamped=True)
    assert 0 < int((fake != bound.signed).sum())
    _rejected(bound, fake.float(), "block extractor: sign of the top-left corner on clamped taps")


@pytest.mark.parametrize("kind", ["ramp", "group_mags"])
def test_mutant_7_quiet_pixel_off_by_half_the_old_allowance(oracle, kind):
    """The pixel with the smallest sum of |terms| (the quiet end of the ramp; under group_mags a pixel whose loud channels happen
    to be small), moved by half of what ``_close(..., relative=True)`` allowed: the old yardstick accepts, the per-pixel bound does
    not.  (A gather output sums over every channel, so under group_mags no pixel of the extractor's 9-tap windows is quiet: those
    two operators are probed with the ramp alone.)"""
    cases = [(gb.warp_case("b2c5_64", "border", kind, False)[3], "warp"), (gb.rs_case("lds_slabs", kind)[3], "resample2d")]
    if kind == "ramp":
        cases += [(gb.be_case("tiles", kind)[4], "block extractor"), (gb.ba_case("c8", kind)[4], "block attention d_flow"),
                  (gb.ba_case("c8", kind)[5], "block attention d_weights")]
    for bound, what in cases:
        live = torch.where(bound.mag > 0, bound.mag, torch.full_like(bound.mag, float("inf")))
        at = int(live.argmin())
        fake = bound.ref.float()
        fake.view(-1)[at] += 0.5 * 1e-5 * (1 + float(bound.ref.abs().max()))
        assert sb.global_close(fake, bound.ref, 1e-5), what
        _rejected(bound, fake, what)
