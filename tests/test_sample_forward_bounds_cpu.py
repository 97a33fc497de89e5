"""The per-element yardstick of tests/sample_forward_bounds.py, checked on the CPU at the shapes and families of
tests/test_gpu_sample_forward_bounds.py:

  * the float32 oracle -- the reference's own arithmetic -- meets every bound at rho / SAFETY;
  * it reproduces the float64 reference EXACTLY on the exact family, and the source value itself where the flow is an integer;
  * the small-sigma inputs judge at most 5 % of their elements through the slack arm, and do hold dead pixels, underflowing
    products and the EPS arm;
  * what the profiler scopes cannot tell is a property of the inputs and proven here: which tiles of the warp's LDS kernel leave
    LDS, which direct warp cases keep a four-channel slab, where a tile's staged box starts next to pixels without a valid corner;
  * six mutants pass the former yardstick max|diff| <= 2e-6 on the same inputs and fail the per-element bound; a seventh restates
    what warp_fwd_lds_kernel did to pixels without a valid corner (the former tests had no non-finite source at all).

Worst error / bound of the float32 oracle at rho / SAFETY:

    warp, power-of-two sizes     0.45     the 2^24 route, feat_mags (rho / SAFETY is 8 u)
    warp, other sizes            0.58     in [1, 3, 96, 130] -> grid 80 x 129, border grid, signed (kappa leads)
    block extractor              0.35     k = 3, ramp
    block attention              0.14     k = 2, feat_mags sources and weights
    resample2d                   0.17     C = 5, ks 2, huge (outside the slack arm, whose ratio is |error| / mag by construction)
"""
import pytest
import torch

import gather_bounds as gb
import sample_forward_bounds as sf
import scatter_bounds as sb


def _as_f32(bound):
    """The bound of a float32 implementation of the same case (the float64 cases carry u64 in kappa)."""
    scale = sb.unit_roundoff(torch.float32) / sb.unit_roundoff(bound.dtype)
    return sf.Bound(bound.ref, bound.mag, bound.kappa * scale, bound.units, torch.float32)


def _f32(*ts):
    """Float32 COPIES: the cached cases stay as they were built."""
    return [t.to(torch.float32, copy=True).contiguous() for t in ts]


def _reference_meets(bound, got, what):
    _as_f32(bound).check(got, bound.units / sf.SAFETY, "fp32 oracle, " + what)


# ------------------------------------------------------------------------------------------------ the float32 oracle
WARP_CASES = sorted({row[1:] for row in sf.WARP_ROWS}, key=str)


@pytest.mark.parametrize("name,grid_kind,kind,flipcat", WARP_CASES)
def test_warp_reference(oracle, name, grid_kind, kind, flipcat):
    feat, grid, bound = sf.warp_case(name, grid_kind, kind, flipcat)
    _reference_meets(bound, oracle.warp_forward(*_f32(feat, grid), flipcat), "warp %s %s %s flipcat %d" % (name, grid_kind, kind, flipcat))
    if grid_kind == "outside":         # bands of pixels without a valid corner: exactly 0 in the reference, and no slack
        dead = bound.mag == 0
        assert int(dead.sum()) > 0 and float((bound.ref[dead]).abs().max()) == 0.0 and float(bound.kappa[dead].abs().max()) == 0.0
    if kind == "nonfinite":
        assert int((~torch.isfinite(bound.ref)).sum()) > 0


@pytest.mark.parametrize("name,kind", sorted({(sf.BE_PATHS[path][0], kind) for path, kind in sf.BE_ROWS}))
def test_block_extractor_reference(oracle, name, kind):
    src, flow, k, bound = sf.be_case(name, kind)
    _reference_meets(bound, oracle.block_extractor_forward(*_f32(src, flow), k), "block extractor %s %s" % (name, kind))
    if kind == "nonfinite":
        assert int((~torch.isfinite(bound.ref)).sum()) > 0


@pytest.mark.parametrize("name,kind,wkind", sorted({(n, k, w) for n, _, k, w in sf.BA_ROWS}))
def test_block_attention_reference(oracle, name, kind, wkind):
    src, flow, w, k, bound = sf.ba_case(name, kind, wkind)
    _reference_meets(bound, sf.attention_composition(oracle, *_f32(src, flow, w), k), "block attention %s %s %s" % (name, kind, wkind))


@pytest.mark.parametrize("name,kind", [r for r in sf.RS_ROWS if r[0] != "direct_small_sigma_f64"])      # (float64 has no underflow regime)
def test_resample2d_reference(oracle, name, kind):
    in1, in2, ks, dil, bound = sf.rs_case(name, kind)
    _reference_meets(bound, oracle.resample2d_forward(*_f32(in1, in2), ks, dil), "resample2d %s %s" % (name, kind))


def test_resample2d_reference_on_a_call_with_irregular_blocks(oracle):
    in1, in2, ks, dil, bound = sf.rs_case("lds_c6", "signed")
    bad = sf.rs_irregular(in2)
    assert int((bad != in2).sum()) == 2
    got = oracle.resample2d_forward(*_f32(in1, bad), ks, dil)
    ref = oracle.resample2d_forward(in1.double(), bad.double(), ks, dil)
    assert gb.same_nonfinite(got, ref) == 0 and not bool(torch.isfinite(ref[0, :, 20, 11]).any())
    same = torch.ones_like(ref, dtype=torch.bool)
    same[0, :, 5, 7] = same[0, :, 20, 11] = False
    assert torch.equal(ref[same], bound.ref[same])     # every other pixel is the regular call's


# ------------------------------------------------------------------------------------------------ the exact family
@pytest.mark.parametrize("flipcat", [False, True])
@pytest.mark.parametrize("shape", sf.EXACT_WARP)
def test_warp_exact_family(oracle, shape, flipcat):
    feat, grid, ref = sf.warp_exact_case(shape, flipcat)
    assert torch.equal(oracle.warp_forward(feat, grid, flipcat).double(), ref)
    B, C, H, W = shape
    ix = ((grid[:, 0].double() + 1) * W - 1) / 2
    whole = (ix == ix.round())[:, ::3]
    assert bool(whole.all())
    # an integer sample inside the image: weights 0 and 1, the output is the source value
    iy = ((grid[:, 1].double() + 1) * H - 1) / 2
    ok = (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1) & (ix == ix.round()) & (iy == iy.round())
    picked = feat.double().reshape(B, C, H * W).gather(2, (iy.clamp(0, H - 1) * W + ix.clamp(0, W - 1)).long().reshape(B, 1, -1).expand(B, C, -1))
    assert int(ok.sum()) > 100 and torch.equal(ref[:, :C][ok.unsqueeze(1).expand(B, C, H, W)], picked.view(B, C, H, W)[ok.unsqueeze(1).expand(B, C, H, W)])


@pytest.mark.parametrize("name", sf.EXACT_BE)
def test_block_extractor_exact_family(oracle, name):
    src, flow, k, ref = sf.be_exact_case(name)
    assert torch.equal(oracle.block_extractor_forward(src, flow, k).double(), ref)
    assert bool((flow[:, :, ::3] == flow[:, :, ::3].round()).all()) and float(ref.abs().max()) <= 31


# ------------------------------------------------------------------------------------------------ what the inputs are for
@pytest.mark.parametrize("name", ["lds_small_sigma", "direct_small_sigma"])
def test_small_sigma_slack_share_and_regimes(oracle, name):
    """At most 5 % of the elements are judged through the slack arm (none, with this sigma set: see sf.rs_small_sigma); the inputs do hold dead pixels (every float product
    underflows), live pixels with products below the normal range, and both of sb.rs_small_sigma's flow populations."""
    in1, in2, ks, dil, bound = sf.rs_case(name, "signed")
    assert bound.slack_share() <= sf.SLACK_SHARE_CAP, bound.slack_share()
    assert 0.1 < float(bound.dead.double().mean()) < 0.5
    assert float(bound.ref[bound.dead.expand_as(bound.ref)].abs().max()) == 0.0
    tp, s, _ = sf.rs_taps(in2, ks, dil, in1.shape[2], in1.shape[3], torch.float32)
    under = sum(((wy * wx) < 2.0 ** -126) & (s >= sb.SUBNORMAL_SUM) for wy, wx, _, _ in tp)
    assert int((under > 0).sum()) > 500
    assert float(in2[:, :2].abs().max()) > 4.0


def test_sigma_zero_takes_the_eps_arm(oracle):
    in1, in2, ks, dil, bound = sf.rs_case("lds_sigma_zero", "signed")
    assert float(in2[:, 2].abs().max()) == 0.0
    assert bool(bound.dead[:, :, 1::2].all())                        # odd flows: every weight is exp(-v^2 / 1e-8) = 0
    assert float(bound.ref[:, :, 1::2].abs().max()) == 0.0
    whole = ((in2[:, 0] == in2[:, 0].round()) & (in2[:, 1] == in2[:, 1].round()))[:, None]
    assert bool(whole[:, :, ::2].all()) and not bool(bound.dead[whole].any())
    B, C, H, W = in1.shape
    ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    row = (ys + in2[:, 1].long()).clamp(0, H - 1)
    col = (xs + in2[:, 0].long()).clamp(0, W - 1)
    picked = in1.double().reshape(B, C, H * W).gather(2, (row * W + col).reshape(B, 1, -1).expand(B, C, -1)).view(B, C, H, W)
    m = whole.expand(B, C, H, W)
    assert torch.equal(bound.ref[m], picked[m])                      # the tap at distance 0 has weight 1: the source value


def test_warp_lds_cases_leave_lds_only_under_zoom25():
    """The profiler scope cannot tell warp_fwd_lds_kernel's staged arm from its direct-gather arm (the same 64 x 16 tiles and
    128 x 32 boxes as the d(flow) kernel's: gather_bounds.warp_lds_boxes): under zoom25 some tiles of [1, 2, 66, 66] leave LDS
    while others of the same launch stay; under every other grid of the LDS rows every tile stays."""
    for name, grid_kind in sorted({(r[1], r[2]) for r in sf.WARP_ROWS if r[0] in ("lds", "natural")}):
        (B, C, Hi, Wi), grid_hw, _ = sf.WARP_CASES[name]
        boxes = gb.warp_lds_boxes(gb.warp_grid(grid_kind, B, (Hi, Wi), grid_hw or (Hi, Wi), 261), (Hi, Wi))
        direct = sum(1 for bw, bh in boxes if bw > 128 or bh > 32)
        if grid_kind == "zoom25":
            assert 0 < direct < sum(1 for bw, bh in boxes if bw > 0), (name, boxes)
        else:
            assert direct == 0 and max(bw for bw, _ in boxes) > 0, (name, grid_kind, boxes)


def test_warp_nonfinite_family_reaches_the_staged_box_of_tiles_with_dead_pixels():
    """Under the `outside` grid of in [1, 3, 96, 130] -> 80 x 129 a tile holds pixels without a valid corner beside live ones, and its
    staged box starts INSIDE the image: the nonfinite family puts a NaN on that first cell, which the dead pixels' four LDS reads
    land on.  The reference gives those pixels 0."""
    (B, C, Hi, Wi), grid_hw, _ = sf.WARP_CASES["grids"]
    grid = sf.warp_grid("nonfinite", "outside", B, (Hi, Wi), grid_hw, 261)
    cells = sf.warp_lds_dead_origins(grid, (Hi, Wi))
    assert len(cells) > 0
    feat, _, bound = sf.warp_case("grids", "outside", "nonfinite", False)
    assert all(bool(torch.isnan(feat[c])) for c in cells)
    dead = bound.mag == 0
    assert int(dead.sum()) > 0 and float(bound.ref[dead].abs().max()) == 0.0


def test_warp_direct_cases_and_their_slabs():
    """warp_fwd_body walks its slab four channels per trip and the rest one by one.  plan() cuts the small cases down to one
    channel per block (the remainder loop alone); [4, 5 / 7, 512, 512] keep their whole slab (one trip + 1 / 3) and
    [2, 8, 512, 512] runs two slabs of four."""
    def slab(name):
        (B, C, Hi, Wi), grid_hw, _ = sf.WARP_CASES[name]
        return sf.warp_forward_slab(B, C, *(grid_hw or (Hi, Wi)))
    assert [slab(n) for n in ("trip5", "trip7", "slabs")] == [5, 7, 4]
    assert [slab(n) for n in ("c5_64", "c7", "small", "grids")] == [1] * 4


def test_resample2d_two_rows_per_thread_case_is_the_smallest():
    (B, C, H, W), _, _, _, _, _, _ = sf.RS_CASES["lds_rpt2"]
    assert B * ((W + 63) // 64) * ((H + 7) // 8) == 2048


def test_nonfinite_family_touches_a_cell_with_weight_zero(oracle):
    """The integer rows: the pixel left of the interior +Inf cell takes it as its right-hand tap with weight 0 -- 0 x Inf = NaN in
    the reference (block extractor: the centre tap of that flow pixel's window)."""
    src, flow, k, bound = sf.be_case("k3", "nonfinite")
    _, C, Hs, Ws = src.shape
    yf, xf = Hs // 2, Ws // 2 - 1
    assert float(flow[0, :, yf, xf].abs().max()) == 0.0 and bool(torch.isinf(src[0, 1, yf, xf + 1]))
    assert bool(torch.isnan(bound.ref[0, 1, 3 * yf + 1, 3 * xf + 1]))


# ------------------------------------------------------------------------------------------------ mutants
def _rejected_but_formerly_accepted(bound, fake, what):
    assert sf.old_yardstick(fake, bound.ref), "%s: the former yardstick rejects the mutant as well" % what
    ratio, wrong = bound.ratio(fake)
    assert ratio > 1.0 or wrong > 0, "%s: the bound accepts the mutant (error / bound = %.3g)" % (what, ratio)


def _warp_standin(name, grid_kind, kind):
    feat, grid, bound = sf.warp_case(name, grid_kind, kind, False)
    s, w, valid, _, _ = sf.warp_parts(feat, grid)
    shape = grid.shape[2:]
    bound.check(sf.warp_compose(s, w, valid, shape), what="the stand-in itself")
    return s, w, valid, shape, bound


def test_mutant_1_one_tap_from_the_neighbouring_cell_in_the_quiet_channel(oracle):
    """Channel 1 of feat_mags (1e-5 next to 1 and 1e3): the first corner reads the cell to its right, on the pixels where that
    moves the output by no more than 2e-6."""
    s, w, valid, shape, bound = _warp_standin("c5_64", "border", "feat_mags")
    diff = (w[0] * (s[1] - s[0]))[:, 1].abs()
    hit = (diff <= sf.OLD_YARDSTICK) & valid[0][:, 0] & valid[1][:, 0]
    assert float(hit.double().mean()) > 0.5
    s0 = s[0].clone()
    s0[:, 1] = torch.where(hit, s[1][:, 1], s[0][:, 1])
    _rejected_but_formerly_accepted(bound, sf.warp_compose([s0] + s[1:], w, valid, shape), "neighbouring tap, quiet channel")


def test_mutant_2_relative_error_of_2_to_the_minus_12_in_one_corner_weight(oracle):
    s, w, valid, shape, bound = _warp_standin("c5_64", "border", "tiny")
    _rejected_but_formerly_accepted(bound, sf.warp_compose(s, w[:3] + [w[3] * (1 + 2.0 ** -12)], valid, shape), "corner weight off by 2^-12")
    in1, in2, ks, dil, bound = sf.rs_case("lds_c6", "tiny")
    good = sf.rs_forward_torch(in1, in2, ks, dil, torch.float64)
    bound.check(good, what="the stand-in itself")
    tp, s_, _ = sf.rs_taps(in2, ks, dil, in1.shape[2], in1.shape[3], torch.float64)
    wy, wx, row, col = tp[0]
    B, C = in1.shape[:2]
    v = gb._gather(in1.double().reshape(B, C, -1), row.reshape(B, -1), col.reshape(B, -1), in1.shape[3]).view_as(good)
    fake = good + 2.0 ** -12 * (wy * wx / s_)[:, None] * v
    _rejected_but_formerly_accepted(bound, fake, "resample2d: first tap's weight off by 2^-12")


def test_mutant_3_first_corner_dropped_on_pixels_with_a_zero_padded_corner(oracle):
    s, w, valid, shape, bound = _warp_standin("c7", "border", "tiny")
    padded = ~(valid[0] & valid[1] & valid[2] & valid[3])
    hit = padded & valid[0]
    assert 0 < int(hit.sum()) < hit.numel() // 8           # border pixels only
    _rejected_but_formerly_accepted(bound, sf.warp_compose(s, w, [valid[0] & ~padded] + valid[1:], shape), "first corner dropped on padded pixels")


def test_mutant_4_resample2d_normalised_per_axis_on_small_sigma(oracle):
    """What ADVICE.md records of rs_bwd1_owned_kernel: the per-axis sums do not underflow where the 2-D products do, so a pixel the
    reference's SAFE_DIV(0, 0) zeroes gets an O(source) value."""
    in1, in2, ks, dil, bound = sf.rs_case("lds_small_sigma", "tiny")
    bound.check(sf.rs_forward_torch(in1, in2, ks, dil, torch.float32), what="the stand-in itself")
    _rejected_but_formerly_accepted(bound, sf.rs_forward_torch(in1, in2, ks, dil, torch.float32, "per_axis"), "per-axis normalisation")


def test_mutant_5_subnormal_products_flushed_to_zero_under_tiny(oracle):
    """sigma = 0.1 near half-integer positions: the weight sum is a normal 1e-9 or so, every term of a 1e-30 source is subnormal --
    flushed, the output is 0 where the reference keeps 1e-30."""
    in1, in2, ks, dil, bound = sf.rs_case("lds_sigma_tenth", "tiny")
    bound.check(sf.rs_forward_torch(in1, in2, ks, dil, torch.float32), what="the stand-in itself")
    _rejected_but_formerly_accepted(bound, sf.rs_forward_torch(in1, in2, ks, dil, torch.float32, "flush"), "subnormal products flushed")


def test_mutant_6_nan_cell_replaced_by_zero_where_its_weight_is_zero(oracle):
    s, w, valid, shape, bound = _warp_standin("c5_64", "border", "nonfinite")
    fake = sf.warp_compose([torch.where(wq == 0, torch.nan_to_num(sq, nan=0.0, posinf=0.0, neginf=0.0), sq) for sq, wq in zip(s, w)], w, valid, shape)
    assert sf.old_yardstick(fake, bound.ref)
    ratio, wrong = bound.ratio(fake)
    assert wrong > 0 and ratio <= 1.0                      # placement alone: every finite element is unchanged


def test_mutant_7_dead_pixel_reads_the_staged_box(oracle):
    """What warp_fwd_lds_kernel did before this yardstick: a pixel without a valid corner multiplied the first four cells of its
    tile's box by weight 0 -- NaN where the box holds one."""
    feat, grid, bound = sf.warp_case("grids", "outside", "nonfinite", False)
    fake = bound.ref.clone()
    dead = bound.mag == 0
    fake[0, :, :, 64:128] = torch.where(dead[0, :, :, 64:128], torch.full_like(fake[0, :, :, 64:128], float("nan")), fake[0, :, :, 64:128])
    assert bound.ratio(fake)[1] > 0                        # (the former tests had no non-finite source: they never looked)


@pytest.mark.parametrize("flipcat", [False, True])
def test_warp_grad_flow_reference_on_the_nonfinite_dead_tile_input(oracle, flipcat):
    """The input of test_gpu_gather_bounds.py::test_warp_grad_flow_lds_dead_pixels_beside_a_nonfinite_cell: the float32 oracle meets
    gather_bounds' d_flow bound at rho / SAFETY, some pixels are non-finite and the pixels without a valid corner are exactly 0."""
    feat, grid, _ = sf.warp_case("grids", "outside", "nonfinite", flipcat)
    go = gb.grads("signed", (1, 6 if flipcat else 3, 80, 129), 163)
    bound = gb.warp_flow_bound(feat, grid, go, flipcat)
    _, got = oracle.warp_backward(*_f32(feat, grid, go), flipcat)
    bound.check(got, bound.units / gb.SAFETY, "fp32 oracle, warp d_flow, nonfinite features")
    dead = bound.mag == 0
    assert int(dead.sum()) > 1000 and float(bound.ref[dead].abs().max()) == 0.0 and int((~torch.isfinite(bound.ref)).sum()) > 0
