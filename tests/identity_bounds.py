"""Yardsticks of the identity evaluation (csrc/lightcnn_eval.hip, ffwm_amd/identity_eval.py); a plain helper module, not a conftest.
SAFETY, U32 (u = 2^-24, fp32's unit roundoff) and rho_any_order are those of tests/conv_bounds.py.

mfm_tail: exact.  One add (h + bias, as ATen adds it first), a selection, one add (the residual), selections (the pool): the
  reference is the fp32 PyTorch composition, compared with `assert_same` (same NaN positions, equal elsewhere).

identity_input, crop = 0: a left-to-right sum of Cin terms and one division: Cin roundings, each relative to a partial result that
  is at most sum_c |x_c| in magnitude:  |got - ref| <= SAFETY Cin u sum_c |x_c| / Cin,  ref = the float64 mean.

identity_input, crop = 1 (`crop_bound`).  ref = the float64 composition from the float64 grid formula (`crop_reference`): plane sample
  (i, j) of the 98 x 98 plane sits at source pixel (27.5 + 98 i / 97, 14.5 + 98 j / 97) -- linspace(-49, 49, 98) around (64, 77), over
  64, un-normalised by grid_sample(align_corners=False): 64 g + 63.5 -- and output pixel o reads the plane at 0.765625 (o + 0.5) - 0.5
  (clamped at 0), half-pixel centres with scale 98 / 128.  Two terms:
  * coordinates.  The resize coordinate is exact in fp32 (49 (2 o + 1) / 128 - 1 / 2 needs 15 bits).  A source coordinate formed in
    fp32 goes through a few roundings of values below 128: ATen's composition has the linspace step and its product (values <= 49),
    + 13 (<= 62), g + 1 (an error of u 2 that the factor 64 carries to u 128) and 128 (g + 1) - 1 (<= 256, halved): (49 + 64 + 64 +
    128 + 128) u < 4 (128 u).  COORD_ROUNDINGS = 4 per axis, each at most 128 u.  The output is piecewise linear and continuous in
    every source coordinate; a shift of one coordinate by d moves a bilinear sample by at most d times the largest difference
    between vertically (or horizontally) adjacent pixels of the gray image around the sample, and the resize weights sum to 1.
    `local_differences` takes that largest adjacent difference over the 7 x 7 pixels around the output pixel's own source position:
    the taps of its four plane samples span at most 3 rows and 3 columns, and the cell beyond an integer crossing is covered too.
        coord = COORD_ROUNDINGS 128 u (Dy + Dx)
  * the weighted sum.  16 taps, each the channel mean (Cin roundings), weights that are products of differences (<= 4 roundings on a
    tap's path), summed in two levels: rho_any_order(16, extra = Cin + 4) relative to sum |w x| = the float64 composition of the
    channel mean of |img| (all weights are >= 0).
  |got - ref| <= SAFETY coord + rho_any_order(16, Cin + 4) mag.  The CPU test shows that ATen's own fp32 composition fed the stored fp32
  grid meets it, that the fixture tensor does, and that two wrong variants (align_corners=True resize; row centre 64 instead of 77)
  break it by a wide factor.

cosine_topk, values: sim = <p, g> / (max(|p|, eps) max(|g|, eps)).  The dot product: D terms in any order, rho_any_order(D) relative
  to sum |p_i g_i| / den.  The denominator: each squared norm is a D-term sum of non-negative products (relative error <= (D + 1) u),
  its square root halves that and rounds once, the product of the two norms and the division round once each: a relative error of
  (D + 1 + 4) u on the similarity itself.  |got - ref| <= rho_any_order(D) sum |p g| / den + SAFETY (D + 5) u |ref|.
  Indices: equal to torch.topk of the float64 similarities where neighbouring ranks differ by more than RANK_GAP = 1e-4 (asserted on
  the inputs, which `separated_gallery` plans with gaps of 1e-3: above twice the value bound, 1.2e-4 at D = 256).

FoldedLightCNN against the reference fixture.  The LightCNN-29 that tests/golden/fill.py fills is ill-conditioned: fp32 rounding alone
  moves its outputs by percent.  The reference's own fp32 forward misses the float64 forward of the same network by
      e_ref = max( rms(fixture - float64)                       the CPU that made the fixture: 1.1e-3 on fc, rms(fc) = 0.127
                 , rms(nets.LightCNN29 on the device - float64) the module path, the vendor's convolutions: 6.2e-3 on the MI355X )
  for no other reason than fp32 rounding; both are measured in the test.  Another fp32 evaluation order is a further draw from that
  error; largest-element errors of such a network are heavy-tailed (a max-feature-map selection that flips), so the comparison is in
  RMS:  rms(got - float64) <= SAFETY e_ref  and  rms(got - fixture) <= (SAFETY + 1) e_ref.  (The CPU figure alone does not describe the
  device: the module path on the MI355X misses SAFETY times it by the same factor as the folded path, 5.7.)  A wrong layer (a pool or
  residual left out, halves swapped) moves the outputs by their own magnitude, 20 x e_ref.  The well-conditioned check of the same
  code is the float64 comparison of `conditioned_lightcnn`, 1e-4 max|ref|.
"""
import math
import os
import sys

import torch
import torch.nn.functional as F

from conv_bounds import SAFETY, U32, rho_any_order  # noqa: F401  (re-exported)
from small_kernel_bounds import assert_same  # noqa: F401  (re-exported)

COORD_ROUNDINGS = 4.0
RANK_GAP = 1e-4
PLANE, FACE = 98, 128
ROW_ORIGIN, COL_ORIGIN = 27.5, 14.5          # (77 - 49) - 64 + 63.5, (64 - 49) - 64 + 63.5

# ---- mfm_tail: the GPU matrix, shapes of h.  The last two pass one sweep of the 2048-block grid on their route (vector, scalar), with
# and without the pool; (2, 10, 6, 8) is the vector route with a batch stride; the odd planes have windows that hang over the edge
KBLOCK, EW_BLOCKS = 256, 2048                 # common.hpp:13, lightcnn_eval.hip `kEwBlocks`
TAIL_SHAPES = [(1, 2 * 3, 5, 7), (2, 2 * 2, 1, 1), (2, 2 * 48, 15, 15), (1, 2 * 8, 16, 16), (2, 2 * 5, 6, 8),
               (1, 2 * 33, 512, 256), (1, 2 * 9, 481, 487)]


def tail_route(shape, pool):
    """lightcnn_eval.hip, ffwm_mfm_tail_forward: vec = W % 4 == 0 (aligned pointers); items = outputs / 4 (vector), / 2 (vector +
    pool), / 1 (scalar).  -> (route, items, past one sweep)."""
    B, C2, H, W = shape
    C = C2 // 2
    outs = B * C * (((H + 1) // 2) * ((W + 1) // 2) if pool else H * W)
    vec = W % 4 == 0
    items = outs // (2 if pool else 4) if vec else outs
    return ("vector" if vec else "scalar"), items, items > EW_BLOCKS * KBLOCK


def tail_reference(h, bias, residual, pool):
    """The fp32 PyTorch composition on the CPU."""
    h = h.detach().cpu()
    if bias is not None:
        h = h + bias.detach().cpu().view(1, -1, 1, 1)
    a, b = torch.split(h, h.shape[1] // 2, 1)
    y = torch.max(a, b)
    if residual is not None:
        y = y + residual.detach().cpu()
    return F.max_pool2d(y, 2, 2, ceil_mode=True) if pool else y


def tail_inputs(shape, seed, with_bias, with_res, pool):
    """h, bias, residual with exact ties between the halves, -0 / +0 and infinities, and NaN planted where it must travel: in the
    first half, in the second, in the residual -- one of them in the last row and one in the last column, where a ceil-mode window
    hangs over the edge when H or W is odd."""
    gen = torch.Generator().manual_seed(seed)
    B, C2, H, W = shape
    C = C2 // 2
    h = torch.randn(shape, generator=gen)
    bias = torch.randn(C2, generator=gen) if with_bias else None
    res = torch.randn(B, C, H, W, generator=gen) if with_res else None
    flat = h.view(B, 2, -1)
    flat[:, 1, ::7] = flat[:, 0, ::7]                     # ties (of h; with a bias only where the two biases agree)
    flat[:, 0, 3::11] = 0.0
    flat[:, 1, 3::11] = -0.0
    if h.numel() >= 64:
        flat[:, 0, 5::53] = float("inf")
        flat[:, 1, 6::59] = -float("inf")
    nan = float("nan")
    h[0, 0, H - 1, W - 1] = nan                           # first half, the corner window
    h[B - 1, C2 - 1, H - 1, 0] = nan                      # second half, last row
    h[0, C - 1, 0, W - 1] = nan                           # first half, last column
    if res is not None:
        res[B - 1, 0, H // 2, W - 1] = nan
    return h.contiguous(), bias, res


# ---- identity_input
def gray_bound(img):
    """-> (float64 mean [B, 1, H, W], per-element bound)."""
    x = img.detach().cpu().double()
    cin = x.shape[1]
    return x.mean(1, keepdim=True), SAFETY * cin * U32 * x.abs().sum(1, keepdim=True) / cin


def crop_coordinates(dtype=torch.float64):
    """-> (ys [98], xs [98]): the source pixel coordinates of the plane's rows and columns."""
    i = torch.arange(PLANE, dtype=dtype)
    return ROW_ORIGIN + 98.0 * i / 97.0, COL_ORIGIN + 98.0 * i / 97.0


def _resize_coordinates(align_corners=False):
    o = torch.arange(FACE, dtype=torch.float64)
    if align_corners:
        return o * (PLANE - 1.0) / (FACE - 1.0)
    return (0.765625 * (o + 0.5) - 0.5).clamp(min=0.0)


def _lerp_axis(t, coord, dim):
    """Linear interpolation of t along `dim` at the float64 positions `coord` (all taps in range; the upper tap is clamped)."""
    n = t.shape[dim]
    i0 = coord.floor().long().clamp(max=n - 1)
    i1 = (i0 + 1).clamp(max=n - 1)
    w1 = coord - i0.double()
    shape = [1] * t.dim()
    shape[dim] = -1
    return t.index_select(dim, i0) * (1.0 - w1).view(shape) + t.index_select(dim, i1) * w1.view(shape)


def crop_reference(img, row_origin=ROW_ORIGIN, align_corners=False):
    """mean -> WarpNet(build_grid(b, 98)) -> bilinear resize to 128 in float64 from the float64 coordinate formula (both steps are
    separable).  row_origin / align_corners: the two wrong variants the CPU test holds the bound against."""
    gray = img.detach().cpu().double().mean(1, keepdim=True)
    ys, xs = crop_coordinates()
    ys = ys - ROW_ORIGIN + row_origin
    plane = _lerp_axis(_lerp_axis(gray, ys, 2), xs, 3)                     # [B, 1, 98, 98]
    r = _resize_coordinates(align_corners)
    return _lerp_axis(_lerp_axis(plane, r, 2), r, 3)


def crop_taps_inside():
    """Every tap of the crop lies inside the 128 x 128 image (zero padding never applies): from the coordinates."""
    ys, xs = crop_coordinates()
    return bool(ys.min() >= 0 and xs.min() >= 0 and ys.floor().max() + 1 <= FACE - 1 and xs.floor().max() + 1 <= FACE - 1)


def local_differences(gray):
    """-> (Dy, Dx) [B, 1, 128, 128]: the largest |difference| between vertically / horizontally adjacent pixels of gray (float64)
    within the 7 x 7 pixels around each output pixel's own source position."""
    dv = F.pad((gray[:, :, 1:] - gray[:, :, :-1]).abs(), (0, 0, 0, 1))
    dh = F.pad((gray[:, :, :, 1:] - gray[:, :, :, :-1]).abs(), (0, 1, 0, 0))
    dv, dh = F.max_pool2d(dv, 7, 1, 3), F.max_pool2d(dh, 7, 1, 3)
    ys, xs = crop_coordinates()
    r = _resize_coordinates()
    yc = _lerp_axis(ys.view(1, 1, -1, 1), r, 2).view(-1).round().long()
    xc = _lerp_axis(xs.view(1, 1, 1, -1), r, 3).view(-1).round().long()
    return dv.index_select(2, yc).index_select(3, xc), dh.index_select(2, yc).index_select(3, xc)


def crop_bound(img):
    """-> (float64 reference [B, 1, 128, 128], per-element bound); see the module docstring."""
    x = img.detach().cpu().double()
    cin = x.shape[1]
    ref = crop_reference(x)
    mag = crop_reference(x.abs())
    dy, dx = local_differences(x.mean(1, keepdim=True))
    coord = COORD_ROUNDINGS * 128.0 * U32 * (dy + dx)
    return ref, SAFETY * coord + rho_any_order(16, extra=cin + 4) * mag


def worst_ratio(got, ref, bound):
    q = (got.detach().cpu().double() - ref).abs() / bound
    q = torch.where(torch.isnan(q), torch.full_like(q, math.inf), q)
    return float(q.max())


# ---- cosine_topk
def cosine_reference(probe, gallery):
    """-> (float64 similarities [B, G], per-element bound of an fp32 evaluation)."""
    p, g = probe.detach().cpu().double(), gallery.detach().cpu().double()
    D = p.shape[1]
    den = p.norm(dim=1).clamp(min=1e-8).view(-1, 1) * g.norm(dim=1).clamp(min=1e-8).view(1, -1)
    ref = (p @ g.t()) / den
    mag = (p.abs() @ g.abs().t()) / den
    return ref, rho_any_order(D) * mag + SAFETY * (D + 5) * U32 * ref.abs()


def rank_gaps(ref, k):
    """-> the smallest gap between neighbouring ranks among the first k + 1 of every row of the float64 similarities."""
    top = torch.sort(ref, dim=1, descending=True)[0][:, :min(k + 1, ref.shape[1])]
    return float((top[:, :-1] - top[:, 1:]).min()) if top.shape[1] > 1 else math.inf


def separated_gallery(B, G, D, seed):
    """Seeded probes and gallery rows with planned similarities (the caller asserts the gaps on the float64 similarities of the fp32
    tensors): the probes are B orthogonal directions (B <= D - 1) of random length; gallery row j belongs to probe j % B, lies at
    cosine s_j to it and is orthogonal to the other probes; the first 64 rows of a probe have s = 0.95, 0.949, ... (steps of 1e-3),
    the rest are uniform in [-0.9, 0.8].  Rows have random lengths and are shuffled, so the leaders are spread over the gallery."""
    gen = torch.Generator().manual_seed(seed)
    q = torch.linalg.qr(torch.randn(D, B, generator=gen, dtype=torch.float64))[0].t()          # [B, D], orthonormal rows
    j = torch.arange(G)
    owner, rank = j % B, j // B
    s = torch.where(rank < 64, 0.95 - 1e-3 * rank.double(), torch.rand(G, generator=gen, dtype=torch.float64) * 1.7 - 0.9)
    noise = torch.randn(G, D, generator=gen, dtype=torch.float64)
    noise = noise - (noise @ q.t()) @ q
    noise = noise / noise.norm(dim=1, keepdim=True)
    rows = s.view(-1, 1) * q[owner] + (1 - s * s).sqrt().view(-1, 1) * noise
    rows = rows * (0.5 + 2.0 * torch.rand(G, 1, generator=gen, dtype=torch.float64))
    rows = rows[torch.randperm(G, generator=gen)]
    probe = q * (0.5 + 2.0 * torch.rand(B, 1, generator=gen, dtype=torch.float64))
    return probe.float().contiguous(), rows.float().contiguous()


# ---- the rank-1 meter's synthetic case (tests/golden/make_identity_golden.py feeds it to the reference's AverageMeter)
CAMERAS = ["050", "140", "041", "130", "080", "190", "090", "200", "010", "120", "110", "240"]


def meter_case(seed=33):
    """-> (24 probe names, two per camera; 20 gallery keys; probe features [24, 256]; gallery features [20, 256]).  A probe is its
    identity's gallery feature plus noise; every fifth probe is built on ANOTHER identity's feature, so some matches are wrong.  The
    seed is one at which neighbouring ranks among each probe's first eleven differ by more than RANK_GAP (the CPU test asserts it)."""
    gen = torch.Generator().manual_seed(seed)
    keys = ["%03d" % (i + 1) for i in range(20)]
    gallery = torch.randn(20, 256, generator=gen)
    names, rows = [], []
    for n in range(24):
        ident = (7 * n + 3) % 20
        names.append("multipie/test/%s_01_01_%s_%02d.png" % (keys[ident], CAMERAS[n % 12], n % 20))
        src = (ident + 1) % 20 if n % 5 == 2 else ident
        rows.append(gallery[src] + 0.5 * torch.randn(256, generator=gen))
    return names, keys, torch.stack(rows).contiguous(), gallery.contiguous()


def golden_dir():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fill_module():
    sys.path.insert(0, golden_dir())
    import fill
    return fill


# ---- FaceIdentifier's case, shared by the CPU check of its inputs and the GPU test
def identifier_case():
    """-> (gallery keys, gallery images [12, 1, 128, 128], probes [4, 3, 128, 128], probes of a second call): seeded images that differ
    visibly -- the closed-form waves of tests/golden/fill.py under different names, each gallery image at its own contrast and brightness."""
    fill = fill_module()
    keys = ["%03d" % (i + 1) for i in range(12)]
    gallery = torch.cat([(fill.image(1, 1, 128, 128, "gallery_%d" % i) - 0.5) * (0.25 + 0.06 * i) + 0.4 + 0.01 * i for i in range(12)], 0)
    return keys, gallery.contiguous(), fill.image(4, 3, 128, 128, "eval_img_S"), fill.image(4, 3, 128, 128, "eval_img_F")


def qualifying_rows(sim, gap=RANK_GAP):
    """Rows of descending similarities [B, k] whose neighbouring ranks differ by more than `gap`."""
    s = sim.detach().cpu().double()
    return (s[:, :-1] - s[:, 1:]).min(dim=1)[0] > gap


def saved_lightcnn(path):
    """A `fill`ed LightCNN-29 saved as a plain state dict, as FFWMModel.load_network reads it."""
    from ffwm_amd import nets
    net = fill_module().fill_module(nets.LightCNN29())
    torch.save({k: v.detach().cpu() for k, v in net.state_dict().items()}, path)
    return path


def conditioned_lightcnn(seed=31):
    """A seeded nets.LightCNN29 (eval, CPU) that is well conditioned AND follows its input: weights N(0, 1 / fan_in), no biases.  Its fp32
    forward keeps 5e-7 of float64, and without biases every bit of its feature is carried from the input through all 29 layers (see
    `structured_image` for how far inputs move it).  (PyTorch's default initialisation shrinks the signal layer by layer until the biases
    make most of the feature; the network tests/golden/fill.py fills turns a one-ulp change of its input into 2 % of the feature.)"""
    from ffwm_amd import nets
    torch.manual_seed(seed)
    net = nets.LightCNN29()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear)):
                m.weight.normal_(0, m.weight[0].numel() ** -0.5)
                m.bias.zero_()
    return net.eval()


def structured_image(B, H, W, name="lightcnn_in"):
    """fill.image under a diagonal brightness ramp: an input whose feature differs from the plain image's by most of its size (two
    plain fill images are statistically alike and move the feature of `conditioned_lightcnn` by 1 %; zeroing one edge column moves it
    by 2e-3, a single pixel by 6e-4 -- all above the 1e-4 the folded path is held to)."""
    fill = fill_module()
    ry, rx = torch.linspace(0, 1, H).view(1, 1, H, 1), torch.linspace(0, 1, W).view(1, 1, 1, W)
    return (fill.image(B, 1, H, W, name) * ry * rx).contiguous()
