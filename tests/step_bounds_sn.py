"""Per-stage float64 bounds and an exact family for the batched spectral norm (csrc/spectral_norm.hip), float32 and float64; the
conventions and the yardstick are those of tests/step_bounds.py.  `unit` is u = 2^-24 for the float32 kernels and u64 = 2^-53 for the
float64 ones; every sum also carries the float64 reference's own n u64 sum |t| (rule (S)), which is what limits the float64 checks.

Every intermediate is observable, so no stage inherits another's error.  W is [rows, cols]; a 256-thread block is 4 waves of 64.
  v_out   against normalize(W^T u_in).  Phase 1: a wave adds every fourth row, chain L1 = ceil(rows / 4), 4 waves meet, the products
          are rounded: |v_raw_j - ref| <= delta_j = rho (L1 + 4 + 1) A_j, A = |W|^T |u|, rho = SAFETY unit.  The norm: block_sumsq, chain
          ceil(cols / 256), 64 + 4 partials, the squares rounded, then the square root: relative rn = rho (1/2 (ceil(cols / 256) + 68 +
          1) + 1), and it moves by at most |delta|_2.  With d = max(|v_raw|, eps):
              |v_j - ref_j| <= delta_j / d + |ref_j| (|delta|_2 / d + rn + rho)        (the last: the division)
  wv      against W v_out with the kernel's OWN v_out (phase 2 divides v_raw by the same norm, computed by the same code): a wave per
          row, chain ceil(cols / 64), 64 lanes meet, product and division rounded: rho (ceil(cols / 64) + 64 + 2) (|W| |v|)_i.
  u_out   against wv / max(|wv|, eps) from the kernel's wv: |ref_i| (rho (1/2 (ceil(rows / 256) + 69) + 2)).
  sigma   against u_out . wv (the kernel's): rho (ceil(rows / 256) + 68 + 1) sum |u_i wv_i|.
  weight_sn against W / sigma_kernel: one division, unit |ref| -- EVERY 8192-element chunk recomputes sigma, only chunk 0 publishes it.
  u_saved, v_saved bit-equal u_out, v_out (and the call with both NULL gives the same results).
  power_iterations = 0: u, v bit-unchanged, wv against W v_in, sigma against u_in . wv.
Squares within range (float32): |v_raw|^2 and |wv|^2 over n elements must be zero or lie in [n 2^-102, 2^120], else ValueError: below,
the squares that underflow (each loses at most 2^-126) may add up to more than one rounding u of the sum; above, squares overflow;
nothing is claimed there.  The families at scale 2^-40 and 2^40 stay inside (tiny layers at 2^-40 run through the eps clamp).
Backward, from the kernel's u, v, sigma:  dW = G / sigma - (<G, W> / sigma^2) u v^T, mag = |G| / sigma + (sum |G W| / sigma^2) |u_r| |v_c|.
  A chunk's partial: chain min(8192, n) / 256 <= 32, 68 partials, rounded products; the sum of the ceil(n / 8192) partials: chain
  ceil(chunks / 256), 68 partials.  L = 32 + ceil(chunks / 256), P = 136; + 8 for the products, sigma^2, the two divisions, u v, the
  product with the coefficient and the subtraction:   |dW - ref| <= (rho (L + P + 8) + n u64) mag.
  partials[c] against the chunk's own dot product: (rho (32 + 68 + 1) + 8192 u64) sum_chunk |G W|.
All-zero layer: v = u = 0 and sigma = 0 through the eps clamp, weight_sn = 0 / 0 = NaN, as torch.  A layer holding a NaN is non-finite
where the float64 reference is (torch's clamp_min keeps a NaN norm), and no neighbouring layer is touched.
Exact family: W = P1 H P2 D, H the Sylvester-Hadamard matrix of order n = 4^k, P permutations, D column signs, u_in = 1/2: W^T u = +-
n/2 e_k, every norm a power of two, sigma = sqrt(n); G small integers whose <G, W> is a multiple of n.
"""
import math

import torch

import step_bounds as sb
from step_bounds import U64, SAFETY, ceil_div

ELEM_CHUNK, SN_MAX_LAYERS = 8192, 32
UNIT = {torch.float32: sb.U32, torch.float64: U64}
SN_SHAPES = [(1, 1), (3, 27), (5, 1120), (257, 65), (16, 512), (1, 8193), (8193, 1), (4, 4608), (1024, 576)]
SN_FAMILIES = ("normal", "scale_lo", "scale_hi", "zero", "nan")
SN_COUNTS = (1, 32, 33, 65)
SN_TINY = [(1, 1), (3, 27), (2, 3), (4, 5)]
SN_MULTI = (257, 65)                       # 3 chunks
SN_EXACT_ORDERS = (4, 16, 64, 256)
SN_EPS = 1e-12
SN_MUTANTS = ("sigma_from_old_u", "no_eps_clamp", "first_partial_only", "transposed_outer", "coef_over_sigma", "wv_slice_overlap")


class Layer:
    def __init__(self, W, u, v, family):
        self.W, self.u, self.v, self.family = W.contiguous(), u.contiguous(), v.contiguous(), family
        self.rows, self.cols = W.shape
        self.chunks = ceil_div(self.rows * self.cols, ELEM_CHUNK)


def make_layer(rows, cols, family="normal", dtype=torch.float32, seed=0):
    gen = torch.Generator().manual_seed(3000 + seed + 7 * rows + cols)
    W = torch.randn(rows, cols, generator=gen, dtype=torch.float64) * 0.1
    W = W + torch.where(W < 0, -0.05, 0.05)                  # no entry so small that a 1 x 1 layer's square leaves the claimed range
    u = torch.nn.functional.normalize(torch.randn(rows, generator=gen, dtype=torch.float64), dim=0)
    v = torch.nn.functional.normalize(torch.randn(cols, generator=gen, dtype=torch.float64), dim=0)
    if family == "scale_lo":
        W = W * 2.0 ** -40
    elif family == "scale_hi":
        W = W * 2.0 ** 40
    elif family == "zero":
        W = torch.zeros_like(W)
    elif family == "nan":
        W[rows // 2, cols // 2] = sb.NAN
    return Layer(W.to(dtype), u.to(dtype), v.to(dtype), family)


def make_grad(layer, seed=0):
    gen = torch.Generator().manual_seed(3500 + seed + layer.rows + 3 * layer.cols)
    return (torch.randn(layer.rows, layer.cols, generator=gen, dtype=torch.float64) * 0.3).to(layer.W.dtype)


def hadamard(n):
    H = torch.ones(1, 1, dtype=torch.float64)
    while H.shape[0] < n:
        H = torch.cat([torch.cat([H, H], 1), torch.cat([H, -H], 1)], 0)
    return H


def make_exact_layer(n, dtype=torch.float32, seed=0):
    """-> the layer and an integer G with <G, W> a multiple of n."""
    if n < 4 or 4 ** round(math.log(n, 4)) != n:
        raise ValueError("exact family: %d is not a power of 4" % n)
    gen = torch.Generator().manual_seed(3900 + seed + n)
    D = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
    W = hadamard(n)[torch.randperm(n, generator=gen)][:, torch.randperm(n, generator=gen)] * D
    G = torch.randint(-2, 3, (n, n), generator=gen).double()
    r = int((G * W).sum()) % n
    flat = G.view(-1)
    for k in range(r):                                      # lower <G, W> by r: one from r different elements
        flat[k] -= W.view(-1)[k]
    layer = Layer(W.to(dtype), torch.full((n,), 0.5, dtype=dtype), torch.full((n,), 0.25, dtype=dtype), "exact")
    return layer, G.to(dtype)


# ------------------------------------------------------------------------------------------------ the references
def _clamped(nrm, eps):
    """max(nrm, eps) that keeps a NaN, as torch.clamp_min."""
    return torch.where(torch.isnan(nrm), nrm, nrm.clamp_min(eps))


def _squares_in_range(x, what, dtype):
    if dtype == torch.float32:
        ss = float((x * x).sum())
        if math.isfinite(ss) and ss != 0 and not x.numel() * 2.0 ** -102 <= ss <= 2.0 ** 120:
            raise ValueError("%s: sum of squares %.3g leaves the range in which anything is claimed for float32" % (what, ss))


def check_forward(ck, layer, out, power_iterations, eps=SN_EPS, safety=SAFETY, saved=True):
    """out: dict of the kernel's v, wv, u, sigma, weight_sn (, u_saved, v_saved) as CPU tensors of the layer's dtype."""
    dt, fam = layer.W.dtype, layer.family
    unit, rho = UNIT[dt], safety * UNIT[dt]
    rows, cols = layer.rows, layer.cols
    eps = sb.f32(eps) if dt == torch.float32 else eps
    W, uin, vin = layer.W.double(), layer.u.double(), layer.v.double()
    vk, wvk, uk, sk = out["v"].double(), out["wv"].double(), out["u"].double(), out["sigma"].double().reshape(())
    exact = fam == "exact"

    def cmp(stage, got, ref, bound):
        if exact:
            ck.equal(stage, fam, got, sb.require_exact(ref, stage, dt).to(dt))
        else:
            ck.bounded(stage, fam, got, ref, bound)
    if power_iterations:
        v_raw = W.t() @ uin
        _squares_in_range(v_raw, "v_raw", dt)
        delta = (rho * (ceil_div(rows, 4) + 4 + 1) + rows * U64) * (W.abs().t() @ uin.abs())
        d = _clamped(v_raw.norm(), eps)
        rn = rho * (0.5 * (ceil_div(cols, 256) + 68 + 1) + 1) + cols * U64
        v_ref = v_raw / d
        cmp("v", out["v"], v_ref, delta / d + v_ref.abs() * (delta.norm() / d + rn + rho))
        v_use = vk
    else:
        ck.equal("v", fam, out["v"], layer.v)
        ck.equal("u", fam, out["u"], layer.u)
        v_use = vin
    cmp("wv", out["wv"], W @ v_use, (rho * (ceil_div(cols, 64) + 64 + 2) + cols * U64) * (W.abs() @ v_use.abs()))
    if power_iterations:
        _squares_in_range(wvk, "wv", dt)
        u_ref = wvk / _clamped(wvk.norm(), eps)
        cmp("u", out["u"], u_ref, u_ref.abs() * (rho * (0.5 * (ceil_div(rows, 256) + 69) + 2) + rows * U64))
    cmp("sigma", out["sigma"].reshape(()), (uk * wvk).sum(), (rho * (ceil_div(rows, 256) + 68 + 1) + rows * U64) * (uk * wvk).abs().sum())
    w_ref = W / sk
    cmp("weight_sn", out["weight_sn"], w_ref, (unit + U64) * w_ref.abs())
    if saved:
        ck.equal("u_saved", fam, out["u_saved"], out["u"])
        ck.equal("v_saved", fam, out["v_saved"], out["v"])


def check_backward(ck, layer, G, u, v, sigma, dW, partials, safety=SAFETY):
    """u, v, sigma: what the backward entry was given (the forward kernel's); dW [rows, cols], partials [chunks]."""
    dt, fam = layer.W.dtype, layer.family
    rho = safety * UNIT[dt]
    n = layer.rows * layer.cols
    W, Gd, ud, vd, s = layer.W.double(), G.double(), u.double(), v.double(), sigma.double().reshape(())
    gw = (Gd * W).reshape(-1)
    pad = torch.cat([gw, torch.zeros(layer.chunks * ELEM_CHUNK - n, dtype=torch.float64)]).view(layer.chunks, ELEM_CHUNK)
    L1 = ceil_div(min(n, ELEM_CHUNK), 256)
    p_ref, p_bound = pad.sum(1), (rho * (L1 + 68 + 1) + ELEM_CHUNK * U64) * pad.abs().sum(1)
    L, P = L1 + ceil_div(layer.chunks, 256), 136
    ref = Gd / s - (gw.sum() / (s * s)) * torch.outer(ud, vd)
    mag = Gd.abs() / s.abs() + (gw.abs().sum() / (s * s)) * torch.outer(ud.abs(), vd.abs())
    if fam == "exact":
        ck.equal("partials", fam, partials, sb.require_exact(p_ref, "partials", dt).to(dt))
        ck.equal("dW", fam, dW, sb.require_exact(ref, "dW", dt).to(dt))
    else:
        ck.bounded("partials", fam, partials, p_ref, p_bound)
        ck.bounded("dW", fam, dW, ref, (rho * (L + P + 8) + n * U64) * mag)


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic in torch
def _sumsq(x):
    return sb.block_sum(sb.chain_sum(x * x, 256))


def emulate_forward(layers, power_iterations, eps=SN_EPS, mutant=None, saved=True):
    """The three phases over ALL layers with one shared wv buffer, in the layers' dtype -> list of output dicts."""
    dt = layers[0].W.dtype
    eps_t = torch.tensor(eps, dtype=dt)
    off, offs = 0, []
    for k, L in enumerate(layers):
        offs.append(off - (1 if (mutant == "wv_slice_overlap" and k > 0) else 0))
        off += L.rows
    wv_buf = torch.full((off,), sb.NAN, dtype=dt)

    def clamp(nrm):
        if mutant == "no_eps_clamp":
            return nrm
        return torch.where(nrm < eps_t, eps_t, nrm)
    v_raws, nrms = [], []
    for L in layers:                                                            # phase 1, and the norm phases 2 and 3 recompute
        if power_iterations:
            prod = L.W * L.u[:, None]                                           # [rows, cols]
            per_wave = sb.chain_sum(prod.t().contiguous(), 4)                   # [cols, 4]: wave w adds rows w, w + 4, ...
            v_raw = ((per_wave[:, 0] + per_wave[:, 1]) + per_wave[:, 2]) + per_wave[:, 3]
            v_raws.append(v_raw)
            nrms.append(clamp(torch.sqrt(_sumsq(v_raw))))
        else:
            v_raws.append(L.v)
            nrms.append(torch.tensor(1.0, dtype=dt))
    for L, o, v_raw, nrm in zip(layers, offs, v_raws, nrms):                   # phase 2
        terms = L.W * (v_raw / nrm)[None, :]
        wv_buf[o:o + L.rows] = sb.tree_sum(sb.chain_sum(terms, 64))
    outs = []
    for L, o, v_raw, nrm in zip(layers, offs, v_raws, nrms):                   # phase 3
        wv = wv_buf[o:o + L.rows].clone()
        if power_iterations:
            unrm = clamp(torch.sqrt(_sumsq(wv)))
            u = wv / unrm
            sig_u = L.u if mutant == "sigma_from_old_u" else u
            v = v_raw / nrm
        else:
            u, v, sig_u = L.u, L.v, L.u
        sigma = sb.block_sum(sb.chain_sum(sig_u * wv, 256))
        out = {"v": v, "wv": wv, "u": u, "sigma": sigma.reshape(1), "weight_sn": L.W / sigma}
        if saved:
            out["u_saved"], out["v_saved"] = u.clone(), v.clone()
        outs.append(out)
    return outs


def emulate_backward(layer, G, u, v, sigma, mutant=None):
    n = layer.rows * layer.cols
    gw = (G * layer.W).reshape(-1)
    pad = torch.cat([gw, torch.zeros(layer.chunks * ELEM_CHUNK - n, dtype=gw.dtype)]).view(layer.chunks, ELEM_CHUNK)
    partials = sb.block_sum(sb.chain_sum(pad, 256))
    used = partials[:1] if mutant == "first_partial_only" else partials
    s = sigma.reshape(())
    coef = sb.block_sum(sb.chain_sum(used, 256)) / (s if mutant == "coef_over_sigma" else s * s)
    outer = torch.outer(u, v)
    if mutant == "transposed_outer":
        outer = torch.outer(v, u).reshape(-1)[:n].view(layer.rows, layer.cols) if layer.rows != layer.cols else torch.outer(v, u)
    return G / s - coef * outer, partials


# ------------------------------------------------------------------------------------------------ the matrix
def family_layers(shape, dtype, seed=0):
    """One layer per family of one shape: five neighbours in a single call."""
    return [make_layer(shape[0], shape[1], f, dtype, seed + k) for k, f in enumerate(SN_FAMILIES)]


def count_layers(count, multi_first, dtype=torch.float32):
    """`count` layers: tiny ones and the multi-chunk layer first or last."""
    tiny = [make_layer(*SN_TINY[k % len(SN_TINY)], "normal", dtype, 50 + k) for k in range(count - 1)]
    multi = make_layer(*SN_MULTI, "normal", dtype, 49)
    return [multi] + tiny if multi_first else tiny + [multi]
