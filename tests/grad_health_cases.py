"""Cases, the float64 restatement and the bounds for the gradient-health pass (csrc/grad_health.hip, ffwm_grad_health) and the scale of
the guarded Adam step (csrc/adam.hip) -- a plain helper module, not a conftest.

Restatement, per segment of the float32 array: the squares of the FINITE elements are exact in float64 (24-bit significands: 48 bits,
and 1e-45^2 is far inside the range), S_ref = math.fsum of them is their correctly rounded sum; the maximum of |g| over the finite
elements, the count of non-finite elements and the element count are exact integers / floats.

Bounds (u = 2^-53):
    sum      every term is >= 0, so a float64 sum of m terms in ANY order is within (m - 1) u of the exact sum, relatively (the kernel's
             extra additions are of exact zeros: idle lanes, non-finite elements, accumulators that start at 0); fsum adds half an ulp:
                 |S - S_ref| <= m u S_ref                     m = the finite elements of the segment; m = 0 or S_ref = 0: S = 0 exactly
    maximum, non-finite count, element count: exact.
    scale    the kernel evaluates optim.clip_coefficient on the record's own sums in double (its sqrt and division are within an ulp
             of double, ~1e-16) and rounds ONCE to float32: within one float32 ulp of clip_coefficient(total, max_norm).

Every case is the smallest shape at which one part of the kernel can go wrong; CHUNK is the kernel's chunk length, imported from the
one place the package states it.
"""
import math

import torch

from ffwm_amd.ops import GRAD_HEALTH_CHUNK as CHUNK
from ffwm_amd.ops import GRAD_HEALTH_MAX_SEGMENTS as MAX_SEGMENTS

U64 = 2.0 ** -53
NAN, INF = float("nan"), float("inf")
KINDS = {"nan": NAN, "pinf": INF, "ninf": -INF}


class Case:
    def __init__(self, name, g, seg_end):
        assert g.dtype == torch.float32 and g.dim() == 1 and seg_end[-1] == g.numel() and list(seg_end) == sorted(seg_end)
        assert all(e % 4 == 0 for e in seg_end[:-1]) and 1 <= len(seg_end) <= MAX_SEGMENTS
        self.name, self.g, self.seg_end, self.n = name, g, list(seg_end), g.numel()
        self._ref = None

    def __repr__(self):
        return "%s-n%d-s%d" % (self.name, self.n, len(self.seg_end))

    @property
    def ref(self):
        """Computed once, shared by every test that needs it."""
        if self._ref is None:
            self._ref = reference(self.g, self.seg_end)
        return self._ref


def reference(g, seg_end):
    """-> per segment a dict: sum (fsum of the exact squares of the finite elements), max, nonfinite, n, m (finite elements)."""
    out, a = [], 0
    g64 = g.double()
    for e in seg_end:
        x = g64[a:e]
        fin = torch.isfinite(x)
        xf = x[fin]
        out.append({"sum": math.fsum((xf * xf).tolist()), "max": float(xf.abs().max()) if xf.numel() else 0.0,
                    "nonfinite": int((~fin).sum()), "n": e - a, "m": int(fin.sum())})
        a = e
    return out


def check_record(case, record, verbose=True):
    """record: [n_seg, 4] (or flat) doubles as the kernel wrote them."""
    rec = record.detach().cpu().double().reshape(-1)[:4 * len(case.seg_end)].view(-1, 4)
    fails = []
    for s, r in enumerate(case.ref):
        S, mx, bad, n = (float(v) for v in rec[s])
        err, bound = abs(S - r["sum"]), r["m"] * U64 * r["sum"]
        if verbose:
            print("GRADHEALTH %r seg %d: sum %.17g ref %.17g err/bound %.3g max %.9g nonfinite %d n %d"
                  % (case, s, S, r["sum"], err / bound if bound else (0.0 if err == 0 else INF), mx, bad, n))
        if not (math.isfinite(S) and err <= bound):
            fails.append("seg %d: |S - S_ref| = %.3g > %.3g" % (s, err, bound))
        if not (mx == r["max"] and math.copysign(1.0, mx) == 1.0):
            fails.append("seg %d: max %r, want %r" % (s, mx, r["max"]))
        if bad != r["nonfinite"] or n != r["n"]:
            fails.append("seg %d: nonfinite %r n %r, want %d %d" % (s, bad, n, r["nonfinite"], r["n"]))
    assert not fails, "%r: %s" % (case, "; ".join(fails))


def record_of(ref):
    """The record a perfect kernel would write, for the restatement's own tests."""
    return torch.tensor([[r["sum"], r["max"], float(r["nonfinite"]), float(r["n"])] for r in ref], dtype=torch.float64)


def _randn(n, seed, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(4100 + seed), dtype=torch.float64) * scale).float()


def cases():
    out = []
    # ---- sizes and segmentation
    for n in (1, 2, 3, 4, 5, 1027, CHUNK + 1, 3 * CHUNK - 3):
        out.append(Case("size", _randn(n, n % 977), [n]))
    out.append(Case("second-pass", _randn(257 * CHUNK + 5, 1, 0.01), [257 * CHUNK + 5]))       # 258 partials: more than 256 threads
    out.append(Case("two-segments", _randn(1027, 2), [516, 1027]))
    n16 = 2 * CHUNK + 7
    ends16 = [4, 8, 8, 40, 1024, 1028, 4096, CHUNK, CHUNK + 4, CHUNK + 8, CHUNK + 512, CHUNK + 516, 2 * CHUNK - 4, 2 * CHUNK, 2 * CHUNK + 4, n16]
    out.append(Case("sixteen-segments", _randn(n16, 3), ends16))                                 # one of them empty
    out.append(Case("four-between-long", _randn(2 * CHUNK + 43, 4), [CHUNK + 8, CHUNK + 12, 2 * CHUNK + 43]))
    out.append(Case("ends-chunk-plus-4", _randn(2 * CHUNK + 2, 5), [CHUNK + 4, 2 * CHUNK + 2]))
    g = _randn(3075, 6)
    g[1024:2048] = 0.0
    out.append(Case("zero-segment", g, [1024, 2048, 3075]))
    # ---- magnitudes
    out.append(Case("uniform-1e-30", torch.full((1027,), 1e-30), [1027]))
    out.append(Case("uniform-1e25", torch.full((1027,), 1e25), [1027]))
    den = (torch.arange(1027) % 97 + 1).float() * 1.4e-45                                       # 1 .. 97 times the smallest denormal
    den[::2] = -den[::2]
    assert float(den.abs().max()) < 1.2e-38 and float(den.abs().min()) > 0
    out.append(Case("denormals", den, [1027]))
    gen = torch.Generator().manual_seed(77)
    mix = (10.0 ** (torch.rand(1027, generator=gen, dtype=torch.float64) * 40 - 20)
           * torch.where(torch.rand(1027, generator=gen) < 0.5, -1.0, 1.0)).float()
    out.append(Case("forty-decades", mix, [516, 1027]))
    out.append(Case("minus-zero", torch.full((1027,), -0.0), [1027]))
    mz = _randn(1027, 8)
    mz[::3] = -0.0
    out.append(Case("minus-zero-mixed", mz, [1027]))
    # ---- non-finite placement: one segment of two chunks and a tail of three
    n = 2 * CHUNK + 7
    places = {"first": 0, "chunk-last": CHUNK - 1, "next-chunk-first": CHUNK, "tail": n - 1}
    for kind, value in KINDS.items():
        for place, at in places.items():
            g = _randn(n, 9)
            g[at] = value
            out.append(Case("%s-%s" % (kind, place), g, [n]))
        g = _randn(2 * CHUNK + 43, 10)
        g[CHUNK + 9] = value
        out.append(Case("%s-in-four" % kind, g, [CHUNK + 8, CHUNK + 12, 2 * CHUNK + 43]))
    g = _randn(3075, 11)
    g[1024:2048] = NAN
    out.append(Case("all-nan-segment", g, [1024, 2048, 3075]))
    return out
