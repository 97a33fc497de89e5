"""Float64 error bound, exact family, non-finite contract and torch restatement of the split correlation maximum
(ffwm_correlation_colmax_split, csrc/correlation.hip): a plain helper module, not a conftest.

Conventions of step_bounds.py: every reference is float64 torch on the CPU, computed from what the kernel is GIVEN; u = 2^-24, u64 =
2^-53; SAFETY = 4 multiplies every count of roundings; no constant is fitted.

The kernel.  Every operand element x (finite fp32) is split in two bf16 terms, hi = bf16_rn(x), lo = bf16_rn(x - hi), and a product
sum is formed on v_mfma_f32_32x32x16_bf16 as  sum_k (s_lo t_hi + s_hi t_lo + s_hi t_hi)  in one fp32 accumulator.

The split.  bf16 keeps 8 significand bits, unit roundoff 2^-9:
    |x - hi| <= 2^-9 |x|, and x - hi is a multiple of ulp32(x) no larger than 2^-9 |x|: it is EXACT in fp32 (denormals included);
    lo = bf16_rn(x - hi):   |x - hi - lo| <= 2^-9 |x - hi| <= 2^-18 |x|;    |hi| <= (1 + 2^-9) |x|,  |lo| <= 2^-9 (1 + 2^-9) |x|.
  Write s = sh + sl + es, t = th + tl + et with |es| <= 2^-18 |s|, |et| <= 2^-18 |t|.  Then
    s t - (sl th + sh tl + sh th) = sl tl + es t + (s - es) et,
    |sl tl| <= 2^-18 (1 + 2^-9)^2 |s t|,   |es t| <= 2^-18 |s t|,   |(s - es) et| <= 2^-18 (1 + 2^-18) |s t|:
  the terms the kernel never sees are bounded by 3 x 2^-18 (1 + 2^-8) |s t| <= 2^-16 |s t| per product        (TRUNC = 2^-16).
The accumulation.  The 3 C partial products are exact in fp32 (8 x 8 significand bits).  The ISA does not document the order or the
  internal width in which the instruction adds its 16 products to the accumulator, so the sum is charged as 3 C fp32 roundings in
  any order (rule (S) of step_bounds.py): gamma = 3 C u / (1 - 3 C u) on sum |terms|, and
    sum |terms| <= (1 + 2^-9)^2 (1 + 2^-8) sum |s t|;   with 3 C u <= 2^-14 the two factors together stay below  MAG = 1 + 2^-6.
  The float64 reference's own sum of C terms errs by C u64 sum |s t|.
Underflow, stated, not silent.  A bf16 term, a product or a partial sum below 2^-126 may be flushed to zero (bf16 has fp32's exponent
  range; the matrix core's denormal handling is not documented): per k at most the four operand terms, each costing 2^-126 times the
  other operand's magnitude, (1 + 2^-9) <= 1.5 folded in; and 3 C products and 3 C partial sums of at most 2^-126 each:
    ETA_ij = 2^-126 (3 sum_k (|s_ik| + |t_kj|) + 6 C)                (~1e-36 on normalised features).
Together
    |prod_ij - ref_ij| <= (2^-16 + SAFETY 3 C u MAG + C u64) sum_k |s_ik t_kj| + ETA_ij,
  and the maximum is 1-Lipschitz: the bound of out[b, j] is the largest of these over i.  At C = 64 that is 6.2e-5 sum |s t| (SAFETY
  = 4; 2.7e-5 with SAFETY = 1), against 1.5e-5 of the fp32 kernel's SAFETY C u.

Non-finite contract (it DIFFERS from ffwm_correlation_colmax).  A NaN in source row i makes out[b, :] NaN, a NaN in target column j
  makes out[b, j] NaN alone.  An infinite operand has hi = inf, lo = bf16(inf - inf) = NaN: it behaves as a NaN in its row or
  column.  The reference is therefore taken from the operands with every infinity replaced by NaN.  Finite |x| >= 2^127 may round
  to an infinite hi: outside the contract, SplitRef raises.

Exact family.  Operands 256 p + q with small integers p, q, at most 4 non-zeros per source row and per target column: hi, lo (a
  small integer) and every partial sum are exact, x = hi + lo, so the kernel's value is EXACTLY sum (hi hi + hi lo + lo hi) = s t -
  sum lo lo; require_exact proves the representability, and the planted maxima carry lo lo != 0, so the full product is a different
  number: a kernel that computed more (or less) than the three terms misses the comparison.

tests/test_colmax_split_cpu.py: the restatement split_emulate meets the bound with SAFETY = 1 and the exact family bit for bit, and
each mutant of it misses an assertion.
"""
import math

import torch

import step_bounds as sb
from step_bounds import NAN, SAFETY, U32, U64

TRUNC = 2.0 ** -16
MAG = 1.0 + 2.0 ** -6
TINY = 2.0 ** -126
# (B, N, C): ragged row tile and ragged column tile; two column tiles at C = 128; N below one column tile; one row past a tile
SPLIT_SHAPES = [(2, 200, 64), (1, 160, 128), (2, 96, 256), (1, 33, 64)]
SPLIT_FAMILIES = ("signed", "positive")
SPLIT_MUTANTS = ("lo_hi_dropped", "hi_lo_dropped", "single_bf16", "lo_wrong_operand")
NONFINITE_CASES = ("nan_source_row", "nan_target_column", "inf_source_row", "inf_target_column")


def split_inputs(B, N, C, family="signed", seed=0):
    """Normalised random features as PerceptualCorrectness hands them over: source [B, N, C] with unit rows, target [B, C, N] with unit
    columns; "positive" = post-ReLU-like features (every product positive: no cancellation, the maxima near 1)."""
    gen = torch.Generator().manual_seed(6100 + seed + 17 * N + C + (1000 if family == "positive" else 0))
    if family == "positive":
        s, t = torch.rand(B, N, C, generator=gen) + 0.1, torch.rand(B, C, N, generator=gen) + 0.1
    else:
        s, t = torch.randn(B, N, C, generator=gen), torch.randn(B, C, N, generator=gen)
    s = s / (s.norm(dim=2, keepdim=True) + 1e-8)
    t = t / (t.norm(dim=1, keepdim=True) + 1e-8)
    return s.contiguous(), t.contiguous()


def split_terms(x):
    """-> hi, lo as float32 tensors holding the bf16 values (round to nearest even, as v_cvt_pk_bf16_f32)."""
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi, lo


class SplitRef:
    def __init__(self, s, t, safety=SAFETY):
        C = s.shape[2]
        for x, what in ((s, "source"), (t, "target")):
            fin = torch.isfinite(x)
            if bool((x[fin].abs() >= 2.0 ** 127).any()):
                raise ValueError("split colmax: a finite %s value of 2^127 or more is outside the contract" % what)
        sd = torch.where(torch.isinf(s), torch.full_like(s, NAN), s).double()          # an infinity counts as a NaN (lo = NaN)
        td = torch.where(torch.isinf(t), torch.full_like(t, NAN), t).double()
        self.out = torch.bmm(sd, td).max(1)[0]
        mag = torch.bmm(sd.abs(), td.abs())
        eta = TINY * (3.0 * (sd.abs().sum(2, keepdim=True) + td.abs().sum(1, keepdim=True)) + 6.0 * C)
        self.bound = ((TRUNC + safety * 3 * C * U32 * MAG + C * U64) * mag + eta).max(1)[0]
        self.bound = torch.where(torch.isfinite(self.bound), self.bound, torch.zeros_like(self.bound))

    def check(self, ck, out, family="normal", per_sample=None):
        B, N = self.out.shape
        if out.numel() > B * N:
            sb.check_guards(out.reshape(-1), B * N, ck.what + " out")
        got = out.detach().cpu().reshape(-1)[:B * N].view(B, N)
        for b in range(B):
            ck.bounded("colmax_split", per_sample[b] if per_sample else family, got[b], self.out[b], self.bound[b])


def split_emulate(s, t, mutant=None):
    """The kernel's arithmetic in torch: bfloat16 casts, three fp32 matrix products added in fp32, torch.max (which keeps a NaN)."""
    sh, sl = split_terms(s)
    th, tl = split_terms(t)
    if mutant == "single_bf16":
        return torch.bmm(sh, th).max(1)[0]
    lo_hi = torch.bmm(sl, tl if mutant == "lo_wrong_operand" else th)
    hi_lo = torch.bmm(sh, tl)
    hi_hi = torch.bmm(sh, th)
    if mutant == "lo_hi_dropped":
        return (hi_lo + hi_hi).max(1)[0]
    if mutant == "hi_lo_dropped":
        return (lo_hi + hi_hi).max(1)[0]
    return ((lo_hi + hi_lo) + hi_hi).max(1)[0]


# ------------------------------------------------------------------------------------------------ exact family
_PLANT = (257.0, -257.0, 515.0, 259.0)        # hi = 256, -256, 516, 260; lo = 1, -1, -1, -1: sum lo lo = 4 on a planted pair


def split_exact_inputs(N, C, seed=0):
    """Operands 256 p + q (p = +-1, q in -3..3; 0 elsewhere), <= 4 non-zeros per source row and target column; the arg-max row of one
    column each is planted (values _PLANT on both sides, 464404 > 4 x 259^2) at row 0, row N - 1, rows of both halves of the MFMA C/D
    layout and in the ragged last tile.  -> s [1, N, C], t [1, C, N], the planted (row, column) pairs."""
    gen = torch.Generator().manual_seed(8900 + seed + N + C)

    def values():
        p = torch.randint(0, 2, (4,), generator=gen).float() * 2 - 1
        return 256.0 * p + torch.randint(-3, 4, (4,), generator=gen).float()
    s, t = torch.zeros(N, C), torch.zeros(C, N)
    for i in range(N):
        s[i, torch.randperm(C, generator=gen)[:4]] = values()
        t[torch.randperm(C, generator=gen)[:4], i] = values()
    rows = sorted({0, N - 1, min(5, N - 1), min(34, N - 1), (N - 1) // 32 * 32, N // 2})
    cols = [(7 * k + N // 3) % N for k in range(len(rows))]
    planted = []
    for i, j in zip(rows, cols):
        if j in [c for _, c in planted]:
            continue
        ks = torch.randperm(C, generator=gen)[:4]
        t[:, j] = 0
        t[ks, j] = torch.tensor(_PLANT)
        s[i] = 0
        s[i, ks] = torch.tensor(_PLANT)
        planted.append((i, j))
    return s.unsqueeze(0).contiguous(), t.unsqueeze(0).contiguous(), planted


def split_exact_reference(s, t, planted=()):
    """-> (three-term maximum, full-product maximum), both float64 and proven exact in float32; raises unless x = hi + lo exactly,
    every product sum is representable and each planted row is the only maximum of its column."""
    sh, sl = split_terms(s)
    th, tl = split_terms(t)
    for x, hi, lo, what in ((s, sh, sl, "source"), (t, th, tl, "target")):
        if not torch.equal(hi.double() + lo.double(), x.double()):
            raise ValueError("split exact family: %s is not hi + lo exactly" % what)
    sh, sl, th, tl = sh.double(), sl.double(), th.double(), tl.double()
    three = torch.bmm(sl, th) + torch.bmm(sh, tl) + torch.bmm(sh, th)
    full = torch.bmm(s.double(), t.double())
    if not torch.equal(full - three, torch.bmm(sl, tl)):
        raise ValueError("split exact family: the three terms and lo lo do not add up to the product")
    C = s.shape[2]
    # every partial sum of any order is an integer below 2^24: sum |terms| bounds them all
    if float(torch.bmm(s.double().abs(), t.double().abs()).max()) * (1 + 2.0 ** -6) >= 2.0 ** 24 or C > 256:
        raise ValueError("split exact family: a partial sum may leave the exact integers of float32")
    sb.require_exact(three, "split exact family (three terms)")
    sb.require_exact(full, "split exact family (full product)")
    for i, j in planted:
        col = three[0, :, j]
        if int(col.argmax()) != i or int((col == col.max()).sum()) != 1:
            raise ValueError("split exact family: the planted row %d is not the only maximum of column %d" % (i, j))
    return three.max(1)[0], full.max(1)[0]


# ------------------------------------------------------------------------------------------------ non-finite contract
def split_nonfinite_inputs(case, N=33, C=64):
    """A batch of two: sample 0 carries the defect (row 3 of the source or column 5 of the target), sample 1 is untouched."""
    s, t = split_inputs(2, N, C, "signed", seed=5)
    bad = NAN if case.startswith("nan") else (math.inf if case.endswith("row") else -math.inf)
    if case.endswith("source_row"):
        s[0, 3 % N, 10] = bad
    else:
        t[0, 20, 5 % N] = bad
    return s, t


def split_nonfinite_check(ck, case, s, t, out):
    N = s.shape[1]
    ref = SplitRef(s, t)
    want_nan = torch.zeros(2, N, dtype=torch.bool)
    if case.endswith("source_row"):
        want_nan[0] = True
    else:
        want_nan[0, 5 % N] = True
    assert torch.equal(torch.isnan(ref.out), want_nan) and bool(torch.isfinite(ref.out[~want_nan]).all())      # the reference itself
    ref.check(ck, out, per_sample=[case, "untouched"])
