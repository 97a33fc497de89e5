"""tests/colmax_split_bounds.py judged without a GPU: the torch restatement of the split correlation maximum (bfloat16 casts, three
fp32 matrix products) meets the bound with SAFETY = 1 at every shape of the GPU matrix, and the exact family bit for bit; each mutant
of the restatement misses an assertion; the interface (header, exports, ABI version, the precision keyword of ops,
PerceptualCorrectness and FlowNetTrainer) is there and validates its argument before it looks at the device."""
import inspect
import os
import re

import pytest
import torch

import colmax_split_bounds as cs
import step_bounds as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["B%d-N%d-C%d" % s for s in cs.SPLIT_SHAPES]


def _fails(fn):
    try:
        fn()
    except AssertionError as e:
        return str(e)
    return None


# ================================================================================================ (a) restatement against the bound
@pytest.mark.parametrize("family", cs.SPLIT_FAMILIES)
@pytest.mark.parametrize("shape", cs.SPLIT_SHAPES, ids=IDS)
def test_restatement_meets_the_bound_without_the_safety_factor(shape, family):
    s, t = cs.split_inputs(*shape, family=family)
    ck = sb.Checks("split %s %s" % (shape, family))
    cs.SplitRef(s, t, 1.0).check(ck, cs.split_emulate(s, t), family=family)
    ck.finish(verbose=False)


def test_the_bound_is_the_formula_of_the_docstring():
    """One product, by hand: C = 64, s t = 1/64 in every k."""
    s, t = torch.full((1, 1, 64), 0.125), torch.full((1, 64, 1), 0.125)
    want = (2.0 ** -16 + 4 * 192 * 2.0 ** -24 * (1 + 2.0 ** -6) + 64 * 2.0 ** -53) * 1.0 + 2.0 ** -126 * (3 * 16 + 6 * 64)
    assert abs(float(cs.SplitRef(s, t).bound) / want - 1) < 1e-12 and float(cs.SplitRef(s, t).out) == 1.0


def test_a_value_of_2_to_the_127_is_outside_the_contract():
    s, t = cs.split_inputs(1, 33, 64)
    s[0, 0, 0] = 2.0 ** 127
    with pytest.raises(ValueError):
        cs.SplitRef(s, t)


# ================================================================================================ (b) exact family
@pytest.mark.parametrize("shape", cs.SPLIT_SHAPES, ids=IDS)
def test_exact_family_bit_for_bit_and_it_exercises_lo(shape):
    _, N, C = shape
    s, t, planted = cs.split_exact_inputs(N, C)
    three, full = cs.split_exact_reference(s, t, planted)
    assert torch.equal(cs.split_emulate(s, t).double(), three)
    assert bool((three != full).any()), "the family never meets lo lo: it would not tell three terms from the full product"
    for _, j in planted:
        assert float(full[0, j] - three[0, j]) == 4.0              # sum lo lo of a planted pair
    assert len(planted) >= 3 and int((s != 0).sum(2).max()) <= 4 and int((t != 0).sum(1).max()) <= 4


def test_require_exact_raises_on_an_unrepresentable_family():
    s, t, _ = cs.split_exact_inputs(33, 64)
    with pytest.raises(ValueError):
        cs.split_exact_reference(s * (1 + 2.0 ** -12), t)          # x is no longer hi + lo
    with pytest.raises(ValueError):
        cs.split_exact_reference(s * 64, t * 64)                   # product sums beyond 2^24
    with pytest.raises(ValueError):
        cs.split_exact_reference(s, t, [(1, 0)])                   # not a planted maximum


# ================================================================================================ (c) mutants
@pytest.mark.parametrize("mutant", cs.SPLIT_MUTANTS)
def test_every_mutant_misses_the_exact_family(mutant):
    for (_, N, C) in cs.SPLIT_SHAPES:
        s, t, planted = cs.split_exact_inputs(N, C)
        three, _ = cs.split_exact_reference(s, t, planted)
        assert not torch.equal(cs.split_emulate(s, t, mutant).double(), three), (mutant, N, C)


@pytest.mark.parametrize("family", cs.SPLIT_FAMILIES)
@pytest.mark.parametrize("mutant", cs.SPLIT_MUTANTS)
def test_every_mutant_misses_the_bound_at_the_full_safety(mutant, family):
    """A dropped or mispaired term errs by ~2^-9 / sqrt(C) of sum |s t|: beyond the bound at C = 64; a single bf16 pass everywhere."""
    shapes = cs.SPLIT_SHAPES if mutant == "single_bf16" else [sh for sh in cs.SPLIT_SHAPES if sh[2] == 64]
    for shape in shapes:
        s, t = cs.split_inputs(*shape, family=family)
        ck = sb.Checks("split %s %s" % (mutant, shape))
        cs.SplitRef(s, t).check(ck, cs.split_emulate(s, t, mutant), family=family)
        assert _fails(lambda: ck.finish(verbose=False)), (mutant, shape)


@pytest.mark.parametrize("case", cs.NONFINITE_CASES)
def test_nonfinite_contract_of_the_restatement(case):
    s, t = cs.split_nonfinite_inputs(case)
    ck = sb.Checks("split non-finite " + case)
    cs.split_nonfinite_check(ck, case, s, t, cs.split_emulate(s, t))
    ck.finish(verbose=False)
    # the fp32 contract (an infinity stays an infinity) is a different one: the plain product misses this check
    if case.startswith("inf"):
        ck = sb.Checks("fp32 contract " + case)
        cs.split_nonfinite_check(ck, case, s, t, torch.bmm(s, t).max(1)[0])
        assert _fails(lambda: ck.finish(verbose=False))


# ================================================================================================ (d) interface
def test_the_symbol_is_declared_exported_and_the_abi_version_stays():
    from ffwm_amd import _lib
    header = open(os.path.join(ROOT, "include", "ffwm_hip.h")).read()
    decl = re.search(r"int\s+ffwm_correlation_colmax_split\s*\(([^)]*)\)\s*;", header)
    assert decl, "ffwm_correlation_colmax_split is not declared in include/ffwm_hip.h"
    fp32 = re.search(r"int\s+ffwm_correlation_colmax\s*\(([^)]*)\)\s*;", header)
    assert re.sub(r"\s+", " ", decl.group(1)) == re.sub(r"\s+", " ", fp32.group(1))          # the same argument list
    assert "ffwm_correlation_colmax_split" in _lib.EXPORTS
    assert _lib._SIGNATURES["ffwm_correlation_colmax_split"] == _lib._SIGNATURES["ffwm_correlation_colmax"]
    assert _lib.ABI_VERSION == 5 and re.search(r"#define\s+FFWM_ABI_VERSION\s+5\b", header)
    assert _lib.load().ffwm_abi_version() == 5
    assert hasattr(_lib.load(), "ffwm_correlation_colmax_split")


def test_the_entry_checks_its_arguments_like_the_fp32_entry():
    """No launch: every call below is refused on the host."""
    from ffwm_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64 * 64)
    p = buf.data_ptr()
    for args in ((p, p, p, 1, 64, 64, _lib.F64, None), (None, p, p, 1, 64, 64, _lib.F32, None), (p, p, p, 0, 64, 64, _lib.F32, None),
                 (p, p, p, 1, 64, 96, _lib.F32, None), (p, p, p, 1, 1 << 30, 64, _lib.F32, None)):
        a, b = lib.ffwm_correlation_colmax_split(*args), lib.ffwm_correlation_colmax(*args)
        assert a == b and a != 0, args


def test_ops_rejects_an_unknown_precision_before_the_device_check():
    from ffwm_amd import ops
    s, t = cs.split_inputs(1, 33, 64)
    with pytest.raises(ValueError):
        ops.correlation_colmax(s, t, precision="x")
    with pytest.raises(NotImplementedError):                       # a known precision reaches the device check
        ops.correlation_colmax(s, t, precision="bf16x3")
    assert inspect.signature(ops.correlation_colmax).parameters["precision"].default == "fp32"


def _cpu_module(**kw):
    from ffwm_amd.losses import PerceptualCorrectness

    def warp(source, flow):
        grid = flow.permute(0, 2, 3, 1)
        return torch.nn.functional.grid_sample(source, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    pc = PerceptualCorrectness(None, warp, **kw)
    gen = torch.Generator().manual_seed(3)
    pc.target_vgg = {"x": torch.rand(2, 64, 8, 8, generator=gen) + 0.1}
    pc.source_vgg = {"x": torch.rand(2, 64, 8, 8, generator=gen) + 0.1}
    flow = (torch.rand(2, 2, 8, 8, generator=gen) * 2 - 1).requires_grad_(True)
    mask = (torch.rand(2, 1, 8, 8, generator=gen) < 0.6).float()
    return pc, flow, mask


def test_perceptual_correctness_validates_in_the_constructor_and_cpu_takes_bmm():
    from ffwm_amd import trainer
    from ffwm_amd.losses import PerceptualCorrectness
    with pytest.raises(ValueError):
        _cpu_module(corr_precision="x")
    assert inspect.signature(PerceptualCorrectness.__init__).parameters["corr_precision"].default == "fp32"
    assert inspect.signature(trainer.FlowNetTrainer.__init__).parameters["corr_precision"].default == "fp32"
    got = {}
    for prec in ("fp32", "bf16x3"):
        pc, flow, mask = _cpu_module(corr_precision=prec)
        assert pc.corr_precision == prec
        loss = pc.calculate_loss(flow, "x", mask, use_bilinear_sampling=True)
        loss.backward()
        got[prec] = (loss.detach(), flow.grad.clone())
    assert torch.equal(got["fp32"][0], got["bf16x3"][0]) and torch.equal(got["fp32"][1], got["bf16x3"][1])
    assert bool(torch.isfinite(got["fp32"][0])) and float(got["fp32"][1].abs().max()) > 0
