"""tests/step_bounds.py and tests/step_bounds_sn.py judged without a GPU: fp32 (and, for the spectral norm, fp64) torch restatements of
the four kernels' arithmetic -- and torch.optim.Adam -- meet every bound with SAFETY = 1 on the shapes, sizes and families of the GPU
matrix and the exact families bit for bit; each mutant of a restatement misses an assertion at the full SAFETY; the conditions raise
ValueError."""
import math

import pytest
import torch

import step_bounds as sb
import step_bounds_sn as sn


def _fails(fn):
    try:
        fn()
    except AssertionError as e:
        return str(e)
    return None


# ================================================================================================ spectral norm
def _sn_roundtrip(layers, power_iterations, safety, mutant=None, grads=None):
    """Forward restatement of all layers against the per-stage bounds, then the backward from its u, v, sigma."""
    ck = sb.Checks("sn %d layers" % len(layers))
    outs = sn.emulate_forward(layers, power_iterations, mutant=mutant)
    for k, (L, out) in enumerate(zip(layers, outs)):
        sn.check_forward(ck, L, out, power_iterations, safety=safety)
        G = grads[k] if grads is not None else sn.make_grad(L, k)
        dW, partials = sn.emulate_backward(L, G, out["u"], out["v"], out["sigma"], mutant=mutant)
        sn.check_backward(ck, L, G, out["u"], out["v"], out["sigma"], dW, partials, safety=safety)
    ck.finish(verbose=False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", sn.SN_SHAPES, ids=lambda s: "%dx%d" % s)
def test_sn_restatement_meets_every_bound_without_the_safety_factor(shape, dtype):
    layers = sn.family_layers(shape, dtype)
    _sn_roundtrip(layers, 1, 1.0)
    _sn_roundtrip(layers, 0, 1.0)


@pytest.mark.parametrize("count,first", [(c, f) for c in sn.SN_COUNTS for f in (True, False)])
def test_sn_restatement_on_the_layer_counts(count, first):
    _sn_roundtrip(sn.count_layers(count, first), 1, 1.0)


@pytest.mark.parametrize("n", sn.SN_EXACT_ORDERS)
def test_sn_exact_family_bit_for_bit(n):
    for dtype in (torch.float32, torch.float64):
        layer, G = sn.make_exact_layer(n, dtype)
        _sn_roundtrip([layer], 1, 1.0, grads=[G])


SN_MUTANT_LAYERS = {
    "sigma_from_old_u": lambda: [sn.make_layer(3, 27), sn.make_layer(257, 65)],
    "no_eps_clamp": lambda: [sn.make_layer(3, 27, "zero"), sn.make_layer(1, 1)],
    "first_partial_only": lambda: [sn.make_layer(257, 65)],
    "transposed_outer": lambda: [sn.make_layer(3, 27)],
    "coef_over_sigma": lambda: [sn.make_layer(3, 27)],
    "wv_slice_overlap": lambda: [sn.make_layer(3, 27), sn.make_layer(5, 1120)],
}


@pytest.mark.parametrize("mutant", sn.SN_MUTANTS)
def test_every_sn_mutant_misses_a_bound(mutant):
    layers = SN_MUTANT_LAYERS[mutant]()
    assert _fails(lambda: _sn_roundtrip(layers, 1, sb.SAFETY)) is None
    why = _fails(lambda: _sn_roundtrip(layers, 1, sb.SAFETY, mutant))
    assert why is not None, mutant
    print(mutant, "->", why[:200])


def test_sn_conditions_raise():
    with pytest.raises(ValueError):
        sn.make_exact_layer(8)
    L = sn.make_layer(3, 27)
    L.W = L.W * 2.0 ** -60                                      # |v_raw|^2 ~ 2^-120: single squares underflow
    out = sn.emulate_forward([L], 1)[0]
    with pytest.raises(ValueError):
        sn.check_forward(sb.Checks("range"), L, out, 1)
    with pytest.raises(ValueError):
        sb.require_exact(torch.tensor([1.0 / 3.0], dtype=torch.float64))


# ================================================================================================ flat Adam
def _adam_check(n, cfg, step, fn, safety, nan_at=(), what="adam"):
    p, g, m, v, fam = sb.adam_inputs(n, nan_at=nan_at)
    sc = sb.adam_scalars(cfg, step)
    ref = sb.AdamRef(p, g, m, v, sc, safety)
    ck = sb.Checks("%s n=%d %s step %d" % (what, n, cfg, step))
    ref.check(ck, *fn(p, g, m, v, sc), fam)
    ck.finish(verbose=False)


def _torch_adam(cfg, step):
    lr, beta1, beta2, eps = sb.ADAM_CONFIGS[cfg]

    def run(p, g, m, v, sc):
        q = torch.nn.Parameter(p.clone())
        q.grad = g.clone()
        opt = torch.optim.Adam([q], lr=lr, betas=(beta1, beta2), eps=eps, foreach=False)
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
        opt.step()
        return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]
    return run


@pytest.mark.parametrize("cfg", list(sb.ADAM_CONFIGS))
@pytest.mark.parametrize("step", sb.ADAM_STEPS)
def test_adam_standins_meet_every_bound_without_the_safety_factor(cfg, step):
    for n in sb.ADAM_SIZES + (4099,):
        _adam_check(n, cfg, step, sb.adam_emulate, 1.0)
        _adam_check(n, cfg, step, _torch_adam(cfg, step), 1.0, what="torch.optim.Adam")


@pytest.mark.parametrize("pos", [0, 1, 2, 3, "tail"])
def test_adam_nan_gradient_stays_in_its_own_element(pos):
    for n in (7, 1027):
        at = n - 1 if pos == "tail" else 4 * ((n // 4) // 2) + pos
        _adam_check(n, "gan", 2, sb.adam_emulate, 1.0, nan_at=(at,))
        why = _fails(lambda: _adam_check(n, "gan", 2, lambda *a: sb.adam_emulate(*a, mutant="nan_poisons_float4"), sb.SAFETY, nan_at=(at,)))
        assert (why is None) == (pos == "tail"), (n, pos, why)       # the tail has no float4 neighbours to poison


@pytest.mark.parametrize("mutant", [m for m in sb.ADAM_MUTANTS if m != "nan_poisons_float4"])
def test_every_adam_mutant_misses_a_bound(mutant):
    caught = []
    for n, cfg, step in ((5, "plain", 1), (1025, "plain", 2), (1023, "gan", 2)):
        assert _fails(lambda: _adam_check(n, cfg, step, sb.adam_emulate, sb.SAFETY)) is None
        why = _fails(lambda: _adam_check(n, cfg, step, lambda *a: sb.adam_emulate(*a, mutant=mutant), sb.SAFETY))
        if why:
            caught.append((n, cfg, step, why[:160]))
    assert caught, mutant
    print(mutant, "->", caught[0])
    if mutant == "beta1_swapped":
        assert all(c[1] == "plain" for c in caught)                 # beta1 = 1/2 cannot tell: the reason for the second configuration


def test_adam_conditions_raise():
    p, g, m, v, _ = sb.adam_inputs(8)
    with pytest.raises(ValueError):
        sb.AdamRef(p, g, m, v, (0.25, sb.f32(0.999), 1e-8, 1e-3, 1.0))


# ================================================================================================ fused L1
L1_CASES = sb.l1_cases()


def _l1_roundtrip(name, safety, mutant=None):
    problems, n_slots = L1_CASES[name]
    out0 = torch.arange(n_slots, dtype=torch.float32) * 0.25 - 0.25            # slot 0 starts negative, slot 1 at zero
    gout = torch.tensor([1.5, -0.75, 2.0, 0.0, 0.3][:n_slots])
    ref = sb.L1Ref(problems, n_slots, out0, gout, safety)
    ck = sb.Checks("l1 " + name)
    ref.check_forward(ck, sb.l1_emulate_forward(problems, n_slots, out0, mutant))
    ref.check_backward(ck, sb.l1_emulate_backward(problems, gout, mutant))
    ck.finish(verbose=False)


@pytest.mark.parametrize("name", list(L1_CASES))
def test_l1_restatement_meets_every_bound_without_the_safety_factor(name):
    _l1_roundtrip(name, 1.0)


@pytest.mark.parametrize("mutant,name", [("mask_without_broadcast", "masks"), ("problem_33_dropped", "count33"), ("problem_33_dropped", "count65"),
                                         ("float4_tail_dropped", "n5"), ("float4_tail_dropped", "n12290"), ("scale_twice_backward", "n4")])
def test_every_l1_mutant_misses_an_assertion(mutant, name):
    assert _fails(lambda: _l1_roundtrip(name, sb.SAFETY)) is None
    why = _fails(lambda: _l1_roundtrip(name, sb.SAFETY, mutant))
    assert why is not None, (mutant, name)
    print(mutant, name, "->", why[:200])


def test_l1_ambiguous_signs_are_refused():
    pr = sb.l1_problem(64, 1)
    pr.y[5] = torch.nextafter(pr.x[5], torch.tensor(math.inf))               # one float apart: inside the two-rounding margin
    with pytest.raises(ValueError):
        sb.L1Ref([pr], 1, torch.zeros(1))


def test_l1_cases_reach_what_they_are_for():
    assert all(p.n for p in L1_CASES["count33"][0]) and len(L1_CASES["count33"][0]) == 33            # a second launch of one problem
    probs, _ = L1_CASES["count65"]
    assert len(probs) == 65 and probs[7].n == 0 and probs[32].n == 0
    assert [p.vec for p in L1_CASES["masks"][0]] == [False, True, False, True, True]
    assert sum(p.blocks for p in L1_CASES["one_slot40"][0]) > 40 and {p.slot for p in L1_CASES["one_slot40"][0]} == {0}


# ================================================================================================ correlation column maximum
@pytest.mark.parametrize("shape", sb.CORR_SHAPES, ids=lambda s: "B%d-N%d-C%d" % s)
def test_corr_restatement_meets_the_bound_without_the_safety_factor(shape):
    s, t = sb.corr_inputs(*shape)
    ck = sb.Checks("corr %s" % (shape,))
    sb.CorrRef(s, t, 1.0).check(ck, sb.corr_emulate(s, t))
    ck.finish(verbose=False)


@pytest.mark.parametrize("N,C", [(1, 64), (31, 64), (33, 128), (129, 64), (160, 256)])
def test_corr_exact_family_bit_for_bit(N, C):
    s, t, planted = sb.corr_exact_inputs(N, C)
    assert planted
    ref = sb.CorrRef(s, t).out
    assert torch.equal(sb.corr_emulate(s, t), sb.require_exact(ref).float())
    if N % 32:
        assert not torch.equal(sb.corr_emulate(s, t, "ragged_tile_dropped"), ref.float())
    if N > 1:
        assert not torch.equal(sb.corr_emulate(s, t, "transposed_readout"), ref.float())


def test_corr_nonfinite_contract_and_its_mutants():
    s, t = sb.corr_nonfinite_inputs()
    ck = sb.Checks("corr non-finite")
    sb.corr_nonfinite_check(ck, s, t, sb.corr_emulate(s, t))
    ck.finish(verbose=False)
    for mutant in ("nan_dropped", "floor_3e38"):
        ck = sb.Checks("corr non-finite " + mutant)
        sb.corr_nonfinite_check(ck, s, t, sb.corr_emulate(s, t, mutant))
        assert _fails(lambda: ck.finish(verbose=False)) is not None, mutant


@pytest.mark.parametrize("mutant,shape", [("ragged_tile_dropped", (2, 31, 64)), ("ragged_tile_dropped", (3, 129, 128)), ("transposed_readout", (2, 33, 64))])
def test_every_corr_mutant_misses_the_bound(mutant, shape):
    s, t = sb.corr_inputs(*shape)
    ck = sb.Checks("corr %s %s" % (mutant, shape))
    sb.CorrRef(s, t).check(ck, sb.corr_emulate(s, t, mutant))
    assert _fails(lambda: ck.finish(verbose=False)) is not None
