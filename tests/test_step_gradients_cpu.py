"""The step-gradient reference (tests/step_gradient_reference.py) on the CPU: the hand-driven sequence IS FFWMTrainer.step(), the
batched loss passes stay within rounding of it, and `check` fails on every kind of damage it is there for.  No float64 pass here
(16-20 s on a CPU): the float64 reference runs on the GPU, in tests/test_gpu_step_gradients.py.

Measured (ngf=16, batch 2, trainer seed 0, batch seed 3, 16 threads), whole-net relative L2 of the gradient:
    harness against step(), batched_losses=False : 0.0 for flowNetF, flowNetB, netG and netD (bit for bit)
    step() batched_losses=True against the harness: flowNetF 1.2e-6, netG 8.5e-7, flowNetB 0.0, netD 0.0
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import step_gradient_reference as sgr  # noqa: E402
import torch_refs  # noqa: E402

# whole-net relative L2 between step(batched_losses=True) and the harness, as measured (module docstring); the bound is 16 x these.
# For flowNetB and netD that is 16 x 0.0, bit equality, on purpose: the batched passes only touch the loss networks' batching, whose
# gradients reach flowNetB through unchanged forward values and netD not at all -- a difference there is a change of the computation,
# not of a summation order.
BATCHED_MEASURED = {"flowNetF": 1.2e-6, "flowNetB": 0.0, "netG": 8.5e-7, "netD": 0.0}


def _step_grads(batched):
    from ffwm_amd import trainer
    t = trainer.FFWMTrainer("cpu", seed=0, ngf=16, warp=torch_refs.warp, warp_flipcat=torch_refs.warp_flipcat, batched_losses=batched)
    t.step(trainer.synthetic_batch(2, "cpu", seed=3))
    return ({net: {n: p.grad.detach().double().clone() for n, p in ps} for net, ps in sgr.graded_parameters(t).items()},
            t.loss_values())


@pytest.fixture(scope="module", autouse=True)
def _sixteen_threads():
    """The thread count the figures were measured with, for the harness and the steps it is compared with; put back afterwards."""
    before = torch.get_num_threads()
    torch.set_num_threads(16)
    yield
    torch.set_num_threads(before)


@pytest.fixture(scope="module")
def harness():
    from ffwm_amd import trainer
    return sgr.reference_passes(torch.float32, "cpu", trainer.synthetic_batch(2, "cpu", seed=3), 0, 16, sgr.LRS, 1)[0]


def test_the_harness_is_the_step_bit_for_bit(harness):
    got, losses = _step_grads(False)
    for net in sgr.NETS:
        assert set(got[net]) == set(harness["grads"][net])
        for n, g in got[net].items():
            assert torch.equal(g, harness["grads"][net][n]), (net, n)
        assert sgr.net_norm(got[net]) > 0
    assert losses == harness["losses"]


def test_batched_loss_passes_stay_within_rounding_of_the_harness(harness):
    got, _ = _step_grads(True)
    for net in sgr.NETS:
        rel = sgr.net_distance(got[net], harness["grads"][net]) / sgr.net_norm(harness["grads"][net])
        print("batched_losses=True against the harness: %-9s %.3e" % (net, rel))
        assert rel <= 16 * BATCHED_MEASURED[net], (net, rel)


# ------------------------------------------------------------------------------------------------ check() on synthetic gradients
_SHAPES = [(8, 3, 3, 3), (8,), (8,), (16, 8, 3, 3), (16,), (16,), (2, 16, 1, 1), (2,)]
_REL = {"flowNetF": 2.5e-2, "flowNetB": 5.7e-3, "netG": 6.7e-3, "netD": 2.5e-4}        # plain float32 against float64, as measured


def _unit(shape, g):
    v = torch.randn(*shape, generator=g, dtype=torch.float64)
    return v / v.norm()


def _synthetic():
    """Gradients shaped like a small net's (weights, biases, one bias in front of a BatchNorm: ~1e-16), their float32 yardstick at the
    measured distances, and an honest `got`: 1.5 x the yardstick's distance in another direction."""
    g = torch.Generator().manual_seed(0)
    g64, g32, got = {}, {}, {}
    for net in sgr.NETS:
        g64[net], g32[net], got[net] = {}, {}, {}
        for i, shape in enumerate(_SHAPES):
            name = "layer%d.%s" % (i, "bias" if len(shape) == 1 else "weight")
            ref = torch.randn(*shape, generator=g, dtype=torch.float64) * (10.0 ** (-(i % 3)))
            if i == 1:
                ref = ref * 1e-16                       # a conv bias feeding a BatchNorm
            noise = max(_REL[net] * float(ref.norm()), 1e-9)
            g64[net][name] = ref
            g32[net][name] = ref + noise * _unit(shape, g)
            got[net][name] = ref + 1.5 * noise * _unit(shape, g)
    return g64, g32, got


def _roll_by_one_tensor(grads):
    """Every tensor reads where its neighbour's gradient was packed: the flat array shifted by the first tensor's size."""
    flat = torch.cat([v.flatten() for v in grads.values()])
    flat = torch.roll(flat, next(iter(grads.values())).numel())
    out, at = {}, 0
    for k, v in grads.items():
        out[k] = flat[at:at + v.numel()].view_as(v)
        at += v.numel()
    return out


_TAMPER = {"doubled": lambda g: {k: 2 * v for k, v in g.items()}, "halved": lambda g: {k: 0.5 * v for k, v in g.items()},
           "zeroed": lambda g: {k: torch.zeros_like(v) for k, v in g.items()}, "rolled": _roll_by_one_tensor}


def test_check_passes_honest_gradients_and_reports_their_ratios():
    g64, g32, got = _synthetic()
    tol = sgr.bounds(g64, g32)
    ratios = sgr.check(got, g64, tol)
    for net in sgr.NETS:
        assert 1.0 < ratios[net]["tensor"] <= 1.5 + 1e-9 and 1.0 < ratios[net]["net"] <= 1.5 + 1e-9, (net, ratios[net])
        assert abs(tol.r[net] - _REL[net]) <= 1e-3 * _REL[net]
    assert sgr.check(g32, g64, tol)["netG"]["net"] == pytest.approx(1.0)


@pytest.mark.parametrize("net", sgr.NETS)
@pytest.mark.parametrize("kind", sorted(_TAMPER))
def test_check_fails_on_a_damaged_gradient_in_any_single_net(kind, net):
    g64, g32, got = _synthetic()
    tol = sgr.bounds(g64, g32)
    got[net] = _TAMPER[kind](got[net])
    # (also under the reliefs the GPU test grants netD: a measured ratio x 1.5, and one scale's group with a whole-net cap)
    with pytest.raises(AssertionError):
        sgr.check(got, g64, tol, relief={"netD": {"ratio": {"tensor": 1.5 * 148.8, "net": 1.5 * 60.6}}})
    with pytest.raises(AssertionError):
        sgr.check(got, g64, tol, relief={"netD": {"one_group": [["layer0.weight", "layer1.bias", "layer2.bias"]], "net": 1.5 * 5.5e-3}})
    with pytest.raises(AssertionError) as e:
        sgr.check(got, g64, tol)
    msg = str(e.value)
    assert net in msg and all(other not in msg for other in sgr.NETS if other != net), msg
    if kind == "doubled" and net == "netD":             # a scale error reads as one: norm ratio 2, cosine 1 (netD: the noise is 4e-4)
        assert "|got|/|ref| 2 " in msg and "cosine 1.0000" in msg, msg
    if kind == "rolled":
        assert "cosine 1.0000" not in msg, msg


def _off(g64, names, rel, seed=1):
    return {k: (v + rel * float(v.norm()) * _unit(v.shape, torch.Generator().manual_seed(seed)) if k in names else v.clone())
            for k, v in g64.items()}


def test_the_one_group_relief_admits_one_group_and_nothing_else():
    """netD's yardstick is 2.5e-4 here; tensors 1e-2 off are 40 x over it."""
    g64, g32, _ = _synthetic()
    tol = sgr.bounds(g64, g32)
    groups = [["layer0.weight", "layer2.bias"], ["layer3.weight", "layer4.bias"]]
    relief = {"netD": {"one_group": groups, "net": 2e-2}}
    got = {net: {k: v.clone() for k, v in g.items()} for net, g in g64.items()}
    got["netD"] = _off(g64["netD"], groups[0], 1e-2)
    with pytest.raises(AssertionError):
        sgr.check(got, g64, tol)
    ratios = sgr.check(got, g64, tol, relief=relief)
    assert ratios["netD"]["tensor"] == pytest.approx(1e-2 / 2.5e-4, rel=1e-2) and ratios["netD"]["net"] > sgr.M       # against the tolerance proper
    with pytest.raises(AssertionError):                              # the whole-net cap holds
        sgr.check(got, g64, tol, relief={"netD": {"one_group": groups, "net": 1e-3}})
    got["netD"] = _off(g64["netD"], [groups[0][0], groups[1][0]], 1e-2)           # two groups at once
    with pytest.raises(AssertionError):
        sgr.check(got, g64, tol, relief=relief)
    got["netD"] = _off(g64["netD"], groups[0] + ["layer6.weight"], 1e-2)          # a tensor outside every group
    with pytest.raises(AssertionError):
        sgr.check(got, g64, tol, relief=relief)
    got["netD"] = {k: v.clone() for k, v in g64["netD"].items()}
    got["netG"] = _off(g64["netG"], ["layer0.weight"], 0.5)                       # another net gets nothing from netD's relief
    with pytest.raises(AssertionError):
        sgr.check(got, g64, tol, relief=relief)


def test_the_ratio_relief_replaces_M_for_its_net_only():
    g64, g32, _ = _synthetic()
    tol = sgr.bounds(g64, g32)
    got = {net: {k: v.clone() for k, v in g.items()} for net, g in g64.items()}
    got["netD"] = _off(g64["netD"], list(g64["netD"]), 1e-2)                      # ratio 40 everywhere
    with pytest.raises(AssertionError):
        sgr.check(got, g64, tol)
    sgr.check(got, g64, tol, relief={"netD": {"ratio": {"tensor": 41, "net": 41}}})
    for bad in ({"tensor": 39, "net": 41}, {"tensor": 41, "net": 39}):
        with pytest.raises(AssertionError):
            sgr.check(got, g64, tol, relief={"netD": {"ratio": bad}})


def test_check_leaves_no_tensor_out():
    g64, g32, got = _synthetic()
    tol = sgr.bounds(g64, g32)
    del got["netG"]["layer3.weight"]
    with pytest.raises(AssertionError):
        sgr.check(got, g64, tol)
    g64, g32, got = _synthetic()
    got["netD"]["layer0.weight"][0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        sgr.check(got, g64, tol)


def test_only_zero_gradient_tensors_live_on_the_floor():
    g64, g32, _ = _synthetic()
    tol = sgr.bounds(g64, g32)
    zero = sgr.zero_gradient_tensors(g64)
    for net in sgr.NETS:
        assert zero[net] == ["layer1.bias"] and sgr.floor_users(tol)[net] == ["layer1.bias"]
        assert tol[net]["layer1.bias"] <= 2 * tol.floor[net]
        assert tol.floor[net] == pytest.approx(16 * 2.0 ** -24 * sgr.net_norm(g64[net]) / len(_SHAPES) ** 0.5)


def test_conv_biases_feeding_a_batchnorm_are_counted_from_the_modules():
    """FlowNet: 13 encoder convs, 6 deconvs and 6 inter_convs in front of a BatchNorm (the unused occlusion branch is in no
    optimizer); netD: 3 scales x 3 convs; netG's PixelShuffle blocks and shortcut convs are not among them."""
    t = sgr.plain_trainer(0, 16)
    names = sgr.conv_biases_feeding_batchnorm(t)
    graded = {net: dict(ps) for net, ps in sgr.graded_parameters(t).items()}
    assert len(names["flowNetF"]) == len(names["flowNetB"]) == 25 and len(names["netD"]) == 9
    n_res = sum(isinstance(m, type(t.netG.e0[-1])) for m in t.netG.modules())
    n_bn_blocks = sum(1 for k in ("e1", "e2", "e3", "att0", "att1", "att2"))
    assert len(names["netG"]) == 2 * n_res + n_bn_blocks
    for net in sgr.NETS:
        assert len(set(names[net])) == len(names[net])
        for n in names[net]:
            assert n.endswith(".bias") and n in graded[net] and "inter_conv_occ" not in n, (net, n)
    assert not any(n.startswith(("d0.", "d1.", "d2.")) or ".input." in n for n in names["netG"])
