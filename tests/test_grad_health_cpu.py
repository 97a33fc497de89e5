"""Gradient health without a GPU: the float64 restatement of tests/grad_health_cases.py against hand-computed cases, the clip rule at
its edges, the three new symbols in the header / the binding table / the built library, and every argument error of FlatAdam and the
trainers -- raised before anything touches a device."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_health_cases as gh  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ffwm_grad_health", "ffwm_grad_health_workspace_bytes", "ffwm_adam_step_guarded")


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_hand_computed_cases():
    g = torch.tensor([3.0, -4.0, gh.NAN, 0.5, 1e-30, gh.INF, -gh.INF, -0.0, 2.0, 1.0, 1.0], dtype=torch.float32)
    ref = gh.reference(g, [4, 8, 8, 11])
    assert ref[0] == {"sum": 25.25, "max": 4.0, "nonfinite": 1, "n": 4, "m": 3}
    f = float(torch.tensor(1e-30, dtype=torch.float32))
    assert ref[1] == {"sum": f * f, "max": f, "nonfinite": 2, "n": 4, "m": 2} and ref[1]["sum"] > 0
    assert ref[2] == {"sum": 0.0, "max": 0.0, "nonfinite": 0, "n": 0, "m": 0}
    assert ref[3] == {"sum": 6.0, "max": 2.0, "nonfinite": 0, "n": 3, "m": 3}
    all_bad = gh.reference(torch.tensor([gh.NAN, gh.INF], dtype=torch.float32), [2])[0]
    assert all_bad == {"sum": 0.0, "max": 0.0, "nonfinite": 2, "n": 2, "m": 0}


def test_check_record_takes_the_exact_record_and_refuses_wrong_ones():
    case = gh.Case("hand", torch.tensor([3.0, -4.0, gh.NAN, 0.5, 2.0], dtype=torch.float32), [4, 5])
    good = gh.record_of(case.ref)
    gh.check_record(case, good, verbose=False)
    for (s, k), v in {(0, 0): 25.25 * (1 + 8 * gh.U64), (0, 1): 3.0, (0, 2): 0.0, (1, 3): 2.0, (1, 1): -2.0}.items():
        bad = good.clone()
        bad[s, k] = v
        with pytest.raises(AssertionError):
            gh.check_record(case, bad, verbose=False)


def test_the_cases_are_all_there():
    cases = gh.cases()
    names = [c.name for c in cases]
    assert len(set(map(repr, cases))) == len(cases)
    sizes = {c.n for c in cases if c.name == "size"}
    assert sizes == {1, 2, 3, 4, 5, 1027, gh.CHUNK + 1, 3 * gh.CHUNK - 3}
    assert any(c.n > 256 * gh.CHUNK and len(c.seg_end) == 1 for c in cases)
    assert {1, 2, 16} <= {len(c.seg_end) for c in cases}
    for kind in gh.KINDS:
        for place in ("first", "chunk-last", "next-chunk-first", "tail", "in-four"):
            assert "%s-%s" % (kind, place) in names
    for name in ("four-between-long", "ends-chunk-plus-4", "zero-segment", "uniform-1e-30", "uniform-1e25", "denormals", "forty-decades",
                 "minus-zero", "all-nan-segment"):
        assert name in names
    mix = next(c for c in cases if c.name == "forty-decades").g.abs()
    assert float(mix.max()) / float(mix.min()) > 1e38


def test_clip_coefficient_at_its_edges():
    from ffwm_amd.optim import clip_coefficient
    assert clip_coefficient(0.0, 1.0) == 1.0                          # norm 0: 1 / 1e-6, clamped
    assert clip_coefficient(123.0, None) == 1.0 and clip_coefficient(123.0, 0) == 1.0 and clip_coefficient(123.0, 0.0) == 1.0
    assert clip_coefficient(4.0, 2.0) == 2.0 / (2.0 + 1e-6) < 1.0     # norm == max_norm: just below 1, as clip_grad_norm_
    assert clip_coefficient(4.0, 1.0) == 1.0 / (2.0 + 1e-6)
    assert clip_coefficient(4.0, 3.0) == 1.0                          # below the limit: exactly 1
    # torch's own coefficient on the same numbers
    p = nn.Parameter(torch.zeros(3))
    p.grad = torch.tensor([1.0, 2.0, 2.0])
    torch.nn.utils.clip_grad_norm_([p], 1.5)
    want = torch.tensor([1.0, 2.0, 2.0]) * torch.tensor(clip_coefficient(9.0, 1.5), dtype=torch.float32)
    assert float((p.grad - want).abs().max()) <= 2.0 ** -23 * 2.0


# ------------------------------------------------------------------------------------------------ exports
def test_the_three_entry_points_are_declared_bound_and_exported():
    from ffwm_amd import _lib, build, ops
    text = open(os.path.join(ROOT, "include", "ffwm_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.EXPORTS
    assert "ffwm_grad_health" in _lib._SIGNATURES and "ffwm_adam_step_guarded" in _lib._SIGNATURES
    assert len(_lib._SIGNATURES["ffwm_grad_health"]) == 9 and len(_lib._SIGNATURES["ffwm_adam_step_guarded"]) == 17
    assert int(re.search(r"#define FFWM_GRAD_HEALTH_CHUNK (\d+)", code).group(1)) == ops.GRAD_HEALTH_CHUNK == gh.CHUNK
    assert int(re.search(r"#define FFWM_GRAD_HEALTH_MAX_SEGMENTS (\d+)", code).group(1)) == ops.GRAD_HEALTH_MAX_SEGMENTS == 16
    assert "#define FFWM_ABI_VERSION 5" in code
    build.build()
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    # one partial of four doubles per chunk; every segment may round up once
    assert lib.ffwm_grad_health_workspace_bytes(1, 1) == 32
    assert lib.ffwm_grad_health_workspace_bytes(3 * gh.CHUNK + 1, 16) == 32 * (3 + 16)
    assert lib.ffwm_grad_health_workspace_bytes(0, 1) == 0 and lib.ffwm_grad_health_workspace_bytes(8, 17) == 0


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from ffwm_amd import _lib, build
    build.build()
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = ctypes.c_void_p((p.value + 15) // 16 * 16)
    assert lib.ffwm_grad_health(None, 8, a, 1, a, 64, a, 0, None) == -1 and b"NULL" in lib.ffwm_last_error()
    assert lib.ffwm_grad_health(a, 8, a, 1, a, 64, a, 1, None) == -2
    assert lib.ffwm_grad_health(a, 0, a, 1, a, 64, a, 0, None) == -1
    assert lib.ffwm_grad_health(a, 8, a, 17, a, 1024, a, 0, None) == -1 and b"n_seg" in lib.ffwm_last_error()
    assert lib.ffwm_grad_health(ctypes.c_void_p(a.value + 4), 8, a, 1, a, 64, a, 0, None) == -1 and b"aligned" in lib.ffwm_last_error()
    assert lib.ffwm_grad_health(a, 8, a, 1, a, 16, a, 0, None) == -1 and b"workspace" in lib.ffwm_last_error()
    args = (a, a, a, a, 8, 1e-3, 0.5, 0.999, 1e-8, a, a)
    assert lib.ffwm_adam_step_guarded(*args, 1, 1.0, 0, a, 0, None) == -1 and b"skip_nonfinite" in lib.ffwm_last_error()
    assert lib.ffwm_adam_step_guarded(*args, 17, 0.0, 1, a, 0, None) == -1 and b"n_seg" in lib.ffwm_last_error()
    assert lib.ffwm_adam_step_guarded(*args, 1, 0.0, 1, None, 0, None) == -1 and b"NULL" in lib.ffwm_last_error()
    assert lib.ffwm_adam_step_guarded(*args, 1, 0.0, 1, a, 1, None) == -2


def test_ops_wrapper_refuses_cpu_tensors():
    from ffwm_amd import ops
    with pytest.raises(NotImplementedError):
        ops.grad_health(torch.zeros(8), [8])
    with pytest.raises(ValueError):
        ops.grad_health(torch.zeros(2, 4), [8])


# ------------------------------------------------------------------------------------------------ FlatAdam's arguments
class _Small(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 5, 3)          # 135 + 5
        self.fc = nn.Linear(7, 3)               # 21 + 3
        self.fc2 = nn.Linear(3, 11)             # 33 + 11


def _reducer(net):
    from ffwm_amd.dp import BucketedGradReducer
    return BucketedGradReducer(list(net.parameters()), gather=False)


def test_flat_adam_checks_its_new_arguments_before_the_device():
    from ffwm_amd.optim import FlatAdam
    net = _Small()
    red = _reducer(net)
    params = list(net.parameters())
    conv, fc, fc2 = list(net.conv.parameters()), list(net.fc.parameters()), list(net.fc2.parameters())
    # the reducer lays the parameters out in reverse registration order: fc2, fc, conv
    assert red.offset[net.fc2.bias][0] == 0
    bad = [
        dict(max_grad_norm=1.0),                                                      # without skip_nonfinite
        dict(max_grad_norm=1.0, monitor=True),
        dict(max_grad_norm=-1.0, skip_nonfinite=True),
        dict(max_grad_norm=float("nan"), skip_nonfinite=True),
        dict(monitor=True, segments=[("conv", conv), ("fc", fc), ("fc2", fc2)]),     # not the reducer's order
        dict(monitor=True, segments=[("fc2", fc2), ("conv", conv)]),                 # a gap
        dict(monitor=True, segments=[("fc2", fc2), ("fc", fc + fc2), ("conv", conv)]),          # an overlap
        dict(monitor=True, segments=[("fc2", fc2), ("w", [net.fc.weight]), ("b", [net.fc.bias]), ("conv", conv)]),   # fc.bias lies in front of fc.weight
        dict(monitor=True, segments=[("a", fc2), ("a", fc), ("conv", conv)]),        # a name twice
        dict(monitor=True, segments=[("scale", fc2), ("fc", fc), ("conv", conv)]),   # a name health() uses itself
        dict(monitor=True, segments=[("fc2", fc2), ("fc", fc), ("conv", conv), ("none", [])]),
        dict(skip_nonfinite=True, segments=[("s%d" % k, fc2) for k in range(17)]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            FlatAdam(params, red, **kw)
    # correct arguments get as far as the device refusal, like the plain optimizer
    for kw in (dict(), dict(monitor=True), dict(skip_nonfinite=True, max_grad_norm=2.0),
               dict(monitor=True, segments=[("fc2", fc2), ("fc", fc), ("conv", conv)]),
               dict(monitor=True, segments=[("fc2", [net.fc2.bias]), ("rest", [net.fc2.weight] + fc + conv)])):
        with pytest.raises(NotImplementedError):
            FlatAdam(params, red, **kw)
    from ffwm_amd.optim import _health_segments
    order = sorted(params, key=lambda q: red.offset[q][0])
    assert _health_segments(None, order, red.offset, 0, 208) == [("all", 208)]
    assert _health_segments([("fc2", fc2), ("fc", fc), ("conv", conv)], order, red.offset, 0, red.offset[net.conv.weight][1]) \
        == [("fc2", red.offset[net.fc.bias][0]), ("fc", red.offset[net.conv.bias][0]), ("conv", red.offset[net.conv.weight][1])]


def test_trainers_refuse_the_arguments_without_the_flat_step():
    from ffwm_amd import trainer
    for kw in (dict(grad_health=True), dict(skip_nonfinite=True), dict(max_grad_norm=1.0, skip_nonfinite=True), dict(max_grad_norm=1.0)):
        with pytest.raises(ValueError):
            trainer.FFWMTrainer("cpu", **kw)
        with pytest.raises(ValueError):
            trainer.FFWMTrainer("cuda:0", flat_adam=False, **kw)          # asked for: refused before anything is built
        with pytest.raises(ValueError):
            trainer.FlowNetTrainer("cpu", **kw)


def test_a_default_trainer_carries_no_health_state():
    import torch_refs
    from ffwm_amd import trainer
    t = trainer.FlowNetTrainer("cpu", seed=0, ngf=8, warp=torch_refs.warp, fused_regularization=False)
    assert t.health_options == {}
    with pytest.raises(RuntimeError):
        t.health()
    assert not [k for k, v in vars(t).items() if "health" in k and torch.is_tensor(v)]
    # every new argument is off by default (the GPU suite checks that a default FlatAdam allocates no record, guard or workspace)
    import inspect
    from ffwm_amd.optim import FlatAdam
    sig = inspect.signature(FlatAdam.__init__)
    assert [sig.parameters[k].default for k in ("monitor", "skip_nonfinite", "max_grad_norm", "segments")] == [False, False, None, None]
    for name in ("grad_health", "skip_nonfinite", "max_grad_norm"):
        assert inspect.signature(trainer.FFWMTrainer.__init__).parameters[name].default in (False, None)
        assert inspect.signature(trainer.FlowNetTrainer.__init__).parameters[name].default in (False, None)
