"""FlatAdam: torch.optim.Adam's update (models/ffwm_model.py:46-49, models/flownet_model.py:33: no weight decay, no
amsgrad) as ONE streaming kernel per step over flat arrays (csrc/adam.hip).

The gradients already live in the data-parallel reducer's flat array (dp.BucketedGradReducer.flat); this class
moves the parameters of one optimizer into a flat array laid out the same way (``param.data`` becomes a view of
it -- the Parameter objects, their names and state dicts are untouched) and keeps both moment estimates flat.
Like the reference's checkpoints (models/base_model.py:save_networks), optimizer state is not saved.

FlatSGD: the same for torch.optim.SGD with momentum and one (learning rate, weight decay) per parameter group
(lightcnn/finetune.py:74-90), csrc/sgd.hip.

Gradient health (FlatAdam's monitor / skip_nonfinite / max_grad_norm, all off by default): the step becomes one streaming reduction
over the optimizer's slice of the flat gradients (csrc/grad_health.hip: per segment sum g^2, max |g|, non-finite count) and an Adam
step that reads its decision -- apply, apply clipped, or skip -- from device memory (ffwm_adam_step_guarded), so both sit inside a
captured step.  The guard protects the parameters and both moment arrays.  It restores nothing else: the BatchNorm running
statistics were already updated by the forward pass of the bad step.
"""
import math

import torch

from . import _lib

MAX_HEALTH_SEGMENTS = 16          # FFWM_GRAD_HEALTH_MAX_SEGMENTS (include/ffwm_hip.h)
_HEALTH_KEYS = ("scale", "skipped", "steps_skipped", "steps_seen", "steps_applied")


def clip_coefficient(sumsq, max_norm):
    """The factor a clipped step multiplies its gradients by, from the sum of their squares: torch.nn.utils.clip_grad_norm_'s
    min(1, max_norm / (sqrt(sumsq) + 1e-6)) in double; 1.0 when max_norm is None or <= 0 (no clipping).  The kernel
    (csrc/adam.hip: adam_guard_advance_kernel) computes the same expression and rounds it once to float32."""
    if max_norm is None or max_norm <= 0:
        return 1.0
    return min(1.0, float(max_norm) / (math.sqrt(sumsq) + 1e-6))


def _health_segments(segments, order, offset, lo, n):
    """[(name, end)] from FlatAdam's ``segments`` (a list of (name, params)): they must tile ``order`` -- the optimizer's parameters
    in the reducer's order -- segment by segment.  A segment ends where the next one's first parameter begins, the last one at n."""
    if segments is None:
        return [("all", n)]
    segments = [(name, [p for p in ps if p.requires_grad]) for name, ps in segments]
    if len(segments) > MAX_HEALTH_SEGMENTS:
        raise ValueError("FlatAdam: at most %d segments (csrc/grad_health.hip), got %d" % (MAX_HEALTH_SEGMENTS, len(segments)))
    names = [name for name, _ in segments]
    if len(set(names)) != len(names) or set(names) & set(_HEALTH_KEYS) or not all(isinstance(k, str) for k in names):
        raise ValueError("FlatAdam: segment names must be distinct strings other than %s" % ", ".join(_HEALTH_KEYS))
    walked, own = [], set(map(id, order))
    for name, ps in segments:
        if not ps:
            raise ValueError("FlatAdam: segment %r has no trainable parameter" % name)
        if any(id(p) not in own for p in ps):
            raise ValueError("FlatAdam: segment %r holds a parameter that is not the optimizer's" % name)
        walked += sorted(ps, key=lambda p: offset[p][0])
    if list(map(id, walked)) != list(map(id, order)):
        raise ValueError("FlatAdam: the segments do not tile the optimizer's parameter range in the reducer's order")
    starts = [min(offset[p][0] for p in ps) - lo for _, ps in segments]
    return list(zip(names, starts[1:] + [n]))


class FlatAdam(object):
    """``monitor``, ``skip_nonfinite``, ``max_grad_norm`` (all off by default; with all three off step() is the one launch it always
    was, and nothing below is allocated):
      monitor         every step() first measures the optimizer's gradients (ffwm_grad_health); health() reports them.
      skip_nonfinite  a step whose gradients hold a NaN or an inf changes neither the parameters nor the moments nor the step count
                      of the bias corrections; the decision is taken on the device, so it also holds for every replay of a captured
                      step.  BatchNorm running statistics the forward pass of that step already wrote are NOT restored.
      max_grad_norm   clip by the global norm over the optimizer's whole range, torch.nn.utils.clip_grad_norm_'s coefficient
                      (clip_coefficient); needs skip_nonfinite.  The gradient array itself is not rescaled.
      segments        [(name, params), ...] tiling the optimizer's parameters in the reducer's order (at most 16): the ranges
                      health() reports on; one segment "all" by default.
    Any of the three turns the step into ffwm_grad_health + ffwm_adam_step_guarded, with the step counter on the device whatever
    ``capturable`` says; record, workspace, guard and the segment table are allocated here, once."""

    def __init__(self, params, reducer, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, capturable=False, monitor=False, skip_nonfinite=False,
                 max_grad_norm=None, segments=None):
        params = [p for p in params if p.requires_grad]
        if reducer.flat is None or not params:
            raise ValueError("FlatAdam needs a reducer with one flat gradient array and at least one parameter")
        spans = sorted(reducer.offset[p] for p in params)
        self.lo, self.hi = spans[0][0], spans[-1][1]
        inside = [p for p, (a, b) in reducer.offset.items() if a >= self.lo and b <= self.hi]
        if len(inside) != len(params) or set(map(id, inside)) != set(map(id, params)):
            raise ValueError("FlatAdam: the parameters are not a contiguous range of the reducer's flat layout")
        if self.lo % 4:
            raise ValueError("FlatAdam: range start is not 16-byte aligned")
        self.reducer = reducer
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        n = self.hi - self.lo
        # the health options are checked before anything touches a device
        if max_grad_norm is not None and not skip_nonfinite:
            raise ValueError("FlatAdam: max_grad_norm needs skip_nonfinite=True (a clip over a non-finite norm has no meaning)")
        if max_grad_norm is not None and not float(max_grad_norm) >= 0:
            raise ValueError("FlatAdam: max_grad_norm must be >= 0 (0 or None: no clipping), got %r" % (max_grad_norm,))
        self.monitor, self.skip_nonfinite = bool(monitor), bool(skip_nonfinite)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.guarded = self.monitor or self.skip_nonfinite or self.max_grad_norm is not None
        self.segments = None
        if self.guarded or segments is not None:
            self.segments = _health_segments(segments, sorted(params, key=lambda p: reducer.offset[p][0]), reducer.offset, self.lo, n)
        dev, dt = reducer.flat.device, reducer.flat.dtype
        if dt != torch.float32 or dev.type != "cuda":
            raise NotImplementedError("FlatAdam runs on float32 CUDA parameters only (csrc/adam.hip)")
        self.params = torch.zeros(n, device=dev, dtype=dt)
        self.exp_avg = torch.zeros(n, device=dev, dtype=dt)
        self.exp_avg_sq = torch.zeros(n, device=dev, dtype=dt)
        with torch.no_grad():
            for p in params:
                a, b = reducer.offset[p]
                view = self.params[a - self.lo:b - self.lo].view_as(p)
                view.copy_(p.data)
                p.data = view
                p._ffwm_flat_adam = True       # updated by a raw-pointer kernel: the version counter does not see it (conv.frozen_cache)
        self.n = n
        self.steps = 0
        # capturable: the step counter lives on the device (ffwm_adam_step_device), so that step() can sit inside a captured hipGraph
        self.capturable = bool(capturable)
        # state[0] step counter, state[1..2] scratch, state[3] the current learning rate (csrc/adam.hip: it overrides the kernel argument
        # a captured graph has baked in)
        self.state = torch.zeros(4, device=dev, dtype=torch.float64) if (self.capturable or self.guarded) else None
        # the health pass: [record (4 per segment) | guard (6)] in one array, so that health() is one copy; a captured step holds these addresses
        self.seg_end = self.record = self.guard = self.workspace = self._health = None
        if self.guarded:
            n_seg = len(self.segments)
            self.seg_end = torch.tensor([e for _, e in self.segments], dtype=torch.int64, device=dev)
            self._health = torch.zeros(4 * n_seg + 6, device=dev, dtype=torch.float64)
            self.record, self.guard = self._health[:4 * n_seg], self._health[4 * n_seg:]
            self.workspace = torch.empty(_lib.load().ffwm_grad_health_workspace_bytes(n, n_seg) // 8, device=dev, dtype=torch.float64)
        if self.state is not None:
            self.state[3] = -1.0          # no learning-rate override yet (0.0 is a legitimate rate: the sentinel is negative)
        # torch.optim's interface for schedulers (base_model.update_learning_rate: StepLR / lambda rules write param_groups[i]['lr'])
        self.param_groups = [{"capturable": self.capturable, "lr": self.lr, "params": params}]
        self._lr_on_device = None
        self._lr_seen = self.lr

    def sync_lr(self):
        """The learning rate of the next step: whichever of ``self.lr`` (direct assignment) and ``param_groups[0]['lr']`` (torch.optim's
        interface: base_model.update_learning_rate, StepLR / lambda rules) CHANGED since the last call -- the scheduler's value when both
        did.  Eager: used by the next step() directly.  Capturable: written to the device state, so it also reaches the REPLAYS of a
        captured step -- call it (or step()) from the host after the scheduler ran; a replay itself runs no Python.  A rate of 0.0 is a
        rate like any other (csrc/adam.hip takes the device value whenever it is >= 0; the state starts at -1 = "no override")."""
        g = float(self.param_groups[0]["lr"])
        if g != self._lr_seen:
            lr = g
        elif float(self.lr) != self._lr_seen:
            lr = float(self.lr)
        else:
            lr = self._lr_seen
        self.lr = self._lr_seen = lr
        self.param_groups[0]["lr"] = lr
        if self.state is not None and lr != self._lr_on_device and not torch.cuda.is_current_stream_capturing():
            self.state[3:4].fill_(lr)
            self._lr_on_device = lr
        return lr

    def step(self):
        self.sync_lr()
        self.steps += 1
        g = self.reducer.flat[self.lo:self.hi]
        dev = self.params.device.index
        cur = torch.cuda.current_device()
        if cur != dev:
            torch.cuda.set_device(dev)
        try:
            if self.guarded:
                lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
                n_seg = len(self.segments)
                _lib.check(lib.ffwm_grad_health(g.data_ptr(), self.n, self.seg_end.data_ptr(), n_seg, self.workspace.data_ptr(),
                                                self.workspace.numel() * 8, self.record.data_ptr(), _lib.F32, stream), "ffwm_grad_health")
                _lib.check(lib.ffwm_adam_step_guarded(self.params.data_ptr(), g.data_ptr(), self.exp_avg.data_ptr(),
                                                      self.exp_avg_sq.data_ptr(), self.n, self.lr, self.betas[0], self.betas[1], self.eps,
                                                      self.state.data_ptr(), self.record.data_ptr(), n_seg, self.max_grad_norm or 0.0,
                                                      int(self.skip_nonfinite), self.guard.data_ptr(), _lib.F32, stream),
                           "ffwm_adam_step_guarded")
            elif self.capturable:
                _lib.check(_lib.load().ffwm_adam_step_device(self.params.data_ptr(), g.data_ptr(), self.exp_avg.data_ptr(),
                                                             self.exp_avg_sq.data_ptr(), self.n, self.lr, self.betas[0], self.betas[1],
                                                             self.eps, self.state.data_ptr(), _lib.F32,
                                                             torch.cuda.current_stream(dev).cuda_stream), "ffwm_adam_step_device")
            else:
                _lib.check(_lib.load().ffwm_adam_step(self.params.data_ptr(), g.data_ptr(), self.exp_avg.data_ptr(),
                                                      self.exp_avg_sq.data_ptr(), self.n, self.lr, self.betas[0], self.betas[1],
                                                      self.eps, self.steps, _lib.F32, torch.cuda.current_stream(dev).cuda_stream),
                           "ffwm_adam_step")
        finally:
            if cur != dev:
                torch.cuda.set_device(cur)

    def zero_grad(self, set_to_none=False):      # the reducer owns the gradients
        self.reducer.flat[self.lo:self.hi].zero_()

    def health(self):
        """What the last step() -- eager or a replay -- saw and decided, in ONE device-to-host copy:
        {segment name: {"norm", "max_abs", "nonfinite", "n"}} (norm and max_abs over the finite elements) plus "scale" (the clip
        factor of that step; 0.0 when it was skipped), "skipped" (that step), "steps_skipped", "steps_seen" and "steps_applied".
        Parameters and moments of a skipped step are untouched; BatchNorm running statistics are not part of the guard."""
        if not self.guarded:
            raise RuntimeError("FlatAdam.health() needs monitor, skip_nonfinite or max_grad_norm")
        host = self._health.cpu().tolist()
        out = {}
        for k, (name, _) in enumerate(self.segments):
            sumsq, max_abs, bad, count = host[4 * k:4 * k + 4]
            out[name] = {"norm": math.sqrt(sumsq), "max_abs": max_abs, "nonfinite": int(bad), "n": int(count)}
        skip, scale, skipped, seen = host[4 * len(self.segments):4 * len(self.segments) + 4]
        out.update({"scale": scale, "skipped": bool(skip), "steps_skipped": int(skipped), "steps_seen": int(seen),
                    "steps_applied": int(seen) - int(skipped)})
        return out


class FlatSGD(object):
    """torch.optim.SGD (momentum, dampening 0, no Nesterov) with per-group learning rate and weight decay as ONE streaming kernel per
    step over flat arrays (csrc/sgd.hip) -- FlatAdam's sibling for lightcnn/finetune.py:74-90, which builds one group per tensor.

    ``param_groups``: torch's form, dicts with 'params' (a tensor or a list), 'lr' and 'weight_decay' (missing keys take the
    ``lr`` / ``weight_decay`` defaults).  The parameters become views of one flat array laid out like the reducer's gradient array;
    every parameter is a segment of it (its padding included), and the segments whose (lr, weight_decay) are equal share one of at
    most 16 device groups.  ``self.param_groups`` keeps one entry per group the caller passed: a scheduler writes
    ``param_groups[i]['lr']``, and ``sync_lr()`` (called by step(), or from the host before a replay) puts the changed values into
    the device tables, where a captured step reads them.

    ``capturable`` exists for interface parity with FlatAdam (the trainers pass it and look it up in ``param_groups[0]``): the kernel
    always reads its rates from the device tables and keeps no step counter, so every FlatSGD step can sit inside a captured hipGraph.
    Likewise the 'momentum' entry of a group is torch's key for readers of ``param_groups``; the step uses ``self.momentum``."""

    MAX_GROUPS = 16
    MAX_SEGMENTS = 1024

    def __init__(self, param_groups, reducer, momentum=0.9, capturable=False, lr=1e-3, weight_decay=0.0):
        groups = []
        for g in param_groups:
            ps = [g["params"]] if torch.is_tensor(g["params"]) else list(g["params"])
            ps = [p for p in ps if p.requires_grad]
            if ps:
                groups.append({"params": ps, "lr": float(g.get("lr", lr)), "weight_decay": float(g.get("weight_decay", weight_decay)),
                               "momentum": float(momentum), "capturable": bool(capturable)})
        params = [p for g in groups for p in g["params"]]
        if reducer.flat is None or not params:
            raise ValueError("FlatSGD needs a reducer with one flat gradient array and at least one parameter")
        if len(set(map(id, params))) != len(params):
            raise ValueError("FlatSGD: a parameter appears in more than one group")
        spans = sorted(reducer.offset[p] for p in params)
        self.lo, self.hi = spans[0][0], spans[-1][1]
        inside = [p for p, (a, b) in reducer.offset.items() if a >= self.lo and b <= self.hi]
        if len(inside) != len(params) or set(map(id, inside)) != set(map(id, params)):
            raise ValueError("FlatSGD: the parameters are not a contiguous range of the reducer's flat layout")
        if self.lo % 4:
            raise ValueError("FlatSGD: range start is not 16-byte aligned")
        if len(params) > self.MAX_SEGMENTS:
            raise ValueError("FlatSGD: at most %d parameter tensors (csrc/sgd.hip stages the segment table in LDS)" % self.MAX_SEGMENTS)
        self.reducer = reducer
        self.momentum = float(momentum)
        n = self.hi - self.lo
        dev, dt = reducer.flat.device, reducer.flat.dtype
        if dt != torch.float32 or dev.type != "cuda":
            raise NotImplementedError("FlatSGD runs on float32 CUDA parameters only (csrc/sgd.hip)")
        self.params = torch.zeros(n, device=dev, dtype=dt)
        self.momentum_buf = torch.zeros(n, device=dev, dtype=dt)
        with torch.no_grad():
            for p in params:
                a, b = reducer.offset[p]
                view = self.params[a - self.lo:b - self.lo].view_as(p)
                view.copy_(p.data)
                p.data = view
                p._ffwm_flat_adam = True       # updated by a raw-pointer kernel: the version counter does not see it (conv.frozen_cache)
        self.n = n
        self.steps = 0
        self.capturable = bool(capturable)
        self.param_groups = groups
        # a segment = one parameter and the padding behind it: it ends where the next parameter begins
        owner = {id(p): i for i, g in enumerate(groups) for p in g["params"]}
        order = sorted(params, key=lambda p: reducer.offset[p][0])
        self._seg_owner = [owner[id(p)] for p in order]
        ends = [reducer.offset[p][0] - self.lo for p in order[1:]] + [n]
        self.seg_end = torch.tensor(ends, dtype=torch.int64, device=dev)
        self.seg_group = torch.zeros(len(order), dtype=torch.int32, device=dev)
        self.group_lr = torch.zeros(self.MAX_GROUPS, dtype=torch.float64, device=dev)
        self.group_wd = torch.zeros(self.MAX_GROUPS, dtype=torch.float64, device=dev)
        self._on_device = None
        self.sync_lr()

    def sync_lr(self):
        """Put the (lr, weight_decay) of every caller group into the device tables when any of them changed since the last call.
        Outside a capture only: a replay runs no Python, so call it (or step()) from the host after the scheduler ran.
        -> the learning rates, one per caller group."""
        pairs = [(float(g["lr"]), float(g["weight_decay"])) for g in self.param_groups]
        if pairs != self._on_device and not torch.cuda.is_current_stream_capturing():
            table = sorted(set(pairs))
            if len(table) > self.MAX_GROUPS:
                raise ValueError("FlatSGD: %d different (lr, weight_decay) settings, csrc/sgd.hip takes %d" % (len(table), self.MAX_GROUPS))
            index = {pair: i for i, pair in enumerate(table)}
            pad = self.MAX_GROUPS - len(table)
            # written in place: a captured step holds these addresses
            self.seg_group.copy_(torch.tensor([index[pairs[o]] for o in self._seg_owner], dtype=torch.int32))
            self.group_lr.copy_(torch.tensor([t[0] for t in table] + [0.0] * pad, dtype=torch.float64))
            self.group_wd.copy_(torch.tensor([t[1] for t in table] + [0.0] * pad, dtype=torch.float64))
            self._on_device = pairs
        return [p[0] for p in pairs]

    def step(self):
        self.sync_lr()
        self.steps += 1
        g = self.reducer.flat[self.lo:self.hi]
        dev = self.params.device.index
        cur = torch.cuda.current_device()
        if cur != dev:
            torch.cuda.set_device(dev)
        try:
            _lib.check(_lib.load().ffwm_sgd_step(self.params.data_ptr(), g.data_ptr(), self.momentum_buf.data_ptr(), self.n,
                                                 self.seg_end.data_ptr(), self.seg_group.data_ptr(), self.seg_end.numel(),
                                                 self.group_lr.data_ptr(), self.group_wd.data_ptr(), self.MAX_GROUPS, self.momentum,
                                                 _lib.F32, torch.cuda.current_stream(dev).cuda_stream), "ffwm_sgd_step")
        finally:
            if cur != dev:
                torch.cuda.set_device(cur)

    def zero_grad(self, set_to_none=False):      # the reducer owns the gradients
        self.reducer.flat[self.lo:self.hi].zero_()
