#!/usr/bin/env python
"""bench.py -- FFWM flow-warp hot path on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload train|flownet|flowtrain|warp|warpatt|ops]
                    [--dump-outputs DIR] [--full]

A plain run sets up, runs W untimed and K timed steps, writes the last timed step's outputs when --dump-outputs is given, and
prints the lines below with the headline figure (metric / value / unit / ms_per_step).  Everything else -- the kernel rows of the
captured step, the roofline copy probe, the `subpaths` legs, the stand-alone operator shapes, the CPU baseline, the all-reduce
sweep of several ranks and the conv flop count -- runs only with --full (the --no-* switches still trim a --full run).

Default workload = BASELINE.json configs[2]: the full FFWM train step (netG + netD + flowNetF + flowNetB, all losses,
three Adam optimizers) on synthetic MultiPIE-shaped 128x128 tensors, batch 8 PER GPU (weak scaling; N > 1 is
configs[3]: DP with RCCL all-reduce of gradient buckets overlapped with backward).  One "step" = one optimisation step
on one batch resident in HBM.  fp32 throughout (the reference's dtype).  Rank 0 prints two verbose JSON lines
({"kernels": [...]}, {"detail": {...}}) and then, as the LAST stdout line, ONE compact (< 4 KB) JSON object -- the line the
driver parses -- with the contract's keys (emit_lines):

  metric/value/unit : train img/s, whole job (W untimed steps, then exactly K steps between barrier + synchronize; one GPU: each
                      step from the same set-up weights, timed by HIP events around it -- timed_from)
  roofline          : the SURVEY 8 a1-a6 kernel (warp / resample2d / block_extractor / local_attn_reshape family) that
                      moves the most algorithmic bytes inside the timed region: algorithmic bytes per launch / average
                      launch duration (HIP events on its launch stream, ffwm_prof_*) vs the 8 TB/s HBM peak;
                      traffic = PMC-measured HBM bytes per launch (profiles/r04_pmc_traffic.json, rocprofv3 FETCH_SIZE /
                      WRITE_SIZE passes of this same command) or null when no valid measurement is committed
  roofline_mfma     : the hand-written MFMA kernel with the largest share of the step (the Winograd convolution, forward + data
                      gradient scopes together); roofline_mfma_2nd: the next one (the 3x3 weight gradient)
  kernels           : the same figures for every hand-written kernel seen in the timed region and for the stand-alone
                      operator shapes of configs[0] / [4] (cfg-1 resample2d, cfg-5 block_extractor / local_attn_reshape)
  subpaths          : (N = 1) the other scopes SURVEY 8(d) asks for, each timed the same way on a few steps:
                      warp_attention_path (netG's warp + flip + cat + attention convs + multiply, base_networks.py:323-333,
                      forward and forward + backward), flownet_fwd_cfg2 (BASELINE configs[1]), train_titers_ge_20000
                      (the guided-filter branch of ffwm_model.py:97-105), train_flow_init_random
  cpu_baseline      : (N = 1, rank 0) the same train step on the host CPU cores -- this repo's PyTorch modules with the
                      oracle's C/OpenMP warp -- on a bounded sample, all usable cores; cpu_baseline_n4 = 4 threads, the
                      reference's own setting (train_ffwm.py:59)

Launch for N > 1:  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
                   --master-port P bench.py --gpus N --steps K --warmup W
"""
import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

HBM_PEAK = 8.0e12          # B/s, MI355X HBM3E spec (/opt/skills/guides/MI355X_MICROARCH.md)
FP32_PEAK = 157.3e12       # FLOP/s, fp32 vector/MFMA
REF_TRAIN_FLOP_PER_IMG = 444e9   # the REFERENCE's step, ~222 GMAC per image (quoted for comparison only)
PMC_FILE = next((p for p in (os.path.join(ROOT, "profiles", "r%02d_pmc_traffic.json" % r) for r in (6, 5, 4, 3, 2)) if os.path.exists(p)),
                os.path.join(ROOT, "profiles", "r05_pmc_traffic.json"))            # the newest committed counter passes
# launch scopes of the SURVEY 8 a1-a6 operators (ffwm_prof_* names)
HOT_PATH_PREFIXES = ("warp", "resample2d", "block_extractor", "local_attn_reshape", "block_attention")


# ---- output contract ------------------------------------------------------------------------------------------------
# The driver parses the LAST stdout line as one JSON object.  Round 3 printed a single 23 KB object and the driver could not
# parse it (BENCH_r03.json parsed: null), so the long material goes out first on lines of its own ({"kernels": [...]},
# {"detail": {...}}) and the last line is a compact (< 4 KB) object with the contract's keys in the contract's order.
FINAL_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline")
FINAL_LIMIT = 4096


def _short(v, n):
    return v if not isinstance(v, str) or len(v) <= n else v[:n - 3] + "..."


def _slim_roofline(r):
    if not isinstance(r, dict):
        return r
    keep = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "avg_us", "launches", "alg_MB_per_launch",
            "alg_GFLOP_per_launch", "frac_binding_roofline", "warp_kernels_GBps", "warp_kernels_frac_hbm_peak", "copy_same_bytes_us",
            "copy_same_bytes_frac_cold")
    return {k: r[k] for k in keep if k in r}


# The per-config operator figures of the final line (SURVEY 8(d) scopes i-ii; BASELINE configs[0], [1], [4]): key -> (kernel scope,
# substring of the row's `where`).  Each value is [avg us, fraction of the 8 TB/s HBM peak] of ONE stand-alone launch at the named
# configuration, HIP-event timed by the library profiler on the launch stream; cfg5 rows at the per-GPU shape, bench flow ~ U[-2, 2).
OPS_ROWS = (
    ("cfg1_rs_fwd", "resample2d_fwd_lds", "cfg1 resample2d ks=4 [1,64"),
    ("cfg1_rs_bwd1", "resample2d_bwd_input1_taplane", "cfg1 resample2d ks=4 backward"),
    ("cfg1_rs_bwd2", "resample2d_bwd_input2_lds", "cfg1 resample2d ks=4 backward"),
    ("rs_fwd@512", "resample2d_fwd_lds", "HBM-resident resample2d ks=4 [8,64,512,512] flow"),
    # (owned: round 6, the owned tiles + their far complement as ONE scope; tile: round 5; auto: rounds 3-4)
    ("rs_bwd1@512", ("resample2d_bwd_input1_owned", "resample2d_bwd_input1_tile", "resample2d_bwd_input1_auto"), "backward, flow~U[-3,3)"),
    ("rs_bwd1@512_smooth", ("resample2d_bwd_input1_owned", "resample2d_bwd_input1_tile", "resample2d_bwd_input1_auto"), "backward, smooth flow"),
    ("rs_bwd2@512", "resample2d_bwd_input2_lds", "backward, flow~U[-3,3)"),
    ("cfg5_be_fwd", "block_extractor_fwd_lds", "src[4,128,256,256] flow~U[-2,2)"),
    ("cfg5_be_bwd", "block_extractor_bwd_tile2", "block_extractor k=3 backward"),
    ("cfg5_be_bwd_smooth", "block_extractor_bwd_tile2", "backward, smooth flow"),
    ("cfg5_lar", "local_attn_reshape_fwd", "cfg5/GPU local_attn_reshape"),
    ("cfg5_lar_bwd", "local_attn_reshape_bwd", "cfg5/GPU local_attn_reshape"),
    ("cfg5_battn_fwd", "block_attention_fwd_lds", "block attention"),
    # (round 6: the WHOLE backward -- far + d(source) + d(flow, weights) launches, "+" = sum of the scopes' times against the operator's
    # algorithmic bytes, which the first scope carries; rounds 4-5 reported the tile2 launch alone, next to a 170 us weights launch)
    ("cfg5_battn_bwd", ("+", "block_attention_bwd_src", "block_attention_bwd_pix", "block_attention_bwd_far"), "block attention"),
    ("warp_fwd@256", "warp_flipcat_fwd@256", "HBM-resident warp"),
    ("warp_bwd_flow@256", "warp_flipcat_bwd_flow@256", "HBM-resident warp"),
    ("warp_bwd_feat@256", "warp_flipcat_bwd_feat_tile@256", "HBM-resident warp"),
)


def ops_summary(kernels, subpaths=None):
    """{key: [avg_us, frac of HBM peak]} for the rows of OPS_ROWS found among `kernels` (first match; the rows of the timed region are
    skipped), plus flownet_fwd_cfg2 = [us per forward of batch 6, fraction of the fp32 MFMA peak] (BASELINE configs[1])."""
    out = {}
    for key, scope, where in OPS_ROWS:
        if isinstance(scope, tuple) and scope[0] == "+":
            found = {}
            for r in kernels:
                if r.get("kernel") in scope[1:] and where in r.get("where", "") and r.get("where") != "timed region":
                    found.setdefault(r["kernel"], r)
            if scope[1] in found:
                us = sum(r["avg_us"] for r in found.values())
                out[key] = [round(us, 2), round(found[scope[1]]["alg_MB"] * 1e6 / (us * 1e-6) / HBM_PEAK, 4)]
            continue
        for r in kernels:
            if r.get("kernel") in ((scope,) if isinstance(scope, str) else scope) and where in r.get("where", "") and r.get("where") != "timed region":
                out[key] = [r["avg_us"], r["frac_hbm_peak"]]
                break
    fl = (subpaths or {}).get("flownet_fwd_cfg2")
    if isinstance(fl, dict) and "ms_per_fwd" in fl:
        out["flownet_fwd_cfg2"] = [round(fl["ms_per_fwd"] * 1e3, 1), fl.get("fp32_flop_frac")]
    return out


def emit_lines(result):
    """The stdout lines of one bench run: verbose lines first, the compact judged line LAST."""
    result = dict(result)
    ops_rows = ops_summary(result.get("kernels", []), result.get("subpaths"))
    lines = [json.dumps({"kernels": result.pop("kernels", [])})]
    detail_keys = [k for k in result if k not in FINAL_KEYS]
    detail = {k: result[k] for k in detail_keys}
    detail["roofline_full"] = result.get("roofline")
    detail["config_full"] = result.get("config")
    lines.append(json.dumps({"detail": detail}))
    final = {}
    for k in FINAL_KEYS:
        v = result.get(k)
        if k == "config" and isinstance(v, dict):
            v = {kk: _short(vv, 160) for kk, vv in v.items()
                 if kk in ("workload", "batch_per_gpu", "global_batch", "parallelism", "launch") or isinstance(vv, (int, float, bool))}
        elif k == "roofline":
            v = _slim_roofline(v)
        elif k == "cpu_baseline" and isinstance(v, dict):
            v = {kk: _short(vv, 200) for kk, vv in v.items()}
        final[k] = v
    for k in ("roofline_mfma", "roofline_mfma_2nd", "roofline_hbm_other"):
        if k in result:
            final[k] = _slim_roofline(result[k])
    if isinstance(result.get("cpu_baseline_n4"), dict):
        final["cpu_baseline_n4"] = {kk: _short(vv, 120) for kk, vv in result["cpu_baseline_n4"].items()}
    for k in ("img_per_s_per_gpu", "fp32_flop_frac", "dp", "allreduce"):
        if k in result:
            final[k] = result[k]
    wa = (result.get("subpaths") or {}).get("warp_attention_path") or result.get("warp_attention_path")
    if isinstance(wa, dict):
        final["warp_attention_path"] = {k: wa[k] for k in ("fwd_img_per_s", "fwd_bwd_img_per_s", "fwd_bwd_ms", "own_kernel_ms_per_pass", "top5",
                                                         "fp32_ceiling_img_per_s") if k in wa}
    if ops_rows:
        # [us, fraction of the roofline] per stand-alone operator launch at BASELINE's configurations (OPS_ROWS)
        final["ops"] = ops_rows
        final["ops_note"] = ("[avg us, frac of 8 TB/s] per stand-alone launch, HIP events; cold caches (512 MiB read between launches) except "
                             "cfg1 / lar (cache-resident sizes); battn_bwd: the WHOLE backward (3 launches); flownet: [us/fwd bs6, frac of 157 TF]")
    if isinstance(final.get("roofline"), dict) and result.get("kernel_rows_from"):
        final["roofline"]["rows_from"] = result["kernel_rows_from"]
    line = json.dumps(final)
    for k in ("allreduce", "roofline_hbm_other", "roofline_mfma_2nd", "cpu_baseline_n4", "ops_note", "roofline_mfma"):   # never exceed the limit
        if len(line) < FINAL_LIMIT:
            break
        final.pop(k, None)
        line = json.dumps(final)
    lines.append(line)
    return lines


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="train", choices=["train", "flownet", "flowtrain", "warp", "warpatt", "ops"])
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch (default: 8 train, 6 flownet)")
    ap.add_argument("--titers", type=int, default=0, help="0 = warm-up branch (<20000), 20000 = guided-filter branch")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-kernels", action="store_true", help="skip the stand-alone cfg-1 / cfg-5 operator shapes")
    ap.add_argument("--no-extras", action="store_true", help="skip the `subpaths` legs (N = 1 only)")
    ap.add_argument("--bucket-mb", type=int, default=64)
    ap.add_argument("--no-dp-ingraph", action="store_true",
                    help="several ranks: do not time the in-graph capture mode (all-reduces overlapping backward) after the serial one")
    ap.add_argument("--flow-init", default="fit-identity", choices=["fit-identity", "random"],
                    help="train workload: stand-in for the reference's PRETRAINED flow nets -- fit flowNetF/B to the identity "
                         "sampling grid for 80 untimed Adam steps (default), or leave them randomly initialised")
    ap.add_argument("--mfma-wgrad", default="on", choices=["on", "off"],
                    help="weight gradients of netG's large 3x3 convs on the hand-written MFMA kernel (off: vendor library)")
    ap.add_argument("--graph", default="auto", choices=["auto", "on", "off"],
                    help="train workload: replay the step from captured hipGraphs (default since round 3: 45.3 vs 52.1 ms on one GPU -- the "
                         "captured step runs the same flat Adam / packed-gradient kernels as the eager one, with flowNetB and the loss "
                         "networks' side passes on their own streams; several ranks: three graphs with the all-reduces between them) or "
                         "run it eagerly (several ranks: hook-launched all-reduces overlapping backward)")
    ap.add_argument("--flownet-path", default="lean", choices=["lean", "module"],
                    help="flownet workload: the launch-lean eval path (BatchNorm folded, fused heads, hipGraph) or the nn.Module")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64; "
                         "arrays above %d elements as a fixed seeded sample of that many)" % DUMP_SAMPLE)
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline figure: kernel rows and roofline probes, the subpaths, the "
                         "stand-alone operator shapes, the CPU baseline, the all-reduce sweep, the conv flop count")
    return ap.parse_args()


# ---- --dump-outputs -----------------------------------------------------------------------------------------------------
DUMP_SAMPLE = 1 << 20            # elements kept of a larger array (4 MiB in float32)
DUMP_LIMIT = 64 << 20            # bytes, all files together


def dump_outputs(path, arrays):
    """Write `arrays` ({name: tensor or float}) as path/<name>.npy.  Floating tensors keep float64 or become float32; an array of
    more than DUMP_SAMPLE elements is reduced to the elements at DUMP_SAMPLE sorted indices drawn from a generator seeded by its
    size, so that two runs (or two builds) with the same arguments write the same positions.  With the same arguments the inputs are
    the same every run and so, up to the rounding of the kernels' float atomics, are the outputs (the train workload: fit_flow_identity,
    timed_from)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    total = 0
    for name, v in arrays.items():
        if torch.is_tensor(v):
            v = v.detach()
            v = v.double() if v.dtype == torch.float64 else v.float()
            flat = v.reshape(-1)
            if flat.numel() > DUMP_SAMPLE:
                g = torch.Generator().manual_seed(flat.numel())
                idx = torch.randint(flat.numel(), (DUMP_SAMPLE,), generator=g).sort().values
                flat = flat[idx.to(flat.device)]
                v = flat
            a = v.cpu().numpy()
        else:
            a = np.asarray(v, dtype=np.float64)
        total += a.nbytes
        if total > DUMP_LIMIT:
            raise RuntimeError("--dump-outputs: more than %d bytes" % DUMP_LIMIT)
        np.save(os.path.join(path, name + ".npy"), a)
    return sorted(arrays)


def net_parameters(net):
    """a network's parameters, flattened and concatenated in named_parameters() order"""
    return torch.cat([p.detach().reshape(-1).float() for _, p in net.named_parameters()])


def train_outputs(t):
    """What the step computed from its inputs: its losses and the forward's images and flows (flowNetF's 128 px flow, netG's three
    reconstructions, the guided-filter output).  The weights after its Adam update are left out: Adam divides every gradient by its
    own running magnitude, so the float atomics' rounding in a gradient that is ~0 becomes a full-size update in either direction."""
    def collect():
        out = {"loss_" + k: float(v.detach()) for k, v in t.losses.items()}
        for name in ("fake32", "fake64", "fake128", "img_GF128"):
            if torch.is_tensor(getattr(t, name, None)):
                out[name] = getattr(t, name).detach().clone()
        flows = getattr(t, "flows_F", None)
        if flows:
            out["flow_F128"] = flows[0].detach().clone()
        return out
    return collect


def init_dist(args):
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # FFWM_DIST_BACKEND=gloo lets the launch path be exercised on a box with fewer GPUs than ranks
        # (ranks then share devices; RCCL refuses that).  The driver's runs use the default: nccl = RCCL.
        backend = os.environ.get("FFWM_DIST_BACKEND", "nccl")
        local = local % torch.cuda.device_count() if backend != "nccl" else local
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    else:
        torch.cuda.set_device(0)
    if args.gpus != world and rank == 0 and world > 1:
        print("warning: --gpus %d but WORLD_SIZE %d" % (args.gpus, world), file=sys.stderr)
    return world, rank, local


def fit_flow_identity(t, b, steps=80, lr=2e-3):
    """FFWMTrainer.pretrain_flow_identity (the stand-in for the reference's pretrained flow nets: both nets fitted to the identity
    sampling grid, Adam, `steps` steps, `lr`) made reproducible: the fit runs on plain copies of the nets through PyTorch's own
    kernels (MIOpen off) with torch.use_deterministic_algorithms on -- an operation without a deterministic implementation raises --
    and the fitted weights are loaded into the trainer's nets.  On the trainer's kernels the atomics' rounding, amplified by Adam,
    leaves the fitted weights 8-11 % apart from run to run; MIOpen's deterministic mode alone still left them 3-5e-2 apart."""
    from ffwm_amd import nets, trainer
    def grid(s):
        lin = (torch.arange(s, dtype=torch.float32, device=t.device) + 0.5) / s * 2 - 1
        yy, xx = torch.meshgrid(lin, lin, indexing="ij")
        return torch.stack((xx, yy), 0).unsqueeze(0)
    targets = [grid(128), grid(64), grid(32)]
    saved = (torch.backends.cudnn.enabled, torch.are_deterministic_algorithms_enabled(),
             torch.is_deterministic_algorithms_warn_only_enabled())
    torch.backends.cudnn.enabled = False
    torch.use_deterministic_algorithms(True)
    last = []
    try:
        for net in (t.flowNetF, t.flowNetB):
            plain = nets.FlowNet(64).to(t.device)               # FFWMTrainer's flow nets (ngf = 64)
            missing, _ = plain.load_state_dict(net.state_dict(), strict=False)
            assert not set(missing) & set(n for n, _ in plain.named_parameters()), missing
            params = [p for n, p in plain.named_parameters() if not n.startswith("inter_conv_occ")]
            opt = torch.optim.Adam(params, lr=lr, foreach=False)
            for _ in range(steps):
                flows = plain(b["img_S"])
                loss = sum((f - g).abs().mean() for f, g in zip(flows, targets))
                opt.zero_grad(set_to_none=True)
                loss.backward()
                opt.step()
            with torch.no_grad():
                for n, p in net.named_parameters():
                    p.copy_(plain.get_parameter(n))
            last.append(float(loss.detach()))
            del plain, opt
    finally:
        torch.backends.cudnn.enabled = saved[0]
        torch.use_deterministic_algorithms(saved[1], warn_only=saved[2])
    trainer.broadcast_module_state([t.flowNetF, t.flowNetB])
    return last


def state_snapshot(t):
    """What a train step reads besides its batch: every float parameter and buffer of the four trained networks and the optimizers'
    moments, device state (step counter, learning rate) and host step count -> (live tensors, their copies, optimizers, step counts)"""
    opts = [o for o in (t.opt_F, t.opt_G, t.opt_D) if hasattr(o, "exp_avg")]
    if len(opts) != 3:
        raise RuntimeError("state_snapshot: the trainer's optimizers are not FlatAdam")
    live = [x for name in t.MODEL_NAMES for x in itertools.chain(getattr(t, name).parameters(), getattr(t, name).buffers())
            if x.is_floating_point()]
    live += [x for o in opts for x in (o.exp_avg, o.exp_avg_sq, o.state) if x is not None]
    return live, [x.detach().clone() for x in live], opts, [o.steps for o in opts]


def timed_from(snapshot, step_fn, steps, warmup):
    """One GPU: W untimed steps, then exactly K steps, each after the networks' weights, buffers and optimizer state are put back to
    `snapshot`, so that every step computes from the same inputs.  Only the steps are timed (HIP events on the step's stream around
    each step; the copy before it is outside); ms per step = their mean.  Returns (seconds of the K steps, launch-scope rows as
    timed())."""
    from ffwm_amd import _lib
    live, saved, opts, counts = snapshot

    def restore():
        with torch.no_grad():
            torch._foreach_copy_(live, saved)
        for o, n in zip(opts, counts):
            o.steps = n
    for _ in range(warmup):
        restore()
        step_fn()
    torch.cuda.synchronize()
    _lib.prof_reset()
    _lib.prof_enable(True)
    evs = []
    for _ in range(steps):
        restore()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step_fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    _lib.prof_enable(False)
    return sum(a.elapsed_time(b) for a, b in evs) * 1e-3, _lib.prof_collect()


def timed(step_fn, steps, warmup, world):
    """W untimed steps, then exactly K steps between (barrier + synchronize) on both sides; max over ranks.
    Returns (seconds, launch-scope rows of the hand-written kernels inside the timed region)."""
    for _ in range(warmup):
        step_fn()
    from ffwm_amd import _lib
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    _lib.prof_reset()
    _lib.prof_enable(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        step_fn()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    _lib.prof_enable(False)
    rows = _lib.prof_collect()
    if world > 1:
        t = torch.tensor([dt], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt, rows


def pmc_traffic():
    """HBM-side bytes per dispatch measured with rocprofv3 PMC passes of this same command (tools/refresh_profiles.sh:
    --pmc FETCH_SIZE and --pmc WRITE_SIZE in separate runs, --kernel-include-regex ffwm; FETCH_SIZE doubled per the gfx950
    calibration).  PMC counters cannot be read from inside the process, so the committed measurement is attached.  A scope
    whose fetch or write count is missing / zero is NOT reported (tools/fold_profiles.py refuses to write such rows)."""
    try:
        with open(PMC_FILE) as f:
            data = json.load(f)
    except (OSError, ValueError):
        return {}
    return {k: v for k, v in data.items() if not k.startswith("_") and v.get("fetch_KiB", 0) > 0 and v.get("write_KiB", 0) > 0}


def kernel_rows(rows, tag):
    out = []
    for name, r in sorted(rows.items(), key=lambda kv: -kv[1]["total_ms"]):
        if r["avg_ms"] <= 0:
            continue
        bps = r["bytes_per_launch"] / (r["avg_ms"] * 1e-3)
        row = {"kernel": name, "where": tag, "launches": r["launches"], "avg_us": round(r["avg_ms"] * 1e3, 2),
               "total_ms": round(r["total_ms"], 3), "alg_MB": round(r["bytes_per_launch"] / 1e6, 3),
               "GBps": round(bps / 1e9, 1), "frac_hbm_peak": round(bps / HBM_PEAK, 4)}
        if r.get("flops_per_launch", 0) > 0:      # the MFMA kernels (conv3x3_wgrad, correlation_colmax)
            fps = r["flops_per_launch"] / (r["avg_ms"] * 1e-3)
            row.update({"alg_GFLOP": round(r["flops_per_launch"] / 1e9, 3), "TFLOPs": round(fps / 1e12, 2),
                        "frac_mfma_fp32_peak": round(fps / FP32_PEAK, 4)})
            if r.get("roofline_ms", 0) > 0 and r["total_ms"] > 0:
                # every launch priced by whichever of ITS two rooflines binds (a scope serves shapes from MFMA-bound down to
                # weight-streaming): sum of max(bytes / 8 TB/s, flops / 157.3 TFLOP/s) over the launches / measured time
                row["frac_binding_roofline"] = round(r["roofline_ms"] / r["total_ms"], 4)
        out.append(row)
    return out


def is_hot_path(row):
    return row["kernel"].startswith(HOT_PATH_PREFIXES)


def standalone_kernels(reps=10):
    """cfg-1 / cfg-5 operator shapes, HIP-event timed through the library profiler; plus
    resample2d at an HBM-resident shape (cfg-1's 8.6 MB live in L2)."""
    from ffwm_amd import _lib, ops
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    rows = []

    # Round 5: the HBM-sized rows are timed COLD -- a 512 MiB READ (twice the 256 MB Infinity Cache; a read, so that the caches are left
    # full of clean lines and the timed launch does not also pay for another kernel's write-back) runs between the repetitions, outside
    # the per-launch event pairs.  Back-to-back repetitions kept the 134 MB source of the cfg-5 extractor in the cache: HIP events read
    # 209-211 us where rocprofv3 of the ops workload (forward and backward alternating) read 239-261 us.  The cfg-1
    # rows stay warm: that configuration is cache-resident by its size.
    evict = torch.zeros(128 << 20, device=dev)
    evict_sink = torch.zeros((), device=dev)

    def run(tag, fn, n=reps, cold=True):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        _lib.prof_reset()
        for _ in range(n):
            if cold:
                evict_sink.copy_(evict.sum())
            _lib.prof_enable(True)
            fn()
            _lib.prof_enable(False)
        torch.cuda.synchronize()
        rows.extend(kernel_rows(_lib.prof_collect(), tag))

    src = torch.rand(4, 128, 256, 256, generator=g).to(dev)
    flow = (torch.rand(4, 2, 256, 256, generator=g) * 4 - 2).to(dev)
    out = torch.empty(4, 128, 768, 768, device=dev)
    run("cfg5/GPU block_extractor k=3 src[4,128,256,256] flow~U[-2,2)", lambda: ops.block_extractor_forward(src, flow, 3, out=out))
    gs, gf = torch.zeros_like(src), torch.zeros_like(flow)
    run("cfg5/GPU block_extractor k=3 backward", lambda: ops.block_extractor_backward(src, flow, out, 3, gs, gf))
    # a SMOOTH flow of the same amplitude (what a trained flow net produces): no LDS bank / same-cell collisions in the backward's
    # scatter; its extrema sit next to integers, so a few pixels take the per-tap paths (fallback block / far kernel)
    yy, xx = torch.meshgrid(torch.arange(256.0), torch.arange(256.0), indexing="ij")
    smooth = torch.stack([2 * torch.sin(xx / 41.0 + yy / 67.0), 2 * torch.cos(xx / 53.0 - yy / 37.0)]).unsqueeze(0).repeat(4, 1, 1, 1).to(dev)
    run("cfg5/GPU block_extractor k=3 smooth flow, amplitude 2 px", lambda: ops.block_extractor_forward(src, smooth, 3, out=out))
    gs.zero_(); gf.zero_()
    run("cfg5/GPU block_extractor k=3 backward, smooth flow", lambda: ops.block_extractor_backward(src, smooth, out, 3, gs, gf))
    del smooth
    if os.environ.get("FFWM_BENCH_SKIP_FALLBACK") != "1":
        # (tools/r06/refresh.sh sets the switch for its rocprofv3 trace of this workload: the +-64 px calls run the SAME kernel with the same
        # launch geometry -- a block-uniform fallback inside -- and would share the fast path's row of the per-kernel table)
        wide = (torch.rand(4, 2, 256, 256, generator=g) * 128 - 64).to(dev)
        run("cfg5/GPU block_extractor k=3 flow~U[-64,64) (gather fallback)", lambda: ops.block_extractor_forward(src, wide, 3, out=out), 3)
        del wide
    del src, out, gs, gf
    attn = torch.rand(4, 9, 256, 256, generator=g).to(dev)
    o = torch.empty(4, 1, 768, 768, device=dev)
    gi = torch.empty_like(attn)
    run("cfg5/GPU local_attn_reshape k=3 [4,9,256,256]", lambda: ops.local_attn_reshape_forward(attn, 3, out=o), cold=False)      # (9.4 MB: cache-resident)
    run("cfg5/GPU local_attn_reshape k=3 backward", lambda: ops.local_attn_reshape_backward(o, 3, gi), cold=False)
    # netG's residual layer (base_networks.py:293-298): 195 -> 195 channels at 128 x 128, batch 8 -- forward and data gradient on
    # csrc/conv_winograd.hip (TFLOPs = the MFMA flops executed; the direct sum it replaces has 2.25 x as many)
    xw = torch.randn(8, 195, 128, 128, generator=g).to(dev)
    ww = (torch.randn(195, 195, 3, 3, generator=g) * 0.02).to(dev)
    bw = torch.randn(195, generator=g).to(dev)
    ow = torch.empty_like(xw)
    run("netG dres conv3x3 195->195 [8,195,128,128] winograd forward", lambda: ops.conv3x3_winograd(xw, ww, bw, out=ow))
    run("netG dres conv3x3 195->195 [8,195,128,128] winograd data gradient", lambda: ops.conv3x3_winograd(xw, ww, None, data_gradient=True, out=ow))
    del xw, ww, bw, ow
    in1 = torch.rand(1, 64, 128, 128, generator=g).to(dev)
    in2 = torch.cat((torch.rand(1, 2, 128, 128, generator=g) * 6 - 3, torch.full((1, 1, 128, 128), 2.0)), 1).to(dev)
    o = torch.empty_like(in1)
    go = torch.rand(1, 64, 128, 128, generator=g).to(dev)
    g1, g2 = torch.zeros_like(in1), torch.empty_like(in2)
    run("cfg1 resample2d ks=4 [1,64,128,128] flow~U[-3,3)", lambda: ops.resample2d_forward(in1, in2, 4, 1, out=o), cold=False)
    run("cfg1 resample2d ks=4 backward", lambda: ops.resample2d_backward(in1, in2, go, 4, 1, g1, g2), cold=False)
    in1 = torch.rand(8, 64, 512, 512, generator=g).to(dev)
    in2 = torch.cat((torch.rand(8, 2, 512, 512, generator=g) * 6 - 3, torch.full((8, 1, 512, 512), 2.0)), 1).to(dev)
    o = torch.empty_like(in1)
    run("HBM-resident resample2d ks=4 [8,64,512,512] flow~U[-3,3)", lambda: ops.resample2d_forward(in1, in2, 4, 1, out=o), 5)
    # the backward at the same HBM-resident shape (d_input1 = the LDS-accumulator tile kernel, d_input2 = the LDS-staged kernel)
    # (as external_function.Resample2dFunction.backward calls it since round 6: grad_input1 handed over uninitialised -- reference_quirk bit 1 --,
    # the owned tiles store every cell once and the wrapper's 0.54 GB zero-fill is gone)
    go = torch.rand(8, 64, 512, 512, generator=g).to(dev)
    g1, g2 = torch.empty_like(in1), torch.empty_like(in2)
    run("HBM-resident resample2d ks=4 [8,64,512,512] backward, flow~U[-3,3)", lambda: ops.resample2d_backward(in1, in2, go, 4, 1, g1, g2, overwrite_input1=True), 3)
    # ... and with a SMOOTH displacement of the same amplitude (what a flow net produces; the random flow is BASELINE configs[0]'s)
    lin = torch.linspace(-1, 1, 512)
    yy, xx = torch.meshgrid(lin, lin, indexing="ij")
    sm = torch.stack((3 * torch.sin(3.1 * yy + 0.3) * torch.cos(2.3 * xx), 3 * torch.cos(2.7 * xx - 0.2) * torch.sin(1.9 * yy),
                      torch.full((512, 512), 2.0)), 0).unsqueeze(0).repeat(8, 1, 1, 1).contiguous().to(dev)
    run("HBM-resident resample2d ks=4 [8,64,512,512] backward, smooth flow, amplitude 3 px", lambda: ops.resample2d_backward(in1, sm, go, 4, 1, g1, g2, overwrite_input1=True), 3)
    del in1, in2, o, go, g1, g2, sm
    # netG's warp + flip + cat at an HBM-resident shape (the HBM claim is taken from shapes beyond the caches)
    feat = torch.rand(32, 64, 256, 256, generator=g).to(dev)
    nflow = smooth_flow(32, 256).to(dev)
    wo = torch.empty(32, 128, 256, 256, device=dev)
    run("HBM-resident warp+flip+cat [32,64,256,256], smooth flow", lambda: ops.warp_forward(feat, nflow, True, out=wo), 5)
    # (as external_function.WarpFunction.backward calls it since round 5: grad_feat handed over uninitialised and produced whole --
    # flipcat bit 1 -- the owned tiles store instead of read-modify-write and the caller's 0.54 GB zero-fill is gone; grad_flow accumulates)
    gfeat, gflow = torch.empty_like(feat), torch.zeros_like(nflow)
    run("HBM-resident warp+flip+cat [32,64,256,256] backward, smooth flow", lambda: ops.warp_backward(feat, nflow, wo, True, gfeat, gflow, overwrite_feat=True), 3)
    del feat, nflow, wo, gfeat, gflow
    # the fused extractor + attention consumer at cfg-5 per GPU
    src = torch.rand(4, 128, 256, 256, generator=g).to(dev)
    flow = (torch.rand(4, 2, 256, 256, generator=g) * 4 - 2).to(dev)
    wts = torch.rand(4, 9, 256, 256, generator=g).to(dev)
    bo = torch.empty(4, 128, 256, 256, device=dev)
    run("cfg5/GPU block attention k=3 (extract x weights -> avg_pool, fused) forward", lambda: ops.block_attention_forward(src, flow, wts, 3, out=bo))
    gs, gf, gw = torch.zeros_like(src), torch.zeros_like(flow), torch.zeros_like(wts)
    run("cfg5/GPU block attention k=3 backward", lambda: ops.block_attention_backward(src, flow, wts, bo, 3, gs, gf, gw), 5)
    return rows


def host_threads():
    """Threads for the CPU leg: the cores this process may run on, capped at 16 -- PyTorch's CPU
    convolutions at batch 8 stop scaling (and then collapse) well before that on a many-core host."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 16))


def cpu_train_baseline(titers):
    """The same train step on the host cores: this repo's modules on CPU, warps through the oracle's
    C/OpenMP restatement (test infrastructure, used here only as the CPU comparison leg).  Two settings:
    all usable cores (<= 16), and 4 threads -- the reference's own (train_ffwm.py:59)."""
    import oracle
    from ffwm_amd import trainer
    oracle.build()

    def warp(images, flow, mode="bilinear"):
        return oracle.WarpOracleFn.apply(images, flow, False)

    def warp_flipcat(feat, flow):
        return oracle.WarpOracleFn.apply(feat, flow, True)

    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or 1
    bs = 8
    cores = host_threads()
    torch.set_num_threads(cores)
    os.environ["OMP_NUM_THREADS"] = str(cores)
    t = trainer.FFWMTrainer("cpu", seed=0, titers=titers, warp=warp, warp_flipcat=warp_flipcat)
    batch = trainer.synthetic_batch(bs, "cpu", seed=1)
    t.step(batch)                                  # untimed: allocator / oneDNN primitive warm-up
    out = {}
    for key, n, steps in (("cpu_baseline", cores, 2), ("cpu_baseline_n4", min(4, cores), 1)):
        torch.set_num_threads(n)
        t0 = time.perf_counter()
        for _ in range(steps):
            t.step(batch)
        dt = time.perf_counter() - t0
        out[key] = {"value": round(bs * steps / dt, 4), "unit": "img/s", "cores": n, "kind": "port",
                    "host_cores_usable": usable,
                    "sample": "%d full FFWM train step(s), batch %d, after 1 warm-up step, %d torch/OpenMP threads, %.1f s%s"
                              % (steps, bs, n, dt, " (of %d usable cores: measured on this box 16 / 32 / 64 / 128 threads = 1.86 / 1.60 / 0.96 / "
                                 "0.43 img/s -- PyTorch's CPU convolutions at batch 8 stop scaling, then collapse)" % usable
                                 if key == "cpu_baseline" and usable > n else "")}
    return out


def cpu_ops_baseline():
    import oracle
    oracle.build()
    cores = host_threads()
    os.environ["OMP_NUM_THREADS"] = str(cores)
    g = torch.Generator().manual_seed(0)
    src = torch.rand(1, 32, 256, 256, generator=g)
    flow = torch.rand(1, 2, 256, 256, generator=g) * 4 - 2
    t0 = time.perf_counter()
    oracle.block_extractor_forward(src, flow, 3)
    dt = time.perf_counter() - t0
    nbytes = 4.0 * (32 * 65536 + 2 * 65536 + 32 * 9 * 65536)
    return {"cpu_baseline": {"value": round(nbytes / dt / 1e9, 3), "unit": "GB/s", "cores": cores, "kind": "port",
                             "sample": "oracle block_extractor forward, src [1,32,256,256] (1/16 of cfg-5 per GPU), %.2f s" % dt}}


def dp_identity(dev, world):
    """Who is in the job: the world size torch.distributed reports and the DISTINCT devices behind the ranks (one all-gather of the device
    UUIDs / PCI bus ids) -- on the final line, so that a multi-GPU record says by itself that N RCCL ranks on N GPUs produced it."""
    try:
        props = torch.cuda.get_device_properties(dev)
        me = str(getattr(props, "uuid", "")) or "%s:%s" % (getattr(props, "pci_bus_id", "?"), getattr(props, "pci_device_id", "?"))
        ids = [None] * world
        dist.all_gather_object(ids, me)
        return {"rccl_ranks": dist.get_world_size(), "backend": "nccl (= RCCL)" if dist.get_backend() == "nccl" else dist.get_backend(),
                "distinct_devices": len(set(ids))}
    except Exception as e:
        return {"rccl_ranks": world, "error": repr(e)}


def dp_time_ingraph(args, dev, world, rank, batch, bs, fallback):
    """Several ranks, after the `serial` measurement (three graphs, the two gradient all-reduces between them, nothing overlapped): the SAME
    step with the bucket all-reduces captured INSIDE one graph on RCCL's stream, where they overlap the rest of backward -- the mode
    north_star describes.  It has never run between two real RCCL ranks on the development box (one GPU), so it is tried here, on a fresh
    trainer, and counts only when every rank's weights are bit-identical (rank spread 0.0) after two replays; then it is timed for exactly
    the same steps.  A watchdog covers what cannot be tested ahead: should the capture or a replay hang, every rank exits 0 after
    FFWM_DP_INGRAPH_TIMEOUT seconds (default 300) and rank 0 prints the serial result (`fallback()` = its finished lines) first."""
    import threading
    from ffwm_amd import trainer
    out = {"tried": True}
    dist.barrier()
    done = threading.Event()

    def bail():
        if done.is_set():
            return
        if rank == 0:
            for line in fallback("ingraph: no answer within the watchdog's time -- the serial measurement stands"):
                print(line, flush=True)
        os._exit(0)
    timer = threading.Timer(float(os.environ.get("FFWM_DP_INGRAPH_TIMEOUT", "300")), bail)
    timer.daemon = True
    timer.start()
    ok, t2, dt2 = True, None, None
    try:
        t2 = trainer.FFWMTrainer(dev, world_size=world, seed=0, titers=args.titers, bucket_bytes=args.bucket_mb << 20,
                                 capturable=True, mfma_wgrad=args.mfma_wgrad == "on")
        if args.flow_init == "fit-identity":
            t2.pretrain_flow_identity(batch)
        t2.capture(batch, warmup=max(2, args.warmup), mode="ingraph")
        for _ in range(2):
            t2.step(batch, batch_increment=0)
        torch.cuda.synchronize()
        spread = t2.rank_spread()
        out["rank_spread_after_2_replays"] = spread
        if not all(v == 0.0 for v in spread.values()):
            raise RuntimeError("the ranks' weights differ after two replays: %r" % (spread,))
    except Exception as e:
        ok = False
        out["error"] = _short(repr(e), 200)
    flag = torch.tensor([1.0 if ok else 0.0], device=dev)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    ok = float(flag.item()) > 0.5
    if ok:
        dt2, _ = timed(lambda: t2.step(batch, batch_increment=0), args.steps, args.warmup, world)
        out["ms_per_step"] = round(dt2 / args.steps * 1e3, 3)
        out["img_per_s"] = round(bs * world * args.steps / dt2, 2)
    out["valid"] = ok
    done.set()
    timer.cancel()
    del t2
    return out, dt2


def allreduce_sweep(dev, world, sizes_mib=(4, 16, 64, 256)):
    """sum all-reduce of fp32 buffers of 4 ... 256 MiB on the job's process group: ms, algorithm and ring bus bandwidth (the bucket
    size, --bucket-mb, should sit where busbw has saturated)"""
    out = []
    for mib in sizes_mib:
        buf = torch.zeros(mib << 18, device=dev)
        ts = []
        for _ in range(4):
            torch.cuda.synchronize()
            dist.barrier()
            t0 = time.perf_counter()
            dist.all_reduce(buf)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        tm = sorted(ts[1:])[1]
        nbytes = mib << 20
        out.append({"MiB": mib, "ms": round(tm * 1e3, 3), "algbw_GBps": round(nbytes / tm / 1e9, 1),
                    "busbw_GBps": round(2.0 * (world - 1) / world * nbytes / tm / 1e9, 1)})
        del buf
    return out


# ------------------------------------------------------------------------------------------------ workloads
def smooth_flow(bs, s):
    """identity grid + ~3 px of low-frequency displacement: what a trained FlowNet produces"""
    lin = (torch.arange(s, dtype=torch.float32) + 0.5) / s * 2 - 1
    yy, xx = torch.meshgrid(lin, lin, indexing="ij")
    amp = 6.0 / s
    fx = xx + amp * torch.sin(3.1 * yy + 0.3) * torch.cos(2.3 * xx)
    fy = yy + amp * torch.cos(2.7 * xx - 0.2) * torch.sin(1.9 * yy)
    return torch.stack((fx, fy), 0).unsqueeze(0).repeat(bs, 1, 1, 1).contiguous()


def hot_rows_summary(rows):
    """bytes-weighted HBM fraction of the a1-a6 kernels among `rows` + the per-kernel list"""
    hot = [r for r in rows if is_hot_path(r)]
    tot_b = sum(r["alg_MB"] * r["launches"] for r in hot)
    tot_t = sum(r["total_ms"] for r in hot)
    return {"warp_kernels_GBps": round(tot_b / tot_t, 1) if tot_t > 0 else None,
            "warp_kernels_frac_hbm_peak": round(tot_b * 1e6 / (tot_t * 1e-3) / HBM_PEAK, 4) if tot_t > 0 else None,
            "kernels": [{k: r[k] for k in ("kernel", "launches", "avg_us", "alg_MB", "GBps", "frac_hbm_peak")} for r in hot]}


def _top_kernels(rows, passes, n):
    rows = sorted(rows, key=lambda r: -r["total_ms"])[:n]
    return [[r["kernel"], round(r["launches"] / passes, 1), round(r["total_ms"] / passes * 1e3, 1)] for r in rows]


def run_warp_attention(dev, bs, steps, warmup, world, seed=1, graph=True, route=True, kernel_rows_after=True, keep=False):
    """netG's warp-attention module alone (base_networks.py:323-333): warp + flip + cat (HIP) -> att convs -> multiply,
    three levels, batch `bs`.  Returns forward-only and forward + backward figures.  kernel_rows_after: (graph) time the hand-written
    kernels in eager passes after the timed region; keep: also return copies of the gradients of the last timed pass."""
    from ffwm_amd import flops, nets
    torch.manual_seed(0)
    mod = nets.WarpAttention(sn=True).to(dev).train()
    # the att convs run on the kernels they run on inside FFMTrainer's netG: same routes, same order (trainer.py:160-205)
    from ffwm_amd.conv import route_training_kernels
    routed = route_training_kernels(mod, convs=route)
    g = torch.Generator().manual_seed(seed)
    feats = [torch.rand(bs, c, s, s, generator=g).to(dev).requires_grad_(True) for c, s in mod.LEVELS]
    flows = [smooth_flow(bs, s).to(dev).requires_grad_(True) for _, s in mod.LEVELS]
    gos = [torch.rand(bs, 2 * c, s, s, generator=g).to(dev) for c, s in mod.LEVELS]

    def fwd():
        with torch.no_grad():
            mod(feats, flows)

    def fwd_bwd():
        for t in feats + flows:
            t.grad = None
        for p in mod.parameters():
            p.grad = None
        torch.autograd.backward(mod(feats, flows), gos)
    fl = flops.count_step([mod], fwd_bwd)

    def replayed(fn):
        """`fn` as one hipGraph (like the trainer's captured step): three eager passes on a side stream, then the capture"""
        from ffwm_amd.norm import reset_scratch
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        reset_scratch()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            fn()
        return gr.replay

    def last_pass():
        if not keep:
            return {}
        out = {"grad_feat%d" % i: t.grad.clone() for i, t in enumerate(feats)}
        out.update({"grad_flow%d" % i: t.grad.clone() for i, t in enumerate(flows)})
        out["grad_params"] = torch.cat([p.grad.reshape(-1).float() for p in mod.parameters() if p.grad is not None])
        return out

    if graph:
        dt_f, _ = timed(replayed(fwd), steps, warmup, world)
        dt_b, rows_b = timed(replayed(fwd_bwd), steps, warmup, world)
        torch.cuda.synchronize(dev)
        last = last_pass()
        rows_f = {}
        if kernel_rows_after:
            # HIP events cannot bracket kernels inside a replayed graph: the per-kernel rows come from eager passes afterwards
            _, rows_f = timed(fwd, 3, 1, world)
            _, rows_b = timed(fwd_bwd, 3, 1, world)
    else:
        dt_f, rows_f = timed(fwd, steps, warmup, world)
        dt_b, rows_b = timed(fwd_bwd, steps, warmup, world)
        last = last_pass()
    imgs = bs * world * steps
    ceil_fb = FP32_PEAK / (fl["total"] / bs)
    return {"scope": "warp + flip + cat (HIP) + attention convs (conv block + sigmoid residual block, spectral norm) + multiply; "
                     "3 levels ([128,32,32], [64,64,64], [64,128,128] per image), batch %d, smooth flows" % bs,
            "launch": "hipGraph replay" if graph else "eager", "routes": routed,
            "fwd_img_per_s": round(imgs / dt_f, 1), "fwd_ms": round(dt_f / steps * 1e3, 3),
            "fwd_bwd_img_per_s": round(imgs / dt_b, 1), "fwd_bwd_ms": round(dt_b / steps * 1e3, 3),
            "conv_GFLOP_per_img": {"fwd": round(fl["fwd"] / bs / 1e9, 2), "fwd_bwd": round(fl["total"] / bs / 1e9, 2)},
            "fp32_ceiling_img_per_s": {"fwd": round(FP32_PEAK / (fl["fwd"] / bs), 0), "fwd_bwd": round(ceil_fb, 0)},
            "fp32_flop_frac": {"fwd": round(imgs / dt_f * fl["fwd"] / bs / FP32_PEAK, 4),
                               "fwd_bwd": round(imgs / dt_b * fl["total"] / bs / FP32_PEAK, 4)},
            "note": "the att convs are %.1f GFLOP per image forward + backward as a DIRECT sum: %.0f img/s at the fp32 MFMA peak; the Winograd "
                    "kernels execute 2.25 x fewer multiplications, so that figure is a yardstick, not a bound" % (fl["total"] / bs / 1e9, ceil_fb),
            "warp_fwd": hot_rows_summary(kernel_rows(rows_f, "warp_attention fwd")),
            "warp_fwd_bwd": hot_rows_summary(kernel_rows(rows_b, "warp_attention fwd+bwd")),
            # where a forward + backward pass goes: the hand-written kernels with the most time per pass (HIP events of 3 eager passes,
            # [kernel, launches per pass, us per pass]) and their sum beside the replayed pass's wall time -- the rest is vendor / ATen
            "top5": _top_kernels(kernel_rows(rows_b, "warp_attention fwd+bwd"), 3, 5),
            "own_kernel_ms_per_pass": round(sum(r["total_ms"] for r in kernel_rows(rows_b, "warp_attention fwd+bwd")) / 3, 3)}, dt_b, rows_b, last


def run_flownet(dev, bs, steps, warmup, world, path, seed=1):
    from ffwm_amd import flops, nets
    torch.manual_seed(0)
    net = nets.FlowNet(64).to(dev).eval()
    x = torch.rand(bs, 3, 128, 128, generator=torch.Generator().manual_seed(seed)).to(dev)
    with torch.no_grad():
        fl = flops.count_step([net], lambda: net(x))
    last = {}
    if path == "lean":
        from ffwm_amd import flownet_eval
        lean = flownet_eval.FoldedFlowNet(net, graph=True)

        def step():
            last["flows"] = lean(x)
    else:
        def step():
            with torch.no_grad():
                last["flows"] = net(x)
    dt, rows = timed(step, steps, warmup, world)
    imgs = bs * world * steps
    return {"img_per_s": round(imgs / dt, 1), "ms_per_fwd": round(dt / steps * 1e3, 4), "batch": bs, "path": path,
            "conv_GFLOP_per_img": round(fl["fwd"] / bs / 1e9, 3),
            "fp32_flop_frac": round(imgs / dt / world * fl["fwd"] / bs / FP32_PEAK, 5)}, dt, rows, last


def main():
    args = parse()
    world, rank, local = init_dist(args)
    if args.graph == "auto":
        args.graph = "on" if args.workload in ("train", "flowtrain", "warpatt") else "off"
    dev = torch.device("cuda", local)
    # MIOpen ships no gfx950 kernel database in this image: every conv kernel is JIT-compiled on a
    # fresh box.  Exhaustive find mode multiplies that start-up cost by the number of candidate
    # solvers (~10 min), so it is opt-in; the default is MIOpen's heuristic ("immediate") choice.
    torch.backends.cudnn.benchmark = os.environ.get("FFWM_MIOPEN_FIND", "0") == "1"
    from ffwm_amd import _lib, miopen_tuning
    # solver selection from the in-tree find-db (ffwm_amd/miopen_db, 245 KB of MIOpen's own text records for the
    # convolutions of this workload on gfx950 / 256 CUs): immediate mode, no find pass at start-up
    miopen_db = miopen_tuning.install()
    _lib.load()                                # fail loudly if the HIP library is missing

    result = {"n_gpus": world, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True,
              "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic"}
    extras = {}
    t = None
    outputs = None          # () -> {name: tensor or float}: what the last timed step computed (--dump-outputs), taken right after timing

    if args.workload == "train":
        from ffwm_amd import flops, trainer
        bs = args.batch or 8
        t = trainer.FFWMTrainer(dev, world_size=world, seed=0, titers=args.titers,
                                bucket_bytes=args.bucket_mb << 20, capturable=args.graph == "on",
                                mfma_wgrad=args.mfma_wgrad == "on")
        batch = trainer.synthetic_batch(bs, dev, seed=1 + rank)
        flow_fit = fit_flow_identity(t, batch) if args.flow_init == "fit-identity" else None
        # one GPU: every warm-up and timed step starts from the weights set up so far (see timed_from)
        snapshot = state_snapshot(t) if world == 1 else None
        graphed = args.graph == "on"
        nets_all = [t.flowNetF, t.flowNetB, t.netG, t.netD, t.lightCNN, t.vgg]
        step_flops = None
        if graphed:            # count on a throw-away eager trainer: hooks + an eager step before capture() must not touch the graphed one
            if args.full:
                tc = trainer.FFWMTrainer(dev, world_size=1, seed=0, titers=args.titers, mfma_wgrad=args.mfma_wgrad == "on")
                step_flops = flops.count_step([tc.flowNetF, tc.flowNetB, tc.netG, tc.netD, tc.lightCNN, tc.vgg],
                                              lambda: tc.step(batch, batch_increment=0))
                del tc
        else:
            step_flops = flops.count_step(nets_all, lambda: t.step(batch, batch_increment=0))       # one untimed eager step
        capture_mode, d_side, dp_spread = None, False, None
        if graphed:
            # several ranks: the capture modes of FFWMTrainer.capture, best first -- "ingraph" (RCCL captured into ONE graph, every
            # bucket's all-reduce overlapping backward; chosen by a probe graph every rank must replay correctly), then "serial" (three
            # graphs, the all-reduces between them).  Should a capture or its first replay fail beside the live process group (several
            # RCCL ranks cannot be tried on the one-GPU development box), the ranks agree on it and try the next mode on a fresh
            # trainer; the last resort is the eager step with hook-launched, overlapped all-reduces.
            forced = os.environ.get("FFWM_DP_CAPTURE")
            # (round 5, ADVICE r4: "serial" first -- the in-graph capture of the collectives is opt-in, FFWM_DP_CAPTURE=ingraph, until it
            # has run between >= 2 real RCCL ranks; "auto" = probe, then ingraph)
            modes = [None] if world == 1 else ([forced, "serial"] if forced else ["serial"])
            tried, captured = [], False
            for m in modes:
                mode = m
                if m == "auto":
                    mode = "ingraph" if trainer.probe_collective_capture(dev) else "serial"
                if mode in tried:
                    continue
                tried.append(mode)
                if t is None:
                    t = trainer.FFWMTrainer(dev, world_size=world, seed=0, titers=args.titers, bucket_bytes=args.bucket_mb << 20,
                                            capturable=True, mfma_wgrad=args.mfma_wgrad == "on")
                    flow_fit = fit_flow_identity(t, batch) if args.flow_init == "fit-identity" else None
                ok = True
                try:
                    t.capture(batch, warmup=max(2, args.warmup), mode=mode)
                    if world > 1:                       # replays must run -- and leave the ranks in lock step -- before the mode counts as working
                        for _ in range(2):
                            t.step(batch, batch_increment=0)
                        torch.cuda.synchronize()
                        spread = t.rank_spread()
                        dp_spread = spread
                        if not all(v == v and v <= 1e-5 for v in spread.values()):
                            raise RuntimeError("the ranks' weights differ after two replays: %r" % (spread,))
                except Exception as e:
                    if world == 1:
                        raise
                    ok = False
                    print("rank %d: hipGraph capture (mode %s) failed (%r)" % (rank, mode, e), file=sys.stderr)
                if world > 1:
                    flag = torch.tensor([1.0 if ok else 0.0], device=dev)
                    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                    ok = float(flag.item()) > 0.5
                if ok:
                    captured = True
                    capture_mode, d_side = t.capture_mode, bool(t._d_side and t.d_stream is not None)
                    break
                del t
                t = None
                torch.cuda.synchronize()
            if not captured:
                graphed = False
                args.graph = "off"
                t = trainer.FFWMTrainer(dev, world_size=world, seed=0, titers=args.titers, bucket_bytes=args.bucket_mb << 20,
                                        capturable=False, mfma_wgrad=args.mfma_wgrad == "on")
                flow_fit = fit_flow_identity(t, batch) if args.flow_init == "fit-identity" else None
            nets_all = [t.flowNetF, t.flowNetB, t.netG, t.netD, t.lightCNN, t.vgg]
        if snapshot is not None:
            dt, rows = timed_from(snapshot, lambda: t.step(batch, batch_increment=0), args.steps, args.warmup)
        else:
            dt, rows = timed(lambda: t.step(batch, batch_increment=0), args.steps, args.warmup, world)
        if args.dump_outputs:
            outputs = train_outputs(t)()
        if graphed and args.full:
            # HIP events cannot bracket kernels inside a replayed graph: time the hand-written kernels
            # in two EAGER steps of the same trainer right after the timed region -- on ONE stream: beside the side streams'
            # kernels a launch shares the chip and the event pair around it measures the sharing, not the kernel (round 4: with the
            # loss networks' ground-truth passes running beside netG's forward the Winograd rows read 0.46 instead of 0.53)
            t.release_graphs()
            t.set_side_streams(False)
            _, rows = timed(lambda: t.step(batch, batch_increment=0), 2, 1, world)
            t.set_side_streams(True)
            result["kernel_rows_from"] = "2 eager single-stream steps after the timed region (events cannot bracket kernels of a replayed graph)"
        imgs = bs * world * args.steps
        result.update({"metric": "train img/s (128x128, full FFWM GAN step)", "value": round(imgs / dt, 2),
                       "unit": "img/s", "ms_per_step": round(dt / args.steps * 1e3, 3),
                       "config": {"workload": "BASELINE configs[2]: full FFWM train step (netG+netD+flowNetF+flowNetB, "
                                              "all losses, 3x Adam), synthetic MultiPIE-shaped 128x128",
                                  "batch_per_gpu": bs, "global_batch": bs * world,
                                  "parallelism": "dp%d" % world,
                                  "launch": ("hipGraph replay"
                                             + ({"ingraph": " (ONE graph, the bucket all-reduces captured inside it on RCCL's stream, overlapping backward)",
                                                 "segments": " (five graphs: backward_G cut at network boundaries, each finished network's all-reduce "
                                                             "overlaps the next segment; experimental)",
                                                 "serial": " (three graphs, the two gradient all-reduces between them)"}.get(capture_mode, ""))
                                             + (", flowNetB and the loss networks' side passes on their own HIP streams" if t.flow_stream is not None else "")
                                             + (", the D step beside them" if d_side else "")
                                             + (" (%d side streams)" % len({id(x) for x in [t.flow_stream, t.d_stream if d_side else None] + list(t.loss_streams or []) if x is not None}) if t.flow_stream is not None else ""))
                                  if graphed else "eager (hook-launched all-reduces overlap backward)" if world > 1 else "eager",
                                  "dp_capture_mode": capture_mode if graphed and world > 1 else None,
                                  "dp_rank_spread_after_2_replays": dp_spread,
                                  "miopen": "immediate mode%s" % (" + in-tree find-db (ffwm_amd/miopen_db)" if miopen_db else ", heuristic solver choice"),
                                  "conv_wgrad": ("MFMA kernel for %d netG layers" % getattr(t, "mfma_wgrad_layers", 0))
                                  if args.mfma_wgrad == "on" else "vendor library",
                                  "conv_fwd_dgrad": "fp32 Winograd F(2x2,3x3) on MFMA (csrc/conv_winograd.hip) for the 3x3/stride-1 calls of %d layers "
                                                    "with >= %d tiles; direct MFMA kernel (csrc/conv_fwd.hip) forward for %d stride-2 / transposed / "
                                                    "small-plane layers; vendor library for the rest" % (
                                                        getattr(t, "winograd_layers", 0), __import__("ffwm_amd.conv", fromlist=["x"]).WINOGRAD_MIN_TILES,
                                                        getattr(t, "mfma_fwd_layers", 0)),
                                  "titers_branch": "<20000" if args.titers < 20000 else ">=20000",
                                  "weights": "seeded random init (no pretrained VGG19/LightCNN/FlowNet offline)",
                                  "flow_nets": ("fitted to the identity grid for 80 untimed steps (stand-in for the reference's "
                                                "pretrained flowNetF/B checkpoints), final L1 %s" % [round(v, 3) for v in flow_fit])
                                  if flow_fit else "randomly initialised"},
                       "img_per_s_per_gpu": round(imgs / dt / world, 2),
                       "losses": {k: round(v, 5) for k, v in t.loss_values().items()}})
        if step_flops is not None:
            own = step_flops["total"] / bs
            result.update({"conv_GFLOP_per_img": {"this_step": round(own / 1e9, 1), "fwd": round(step_flops["fwd"] / bs / 1e9, 1),
                                                  "bwd": round(step_flops["bwd"] / bs / 1e9, 1),
                                                  "reference_step_estimate": REF_TRAIN_FLOP_PER_IMG / 1e9,
                                                  "note": "counted over every conv / linear call of one step (ffwm_amd/flops.py); "
                                                          "lower than the reference's estimate because frozen LightCNN / VGG19 get no "
                                                          "weight gradients, target-side extractors run under no_grad and the LightCNN "
                                                          "passes are deduplicated (result-preserving)"},
                           "fp32_flop_frac": round(imgs / dt / world * own / FP32_PEAK, 4),
                           "fp32_ceiling_img_per_s_per_gpu": round(FP32_PEAK / own, 1)})
        if world > 1 and args.full:
            # what the collectives cost when nothing overlaps them (outside the timed region, device idle): every bucket of the
            # G-step set on its own, and a message-size sweep that shows where the ring saturates the xGMI links
            try:
                rccl = dist.get_backend() == "nccl"          # (the gloo launch-path test shares one GPU: one repetition, no sweep)
                result["allreduce"] = {"backend": "nccl (= RCCL)" if rccl else dist.get_backend(),
                                       "G_buckets": t.red_G.time_buckets(3 if rccl else 1), "D_buckets": t.red_D.time_buckets(3 if rccl else 1),
                                       "sweep": allreduce_sweep(dev, world) if rccl else None}
                tot = sum(b["ms"] for b in result["allreduce"]["G_buckets"] + result["allreduce"]["D_buckets"])
                result["allreduce"]["sum_ms_per_step_if_not_overlapped"] = round(tot, 3)
            except Exception as e:
                result["allreduce"] = {"error": repr(e)}
            t.red_G.zero_grad()
            t.red_D.zero_grad()
        result["config"]["grad_bytes_per_step"] = t.red_G.grad_bytes() + t.red_D.grad_bytes()
        result["config"]["grad_buckets"] = len(t.red_G.buckets) + len(t.red_D.buckets)
        result["config"]["bucket_MiB"] = args.bucket_mb
    elif args.workload == "flownet":
        bs = args.batch or 6
        r, dt, rows, last = run_flownet(dev, bs, args.steps, args.warmup, world, args.flownet_path, seed=1 + rank)
        outputs = {"flow%d" % i: f for i, f in enumerate(last["flows"])}
        result.update({"metric": "FlowNetF forward img/s (128x128)", "value": r["img_per_s"], "unit": "img/s",
                       "ms_per_step": round(dt / args.steps * 1e3, 4),
                       "config": {"workload": "BASELINE configs[1]: FlowNetF forward-only, bs=%d" % bs, "path": args.flownet_path,
                                  "batch_per_gpu": bs, "parallelism": "dp%d" % world},
                       "conv_GFLOP_per_img": r["conv_GFLOP_per_img"], "fp32_flop_frac": r["fp32_flop_frac"]})
    elif args.workload == "flowtrain":
        # FlowNet pre-training step (train_flow.py / models/flownet_model.py:57-78): the only trainer of the
        # reference that runs the custom ops; README.md:105,116 trains it with batch 6
        from ffwm_amd import trainer
        bs = args.batch or 6
        graphed = args.graph != "off"
        ft = trainer.FlowNetTrainer(dev, world_size=world, seed=0, bucket_bytes=args.bucket_mb << 20, capturable=graphed)
        batch = trainer.synthetic_batch(bs, dev, seed=1 + rank)
        if graphed:
            ok = 1
            try:
                ft.capture(batch)
            except Exception as e:       # e.g. a capture beside a live process group: every rank falls back to the eager step
                ok = 0
                sys.stderr.write("flowtrain: capture failed (%r), eager step\n" % (e,))
            if world > 1:
                flag = torch.tensor([ok], device=dev)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                ok = int(flag.item())
            if not ok:
                graphed = False
                ft = trainer.FlowNetTrainer(dev, world_size=world, seed=0, bucket_bytes=args.bucket_mb << 20)
        dt, rows = timed(lambda: ft.step(batch), args.steps, args.warmup, world)
        if args.dump_outputs:
            outputs = {"loss_" + k: float(v.detach()) for k, v in ft.losses.items()}
            outputs["flowNet_params"] = net_parameters(ft.flowNet)
        imgs = bs * world * args.steps
        result.update({"metric": "FlowNet pre-training img/s (128x128)", "value": round(imgs / dt, 2), "unit": "img/s",
                       "ms_per_step": round(dt / args.steps * 1e3, 3),
                       "config": {"workload": "FlowNetModel train step (correctness + affine regularisation + landmark "
                                              "losses, Adam), synthetic 128x128", "batch_per_gpu": bs,
                                  "parallelism": "dp%d" % world, "weights": "seeded random init",
                                  "launch": "hipGraph replay" if graphed else "eager", "routed_layers": ft.routed_layers},
                       "losses": {k: round(v, 5) for k, v in ft.loss_values().items()}})
    elif args.workload == "warpatt":
        bs = args.batch or 8
        r, dt, rows, outputs = run_warp_attention(dev, bs, args.steps, args.warmup, world, seed=1 + rank, graph=args.graph == "on",
                                                  route=os.environ.get("FFWM_WARPATT_ROUTE", "1") != "0", kernel_rows_after=args.full,
                                                  keep=bool(args.dump_outputs))
        result.update({"metric": "warp+attention path img/s (3 netG levels, fwd+bwd)", "value": r["fwd_bwd_img_per_s"], "unit": "img/s",
                       "ms_per_step": r["fwd_bwd_ms"],
                       "config": {"workload": "netG warp-attention module (base_networks.py:323-333), 3 levels, fwd+bwd", "batch_per_gpu": bs,
                                  "parallelism": "dp%d" % world}, "warp_attention_path": r})
    elif args.workload == "warp":
        # the warp + flip + cat kernels of netG's warp-attention alone, forward + backward, bs images
        from ffwm_amd.external_function import WarpFlipCat
        bs = args.batch or 8
        g = torch.Generator().manual_seed(1 + rank)
        feats = [torch.rand(bs, c, s, s, generator=g).to(dev).requires_grad_(True) for c, s in ((128, 32), (64, 64), (64, 128))]
        flows = [smooth_flow(bs, s).to(dev).requires_grad_(True) for s in (32, 64, 128)]
        gos = [torch.rand(bs, 2 * c, s, s, generator=g).to(dev) for c, s in ((128, 32), (64, 64), (64, 128))]
        mod = WarpFlipCat()
        keep = [None] * len(feats) if args.dump_outputs else None

        def step():
            for i, (f, fl, go) in enumerate(zip(feats, flows, gos)):
                f.grad = fl.grad = None
                y = mod(f, fl)
                y.backward(go)
                if keep is not None:
                    keep[i] = y
        dt, rows = timed(step, args.steps, args.warmup, world)
        if keep is not None:
            outputs = {}
            for i, (y, f, fl) in enumerate(zip(keep, feats, flows)):
                outputs.update({"out%d" % i: y, "grad_feat%d" % i: f.grad, "grad_flow%d" % i: fl.grad})
        imgs = bs * world * args.steps
        result.update({"metric": "warp+flip+cat kernels img/s (3 netG levels, fwd+bwd)", "value": round(imgs / dt, 2),
                       "unit": "img/s", "ms_per_step": round(dt / args.steps * 1e3, 3),
                       "config": {"workload": "netG warp-attention warp kernels (warp + flip + cat), 3 levels, fwd+bwd, smooth flows", "batch_per_gpu": bs,
                                  "parallelism": "dp%d" % world}})
    else:   # ops: cfg-5 per GPU block_extractor forward + backward
        from ffwm_amd import ops
        g = torch.Generator().manual_seed(1 + rank)
        bs = args.batch or 4
        src = torch.rand(bs, 128, 256, 256, generator=g).to(dev)
        flow = (torch.rand(bs, 2, 256, 256, generator=g) * 4 - 2).to(dev)
        out = torch.empty(bs, 128, 768, 768, device=dev)
        gs, gf = torch.zeros_like(src), torch.zeros_like(flow)

        def step():
            ops.block_extractor_forward(src, flow, 3, out=out)
            gs.zero_()
            gf.zero_()
            ops.block_extractor_backward(src, flow, out, 3, gs, gf)
        dt, rows = timed(step, args.steps, args.warmup, world)
        outputs = {"out": out, "grad_src": gs, "grad_flow": gf}
        imgs = bs * world * args.steps
        result.update({"metric": "block_extractor fwd+bwd img/s (256x256, C=128, k=3)", "value": round(imgs / dt, 2),
                       "unit": "img/s", "ms_per_step": round(dt / args.steps * 1e3, 3),
                       "config": {"workload": "BASELINE configs[4] per GPU: block_extractor fwd+bwd", "batch_per_gpu": bs,
                                  "parallelism": "dp%d" % world}})

    # ---- the other scopes of SURVEY 8(d), N = 1 only (they do not take part in the scaling curve)
    if args.dump_outputs and outputs is not None:
        torch.cuda.synchronize()
        dump_outputs(args.dump_outputs if world == 1 else os.path.join(args.dump_outputs, "rank%d" % rank), outputs)

    if args.workload == "train" and world == 1 and args.full and not args.no_extras:
        from ffwm_amd import trainer
        bs = args.batch or 8
        try:
            r, _, _, _ = run_warp_attention(dev, bs, 20, 5, world)
            extras["warp_attention_path"] = r
        except Exception as e:
            extras["warp_attention_path"] = {"error": repr(e)}
        for path in ("lean", "module"):
            try:
                r, _, _, _ = run_flownet(dev, 6, 30, 10, world, path)
                extras["flownet_fwd_cfg2" if path == "lean" else "flownet_fwd_cfg2_module_path"] = r
            except Exception as e:
                extras["flownet_fwd_cfg2" if path == "lean" else "flownet_fwd_cfg2_module_path"] = {"error": repr(e)}
        try:
            # the other titers branch on the SAME trainer (ffwm_model.py:97-105: >= 20000 adds the guided filters on the
            # 64 / 32 px outputs and the two-sided identity loss)
            keep = t.titers
            t.titers = 20000 if keep < 20000 else 0
            dt2, _ = timed(lambda: t.step(batch, batch_increment=0), 5, 3, world)
            extras["train_titers_ge_20000" if keep < 20000 else "train_titers_lt_20000"] = {
                "img_per_s": round(bs * 5 / dt2, 2), "ms_per_step": round(dt2 / 5 * 1e3, 3), "steps": 5, "warmup": 3,
                "launch": "eager (compare with --graph off: the default line replays a captured step)"}
            t.titers = keep
        except Exception as e:
            extras["train_titers_other_branch"] = {"error": repr(e)}
        try:
            other = "random" if args.flow_init == "fit-identity" else "fit-identity"
            t2 = trainer.FFWMTrainer(dev, world_size=1, seed=0, titers=args.titers, bucket_bytes=args.bucket_mb << 20,
                                     mfma_wgrad=args.mfma_wgrad == "on")
            if other == "fit-identity":
                t2.pretrain_flow_identity(batch)
            dt3, _ = timed(lambda: t2.step(batch, batch_increment=0), 5, 3, world)
            extras["train_flow_init_" + other.replace("-", "_")] = {
                "img_per_s": round(bs * 5 / dt3, 2), "ms_per_step": round(dt3 / 5 * 1e3, 3), "steps": 5, "warmup": 3,
                "launch": "eager (compare with --graph off)",
                "note": "an untrained FlowNet outputs tanh(~0): every pixel samples the image centre (all lanes on one cache "
                        "line, all scatter-adds on four cells) -- an access pattern real training never produces"
                        if other == "random" else ""}
            del t2
        except Exception as e:
            extras["train_flow_init_other"] = {"error": repr(e)}
        result["subpaths"] = extras

    if rank == 0:
        inrun = kernel_rows(rows, "timed region")
        traffic = pmc_traffic() if args.workload == "train" else {}      # measured on the default train workload

        def roofline_row(top, bound):
            pmc = traffic.get(top["kernel"]) or top.get("_pmc")
            base = {"bound": bound, "kernel": top["kernel"], "avg_us": top["avg_us"], "launches": top["launches"],
                    "traffic": pmc["traffic_bytes"] if pmc else None,
                    "traffic_source": ("profiles/" + os.path.basename(PMC_FILE) + ": rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this "
                                       "command (--kernel-include-regex ffwm), bytes per launch, FETCH_SIZE x2 per the gfx950 calibration")
                    if pmc else None}
            if bound == "hbm":
                base.update({"achieved": top["GBps"], "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": top["frac_hbm_peak"],
                             "alg_MB_per_launch": top["alg_MB"],
                             "note": ("SURVEY 8 a1-a6 kernel moving the most algorithmic bytes per step" if is_hot_path(top)
                                      else "streaming kernel outside SURVEY 8 a1-a6 moving the most algorithmic bytes per step")
                                     + "; HIP events on its launch stream"})
            else:
                base.update({"achieved": top["TFLOPs"], "peak": FP32_PEAK / 1e12, "unit": "TFLOP/s", "frac": top["frac_mfma_fp32_peak"],
                             "alg_GFLOP_per_launch": top["alg_GFLOP"],
                             "frac_binding_roofline": top.get("frac_binding_roofline"),
                             "note": "hand-written fp32-in / fp32-accumulate MFMA kernel (v_mfma_f32_32x32x2_f32); flops and duration "
                                     "averaged over the layer shapes of the step"})
            return base
        hot = [r for r in inrun if is_hot_path(r) and "TFLOPs" not in r]
        mfma = [r for r in inrun if "TFLOPs" in r]
        other_hbm = [r for r in inrun if not is_hot_path(r) and "TFLOPs" not in r]
        if hot:
            result["roofline"] = roofline_row(max(hot, key=lambda r: r["alg_MB"] * r["launches"]), "hbm")
            result["roofline"].update(hot_rows_summary(inrun))
            result["roofline"].pop("kernels", None)
            if args.full:
                try:
                    # context for a launch of this SIZE: torch's copy_ moving the same number of bytes (half read, half written), timed the
                    # same way on warm caches and after a 1 GiB fill (the cache state an in-step launch finds) -- tools/stream_probe.py
                    nbytes = int(result["roofline"]["alg_MB_per_launch"] * 1e6)
                    src = torch.rand(nbytes // 8, device=dev)
                    dst = torch.empty_like(src)
                    big = torch.empty(256 << 20, device=dev)

                    def copy_us(cold, n=8):
                        dst.copy_(src)
                        torch.cuda.synchronize()
                        tot = 0.0
                        for _ in range(n):
                            if cold:
                                big.fill_(1.0)
                            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            a.record()
                            dst.copy_(src)
                            b.record()
                            torch.cuda.synchronize()
                            tot += a.elapsed_time(b)
                        return tot / n * 1e3
                    warm, cold = copy_us(False), copy_us(True)
                    result["roofline"]["copy_same_bytes_us"] = {"warm": round(warm, 1), "cold": round(cold, 1)}
                    result["roofline"]["copy_same_bytes_frac_cold"] = round(nbytes / (cold * 1e-6) / HBM_PEAK, 4)
                    del src, dst, big
                except Exception as e:
                    result["roofline"]["copy_same_bytes_us"] = {"error": repr(e)}
        elif other_hbm:
            result["roofline"] = roofline_row(max(other_hbm, key=lambda r: r["alg_MB"] * r["launches"]), "hbm")
        else:
            result["roofline"] = None
        if mfma:
            # the forward and the data gradient of the Winograd convolution are ONE kernel under two launch scopes: they compete
            # for "the MFMA kernel with the largest share of the step" together
            wino = [r for r in mfma if r["kernel"] in ("conv_winograd_fwd", "conv_winograd_dgrad")]
            cands = [r for r in mfma if r not in wino]
            if wino:
                tot = sum(r["total_ms"] for r in wino)
                n = sum(r["launches"] for r in wino)
                gflop = sum(r["alg_GFLOP"] * r["launches"] for r in wino)
                tf = gflop / tot                                  # GFLOP / ms = TFLOP/s
                parts = [(traffic[r["kernel"]]["traffic_bytes"], r["launches"]) for r in wino if r["kernel"] in traffic]
                cands.append({"kernel": "conv_winograd (fwd + dgrad)", "where": "timed region", "launches": n, "avg_us": round(tot / n * 1e3, 2),
                              "total_ms": round(tot, 3), "alg_GFLOP": round(gflop / n, 3), "TFLOPs": round(tf, 2),
                              "frac_mfma_fp32_peak": round(tf * 1e12 / FP32_PEAK, 4),
                              "_pmc": {"traffic_bytes": int(sum(b * m for b, m in parts) / sum(m for _, m in parts))} if parts else None})
            ranked = sorted(cands, key=lambda r: -r["total_ms"])
            result["roofline_mfma"] = roofline_row(ranked[0], "mfma")
            if ranked[0]["kernel"].startswith("conv_winograd"):
                result["roofline_mfma"]["note"] = ("hand-written fp32 Winograd F(2x2,3x3) convolution on v_mfma_f32_32x32x2_f32 (forward + data gradient, one "
                                                   "kernel): flops = the multiplications the MFMAs execute (the direct sum it replaces has 2.25 x as many), "
                                                   "averaged over the layer shapes of the step")
            if len(ranked) > 1:
                result["roofline_mfma_2nd"] = roofline_row(ranked[1], "mfma")
        if other_hbm and hot:
            result["roofline_hbm_other"] = roofline_row(max(other_hbm, key=lambda r: r["alg_MB"] * r["launches"]), "hbm")
        result["kernels"] = inrun
        if args.full and not args.no_kernels:
            result["kernels"] = inrun + standalone_kernels()
        for row in result["kernels"]:
            if row["kernel"] in traffic and row["where"] == "timed region":
                row["pmc_traffic_MB"] = round(traffic[row["kernel"]]["traffic_bytes"] / 1e6, 3)
        if world == 1 and args.full and not args.no_cpu_baseline:
            try:
                result.update(cpu_train_baseline(args.titers) if args.workload in ("train",) else cpu_ops_baseline())
            except Exception as e:      # the baseline leg must never take the measurement down
                result["cpu_baseline"] = {"error": repr(e)}
    if args.workload == "train" and world > 1:
        # the first multi-GPU run explains itself: who ran, what each capture mode cost, what the collectives expose
        dp = dp_identity(dev, world)
        serial_ms = result.get("ms_per_step") if rank == 0 else None
        dp["modes"] = {(capture_mode or ("eager" if not graphed else "graph")): {"ms_per_step": serial_ms}}
        dp["rank_spread_after_2_replays"] = dp_spread
        ar = result.get("allreduce") if rank == 0 else None
        if isinstance(ar, dict) and "G_buckets" in ar:
            dp["exposed_allreduce_ms_per_step_unoverlapped"] = ar.get("sum_ms_per_step_if_not_overlapped")
            big = [b for b in ar["G_buckets"] if b["MiB"] >= 0.9 * args.bucket_mb]
            if big:
                dp["bucket_%dMiB_busbw_GBps" % args.bucket_mb] = round(sum(b["busbw_GBps"] for b in big) / len(big), 1)
        result["dp"] = dp
        if graphed and capture_mode == "serial" and not args.no_dp_ingraph and not os.environ.get("FFWM_DP_CAPTURE") \
                and dist.get_backend() == "nccl":
            def fallback(note):
                r = dict(result)
                r["dp"] = dict(dp, ingraph=note)
                return emit_lines(r)
            second, dt2 = dp_time_ingraph(args, dev, world, rank, batch, bs, fallback)
            dp["modes"]["ingraph"] = second
            if second.get("valid") and dt2 is not None and rank == 0 and dt2 < dt:
                # the overlapped mode is the measurement: exactly K timed steps between barriers, like the serial one
                imgs = bs * world * args.steps
                result.update({"value": round(imgs / dt2, 2), "ms_per_step": round(dt2 / args.steps * 1e3, 3),
                               "img_per_s_per_gpu": round(imgs / dt2 / world, 2)})
                result["config"]["dp_capture_mode"] = "ingraph"
                result["config"]["launch"] = ("hipGraph replay (ONE graph, the bucket all-reduces captured inside it on RCCL's stream, overlapping backward; "
                                              "serial mode timed beside it: dp.modes)")
            dp["used"] = result["config"].get("dp_capture_mode") if rank == 0 else None
    if rank == 0:
        for line in emit_lines(result):
            print(line, flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
