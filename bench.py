#!/usr/bin/env python3
"""bench.py -- env-steps/sec of the batched random-action rollout (BASELINE.json metric).

  python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

N > 1 without a launcher: bench.py starts its own N ranks (python -m torch.distributed.run --nnodes=1 --nproc-per-node N
--master-addr 127.0.0.1 ..., steppingstone_amd/launch.py), the way the reference's make_vec_envs forks its own
workers (common/envs_utils.py:519-538); started by torch.distributed.run already, it runs as one rank.

A "step" is one control step of every environment of the job: 4096 Walker3DStepperEnv-v0 environments per GPU
(BASELINE.json configs[1]: flat terrain, curriculum off, random actions drawn on the device, auto-reset on), each
step = 4 physics substeps, contact solve, reward, termination, auto-reset, 60-float observation, all written to HBM.
  N = 1: the K timed steps run through ss_rollout_random's multi-step kernel (up to 1000 control steps
         per launch, state resident in LDS between steps, outputs and the HBM state copy written every step); the
         one-launch-per-step path (what a policy-in-the-loop caller uses) is timed beside it as `per_step_launch` (--full).
  N > 1: every rank owns 4096 envs (weak scaling) and every step's packed [4096,62] obs|rew|done block is all-gathered
         over RCCL (BASELINE configs[3]).  The same multi-step kernel runs here too: 32 control steps per launch, each
         step's block written to its own slot, ONE all-gather per 32-step chunk under the next chunk's kernel (same bytes
         per step on the wire, 32 x fewer collectives) -- so the N = 1 and N > 1 lines time the same kernel and their ratio
         is the cost of the exchange, not of a different launch shape.  Side rows (--full): `no_gather` (same K steps, no
         collective), `per_step_gather` (one launch + one all-gather per step: what a policy-in-the-loop caller pays).
State is resident in HBM before the timed region.  A plain run times exactly K steps in one region (after the clock-ramp launch
and the W warm-up steps) and rank 0 prints ONE JSON line with `value` and `ms_per_step` of that region.  --full adds the repeated
regions (median / min / max), `roofline`, the side rows, the exchange self-check, the Mike / capacity rows and `cpu_baseline` to the
same line.  --dump-outputs DIR writes the last timed step's obs / rew / done (see dump_outputs).
"""
import argparse
import glob
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ENVS_PER_GPU = 4096
ENV_ID = "Walker3DStepperEnv-v0"
# ALGORITHMIC HBM bytes per env-step with this repository's state layout:
#   one launch per step: read 90 f32 state / stone-cache fields + 4 i32 = 376 B; write 60 f32 + 5 i32 state = 260 B,
#                        obs 240 B, rew 4 B, done 1 B, info 24 B = 529 B                                     -> 905 B
#   K steps per launch:  the 376 B are read once per launch, the 529 B written every step; the epilogue's re-read of
#                        the 13 bookkeeping words + stone cache is served by L2                 -> 529 + 376/K B
# (rounds 1-2: 348 + 521 = 869 B, before the second word of the episode return: ss_info.ep_ret_lo; rounds 3-5: 352 + 529 = 881 B,
#  before the six heading words of the three active stones (the plank footprint, PHYSICS.md 3.3): fstate rows 83..88.)
# roofline.achieved is computed from the 905 B per-unit figure for both launch shapes; the smaller figure of
# the K-step kernel and the PMC-measured traffic are reported beside it.
ALGO_READ_B, ALGO_WRITE_B = 376, 529
HBM_PEAK_GBS = 8000.0
VALU_FP32_PEAK_TFLOPS = 157.3          # packed-f32 vector peak (MI355X_MICROARCH.md): 256 CUs x 2.4 GHz x 256 flop/clk


def _natural(path):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", os.path.basename(path))]


def latest_profile(pattern):
    """Newest committed profile matching the glob: round / build numbers compared as NUMBERS (r01_v10 > r01_v9)."""
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)), key=_natural)
    return files[-1] if files else None


def traffic_model(n_envs):
    """HBM bytes per launch of the dominant kernel as a function of the control steps in the launch, from the two latest
    committed PMC runs of that kernel at this batch size (separate FETCH_SIZE / WRITE_SIZE passes, calibrated on a
    dword-per-lane copy: tools/hbm_traffic.py + tools/hbm_traffic_report.py): two launch lengths of the rollout kernel (25 and 250
    steps; before r03_v5: a 1-step launch of the step kernel and a 250-step launch)
    give  bytes(launch of k steps) = const + per_step * k.  The traffic is almost a per-launch constant (state in once,
    dirty lines out once; the per-step rows are overwritten in L2), so a per-env-step figure recorded at one launch length
    must not be scaled linearly to another.  PMC collection needs rocprofv3 around the process, so bench.py reports the
    model and names its sources; (None, None) if a file is missing."""
    fs = latest_profile("*hbm_traffic_rollout_%d.json" % n_envs)
    f1 = latest_profile("*hbm_traffic_rollout25_%d.json" % n_envs)          # a second launch length of the SAME kernel, if recorded
    same_kernel = bool(f1) and bool(fs) and os.path.basename(f1).split("_hbm_")[0] == os.path.basename(fs).split("_hbm_")[0]
    if not same_kernel:
        f1 = latest_profile("*hbm_traffic_%d.json" % n_envs)                # else the 1-step launch of the step kernel
    if not f1 or not fs:
        return None, None
    with open(f1) as fh:
        d1 = json.load(fh)
    with open(fs) as fh:
        ds = json.load(fh)
    s1, ss = float(d1.get("steps_per_launch", 1)), float(ds["steps_per_launch"])
    b1, bs = float(d1["hbm_bytes_per_launch"]), float(ds["hbm_bytes_per_launch"])
    if ss <= s1:
        return None, None
    per_step = (bs - b1) / (ss - s1)
    const = b1 - per_step * s1
    info = {"bytes_per_launch_const": const, "bytes_per_step": per_step,
            "fitted_from": [{"file": os.path.relpath(f1, ROOT), "steps_per_launch": s1, "bytes_per_launch": b1},
                            {"file": os.path.relpath(fs, ROOT), "steps_per_launch": ss, "bytes_per_launch": bs}],
            "note": ("two launch lengths of the rollout kernel" if same_kernel else
                     "1-step launches are the step kernel, S-step launches the rollout kernel (same step_env code, state resident in "
                     "LDS between the steps)")}
    return (lambda k: const + per_step * k), info


def recorded_pmc():
    f = latest_profile("*pmc_4096.json")
    if not f:
        return None, None
    with open(f) as fh:
        return json.load(fh), os.path.relpath(f, ROOT)


def pmc_note(d):
    """The limiter statement of roofline.note, derived from the current PMC file (not hard-coded)."""
    if not d:
        return "per-lane rigid-body dynamics, not HBM-bound (DESIGN.md 5.1); no PMC profile committed"
    w = d.get("per_wave_per_launch", {})
    cyc = w.get("SQ_WAVE_CYCLES") or 0
    if not cyc:
        return "per-lane rigid-body dynamics, not HBM-bound (DESIGN.md 5.1)"
    busy = 100.0 * (w.get("SQ_ACTIVE_INST_VALU") or 0) / cyc
    wait = 100.0 * (w.get("SQ_WAIT_ANY") or 0) / cyc
    return ("not HBM-bound: per-lane rigid-body dynamics limited by VALU issue / dependent-chain latency; averaged over "
            "the %s wavefronts of a launch (main + helper wavefronts) SQ_ACTIVE_INST_VALU = %.0f %% and SQ_WAIT_ANY = "
            "%.0f %% of wave cycles (DESIGN.md 5.1)" % (d.get("waves_per_launch", "?"), busy, wait))


# ------------------------------------------------------------------------------------------------ CPU baseline
def _oracle_fast_lib():
    """the CPU port built -O3 -march=native ON THE BOX THAT RUNS IT (the parity oracle is -O2
    -ffp-contract=off for reproducibility and is not what a CPU user would ship).  Falls back to the parity build."""
    import subprocess
    src = os.path.join(ROOT, "oracle", "ss_oracle.c")
    out = os.path.join(ROOT, "oracle", "lib", "libss_oracle_f32_native.so")
    try:
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["gcc", "-O3", "-march=native", "-fPIC", "-shared", "-std=c11", "-fopenmp", "-DSSO_REAL=float",
                               "-o", out, src, "-lm"], stderr=subprocess.DEVNULL)
        return out, "-O3 -march=native"
    except Exception:
        return None, "-O2 -ffp-contract=off (parity build; native build failed)"


def usable_cpus():
    """CPUs this process may really use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = min(n, max(1, int(float(q) / float(per))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(budget=24.0):
    """The CPU oracle (a port of docs/PHYSICS.md, NOT PyBullet) on the host cores of this box, bounded samples of the
    same workload.  Rows of BASELINE.md section 3: C1 single_thread, C2 all_cores (= the headline value), C3
    shmem_frontend (process-per-env architecture of common/envs_utils.py:486-675), C4 ipc_only (that front end with a
    no-op env)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes
    import numpy as np
    import oracle_lib as ol
    import shmem_frontend as sf
    lib_path, flags = _oracle_fast_lib()
    if lib_path:
        ol.load("f32")                                           # declares the prototypes on the parity build ...
        fast = ctypes.CDLL(lib_path)
        proto = ol._libs["f32"]
        for fn in ("sso_create", "sso_destroy", "sso_reset", "sso_step", "sso_random_actions", "sso_set_auto_reset"):
            getattr(fast, fn).argtypes = getattr(proto, fn).argtypes
            getattr(fast, fn).restype = getattr(proto, fn).restype
        ol._libs["f32_native"] = fast                            # ... and the same ones on the native build

    gomp = ctypes.CDLL("libgomp.so.1")

    def make(n, threads):
        gomp.omp_set_num_threads(int(threads))                   # OMP_NUM_THREADS is read once, at library load
        e = ol.OracleEnv.__new__(ol.OracleEnv)
        e.lib = ol._libs["f32_native"] if lib_path else ol.load("f32")
        e.real, e.kind, e.n = np.float32, ol.KIND["walker3d"], n
        e.h = e.lib.sso_create(e.kind, n, 0, 0)
        return e

    def rate(env, acts, seconds, max_steps):
        env.reset()
        env.step(acts[0])
        t0, steps = time.perf_counter(), 0
        while True:
            env.step(acts[steps % len(acts)])
            steps += 1
            el = time.perf_counter() - t0
            if el > seconds or steps >= max_steps:
                return env.n * steps / el, steps, el

    rng = np.random.default_rng(0)
    # C1: one env, one thread
    e1 = make(1, 1)
    v1, s1, t1 = rate(e1, rng.uniform(-1, 1, (64, 1, 21)).astype(np.float32), 0.15 * budget, 2000)
    e1.close()
    # C2: 4096 envs, OpenMP over the host threads.  os.cpu_count() is not what a container may use (affinity mask,
    # cgroup quota) and oversubscribed OpenMP teams collapse, so the team size is swept and the best one reported.
    usable = usable_cpus()
    cand = sorted({max(1, usable >> k) for k in range(0, 6)} | {min(usable, 64), min(usable, 32)}, reverse=True)
    sweep = {}
    acts4 = None
    for th in cand:
        e = make(ENVS_PER_GPU, th)
        acts4 = acts4 or [e.random_actions(t) for t in range(4)]
        sweep[th] = rate(e, acts4, 0.04 * budget, 6)[0]
        e.close()
    best_th = max(sweep, key=sweep.get)
    eN = make(ENVS_PER_GPU, best_th)
    vN, sN, tN = rate(eN, acts4, 0.3 * budget, 400)
    eN.close()
    cores = best_th
    out = {"value": vN, "unit": "env-steps/s", "cores": cores, "kind": "port",
           "sample": "%d control steps of %d Walker3D envs, oracle/ss_oracle.c fp32 built %s on this box, OpenMP over %d "
                     "host threads, %.1f s" % (sN, ENVS_PER_GPU, flags, cores, tN),
           "all_cores": {"value": vN, "cores": cores, "envs": ENVS_PER_GPU, "steps": sN, "seconds": tN,
                         "os_cpu_count": os.cpu_count(), "usable_cpus": usable,
                         "thread_sweep": {str(k): round(v) for k, v in sorted(sweep.items())}},
           "single_thread": {"value": v1, "cores": 1, "envs": 1, "steps": s1, "seconds": t1,
                             "ms_per_env_step": 1e3 / v1}}
    # C3 / C4: process-per-env shared-memory front end, P = min(cores, 64) workers
    workers = max(2, min(usable, 64))
    try:
        if lib_path:
            os.environ["SS_ORACLE_LIB_F32"] = lib_path            # the workers (spawned processes) load the same native build as C2
        v3, s3, t3 = sf.measure("walker3d", workers, seconds=0.2 * budget)
        out["shmem_frontend"] = {"value": v3, "cores": workers, "envs": workers, "steps": s3, "seconds": t3,
                                 "note": "one worker process per env, pipe + shared-memory obs (architecture of "
                                         "common/envs_utils.py:486-675) around the same oracle build as all_cores (%s)" % flags}
        v4, s4, t4 = sf.measure("noop", workers, seconds=0.1 * budget)
        out["ipc_only"] = {"value": v4, "cores": workers, "envs": workers, "steps": s4, "seconds": t4,
                           "note": "same front end, no-op env: ceiling of the process-per-env architecture on this host"}
    except Exception as exc:                                     # a baseline row must never fail the bench
        out["shmem_frontend"] = {"value": None, "error": repr(exc)[:200]}
    finally:
        os.environ.pop("SS_ORACLE_LIB_F32", None)
    return out


# ------------------------------------------------------------------------------------------------ the bench
DUMP_MAX_BYTES = 64 << 20


def dump_outputs(outdir, last):
    """--dump-outputs: what the timed path returned for its last step -- (obs [N,60], rew [N], done [N]) of every env of the job
    -- as DIR/obs.npy, DIR/rew.npy, DIR/done.npy in float32 (done as 0 / 1).  Above DUMP_MAX_BYTES in all, a fixed sample of
    env rows (numpy default_rng(0), sorted) is written instead, and its row indices as DIR/sample_rows.npy (float64)."""
    import numpy as np
    arrays = {name: t.detach().float().cpu().numpy() for name, t in zip(("obs", "rew", "done"), last)}
    n = arrays["obs"].shape[0]
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_MAX_BYTES:
        keep = int(n * DUMP_MAX_BYTES // (total + 8 * n))
        rows = np.sort(np.random.default_rng(0).choice(n, keep, replace=False))
        arrays = {name: a[rows] for name, a in arrays.items()}
        arrays["sample_rows"] = rows.astype(np.float64)
    os.makedirs(outdir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(outdir, name + ".npy"), np.ascontiguousarray(a))


def launch_shape(W, K, spl, ms_per_step, prewarm=0):
    """The launches of the dominant kernel in this run (warm-up and timed) and the per-launch average a `rocprofv3 --stats`
    summary of the same command shows for it: the warm-up launch is shorter than the timed ones, so that average is not
    `kernel_ms` (profiles/*_rocprofv3_rollout_dispatches.csv lists the dispatches one by one)."""
    def sizes(n):
        out = []
        while n > 0:
            out.append(min(spl, n))
            n -= out[-1]
        return out
    warm, timed = sizes(W), sizes(K)
    every = ([prewarm] if spl > 1 and prewarm else []) + warm + timed     # the clock-ramp launch runs the same kernel
    def rle(xs):           # run-length form [[steps per launch, launches], ...]: the driver's shape repeats its 20-step launch thousands of times
        out = []
        for x in xs:
            if out and out[-1][0] == x:
                out[-1][1] += 1
            else:
                out.append([x, 1])
        return out
    return {"launch_steps": {"prewarm": prewarm, "warmup": warm, "timed_steps_x_launches": rle(timed)},
            "rocprofv3_stats_average_ms_expected": ms_per_step * sum(every) / max(len(every), 1)}


PHASE = {"name": "start"}          # what the rank is doing, for the watchdog's error line


def start_watchdog(args, rank, world):
    """A multi-GPU run that hangs (a rank that died, a collective that never completes, an xGMI link down) must say so: after
    --watchdog seconds every rank still running prints ONE JSON line {"error": ..., "phase": ..., "rank": ...} and leaves with exit
    code 3, so the driver's SCALE file holds a reason instead of a timeout."""
    import threading
    limit = args.watchdog if args.watchdog >= 0 else (900.0 if (world > 1 or args.gpus > 1) else 0.0)
    if limit <= 0:
        return None

    def fire():
        line = json.dumps({"error": "watchdog: rank %d of %d still in phase '%s' after %.0f s -- a rank died or a collective hangs"
                                    % (rank, world, PHASE["name"], limit), "rank": rank, "world_size": world, "phase": PHASE["name"],
                           "metric": "env-steps/sec (batched random-action rollout)", "value": None, "n_gpus": world})
        sys.stdout.write(line + "\n")
        sys.stdout.flush()
        os._exit(3)

    t = threading.Timer(limit, fire)
    t.daemon = True
    t.start()
    return t


def device_identity(torch, dist, dev, use_dist, world):
    """PCI bus id and name of every rank's GPU (all-gathered): the line itself shows that N ranks sat on N different devices."""
    p = torch.cuda.get_device_properties(dev)
    mine = "%s %s" % (getattr(p, "pci_bus_id", "?") if not hasattr(p, "pci_domain_id") else
                      "%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id), p.name)
    if not use_dist:
        return [mine]
    out = [None] * world
    dist.all_gather_object(out, mine)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--envs-per-gpu", type=int, default=ENVS_PER_GPU)
    ap.add_argument("--env", default=ENV_ID)
    ap.add_argument("--curriculum", type=int, default=0)
    ap.add_argument("--steps-per-launch", type=int, default=0, help="N=1: control steps per kernel launch (0 = min(K, 1000); 1 = one launch per step)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: repeated timed regions (median / min / max), the roofline, the side rows, the exchange "
                         "self-check, the Mike / capacity rows and the CPU baseline (a plain run does only the headline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the obs / rew / done of their last step as DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="--full: skip the Mike / capacity side measurements")
    ap.add_argument("--no-gather", action="store_true", help="N>1: time only the collective-free rollout")
    ap.add_argument("--per-step-exchange", action="store_true",
                    help="N>1: headline = one launch + one all-gather per step instead of 32-step chunks")
    ap.add_argument("--peer-store", action="store_true",
                    help="N>1: also time the peer-store exchange (steppingstone_amd/peer.py; validated on one GPU only so far)")
    ap.add_argument("--ppo", action="store_true",
                    help="BASELINE configs[4] instead of the rollout metric: PPO end to end (MikeStepperEnv-v0, curriculum on, 4096 "
                         "envs per GPU, 32-step rollouts, actor/critic on PyTorch-ROCm), frames/s; --updates U")
    ap.add_argument("--ppo-rows", default="torch,torch_scaled", help="--ppo: which minibatch rows to run (row A 'torch' is the value)")
    ap.add_argument("--updates", type=int, default=10, help="--ppo: number of PPO updates (<= 10 keeps the run under two minutes)")
    ap.add_argument("--dry-launch", action="store_true", help="start the N ranks, report RANK / WORLD_SIZE, exit (no GPU needed)")
    ap.add_argument("--watchdog", type=float, default=-1.0,
                    help="seconds after which a rank that has not finished prints a JSON error line and exits with code 3 instead of "
                         "hanging in a collective (default: 900 at N > 1, off at N = 1; 0 = off)")
    args = ap.parse_args()

    # more hardware queues than HIP's default 4, so that RCCL's stream never shares one with the launch stream
    # (steppingstone_amd/distributed.py); must be set before the HIP runtime starts
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    from steppingstone_amd import launch
    rc = launch.ensure_ranks(args.gpus, [os.path.abspath(__file__)] + sys.argv[1:])
    if rc is not None:
        raise SystemExit(rc)
    rank, local_rank, world = launch.rank_info()
    watchdog = start_watchdog(args, rank, world)
    if args.dry_launch:
        # one write per line: the ranks share the launcher's stdout, and print() sends the text and the newline separately
        sys.stdout.write(json.dumps({"dry_launch": True, "rank": rank, "local_rank": local_rank, "world_size": world,
                                     "master": "%s:%s" % (os.environ.get("MASTER_ADDR"), os.environ.get("MASTER_PORT"))}) + "\n")
        sys.stdout.flush()
        return

    import torch
    import torch.distributed as dist
    from steppingstone_amd.distributed import ShardedVecEnv
    from steppingstone_amd.envs import SteppingStoneVecEnv

    # Test hook (tests/test_gpu_two_ranks.py): SS_BENCH_TEST_TRANSPORT=gloo runs every rank on cuda:0 with gloo as the transport, so
    # that the N > 1 code path executes end to end on a one-GPU box.  The line it prints says so and is never a measurement.
    test_transport = os.environ.get("SS_BENCH_TEST_TRANSPORT", "")
    if test_transport:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    force = os.environ.get("SS_FORCE_COLLECTIVE") == "1"      # world 1 under torchrun: still go through RCCL
    use_dist = world > 1 or (force and launch.launched())
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if test_transport:
            dist.init_process_group(test_transport)
        else:
            dist.init_process_group("nccl", device_id=dev)

    PHASE["name"] = "process group up"
    n_local = args.envs_per_gpu
    if args.ppo:
        ppo_e2e(args, torch, dist, dev, rank, world, use_dist, n_local)
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        return
    local = SteppingStoneVecEnv(args.env, n_local, seed=0, device=dev, env_id_offset=rank * n_local, return_numpy=False)
    if args.curriculum:
        local.update_curriculum(args.curriculum)
    env = ShardedVecEnv(local)
    env.reset()
    gather = use_dist and not args.no_gather
    spl = args.steps_per_launch if args.steps_per_launch > 0 else min(args.steps, 1000)
    multi_step = not use_dist and spl > 1

    def sync():
        torch.cuda.synchronize(dev)
        if use_dist:
            dist.barrier()
            torch.cuda.synchronize(dev)

    def timed(fn, events=True):
        """wall clock (barrier + synchronize on both sides) and, if `events`, the HIP-event time on the launch stream of fn()"""
        if not events:
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            return time.perf_counter() - t0, None
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record(); ev1.record()          # torch creates the HIP events lazily at the first record(): not inside the timed region
        sync()
        t0 = time.perf_counter()
        ev0.record()
        fn()
        ev1.record()
        sync()
        return time.perf_counter() - t0, ev0.elapsed_time(ev1)

    K, W = args.steps, args.warmup
    chunked = use_dist and not args.per_step_exchange
    if multi_step:
        run = lambda k, t0: local.rollout_random(k, t0=t0, steps_per_launch=spl)            # noqa: E731
    elif chunked:
        run = lambda k, t0: env.rollout_random_chunked(k, t0=t0, gather=gather)             # noqa: E731
    else:
        run = lambda k, t0: env.rollout_random(k, t0=t0, gather=gather)                     # noqa: E731
    # Clock ramp, before and apart from the W warm-up steps: the GPU leaves its idle power state only after some tens of
    # milliseconds of load, and a short run (the driver has used --steps 20 --warmup 5) would otherwise time the ramp: 72.8 instead
    # of 82 M env-steps/s.  Collective-free steps on the local shard (the envs simply are 256 steps further along).
    PREWARM = 256
    PHASE["name"] = "clock-ramp launch + first barrier"
    local.rollout_random(PREWARM, t0=1 << 20, steps_per_launch=PREWARM)
    sync()
    PHASE["name"] = "warm-up / timed rollout (kernels + %s)" % ("RCCL all-gather" if gather else "no exchange")

    def reduce_max(x):
        if not use_dist:
            return x
        v = torch.tensor([x], dtype=torch.float64, device=dev)
        dist.all_reduce(v, op=dist.ReduceOp.MAX)
        return float(v.item())

    if W:
        run(W, 0)
    # The headline: ONE timed region of EXACTLY K steps between barrier + synchronize on both sides, max over ranks, no
    # instrumentation inside it.  `value` and `ms_per_step` come from this region alone.
    t_next = W
    last = []
    el, _ = timed(lambda: last.append(run(K, t_next)), events=False)
    elapsed = reduce_max(el)
    t_next += K
    if args.dump_outputs:
        PHASE["name"] = "dump outputs"
        if rank == 0:
            dump_outputs(args.dump_outputs, last[-1])
    out = None
    if rank == 0:
        total_envs = n_local * world
        value = total_envs * K / elapsed
        steps_in_launch = spl if multi_step else (32 if chunked else 1)
        out = {
            "metric": "env-steps/sec (batched random-action rollout)",
            "value": value, "unit": "env-steps/s", "n_gpus": world, "steps": K, "warmup": W,
            "ms_per_step": 1e3 * elapsed / K,
            "region_is": "one region of exactly %d steps between barrier + synchronize on both sides (max over ranks); value and "
                         "ms_per_step are that region's" % K,
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "%s, %d envs per MI355X, curriculum %d%s, on-device Philox U(-1,1) actions, auto-reset on"
                                   % (args.env, n_local, args.curriculum, " (flat terrain)" if not args.curriculum else ""),
                       "envs_total": total_envs,
                       "parallelism": "env-shard x%d%s" % (world, "+allgather" if gather else ""),
                       "ranks": world, "collective": ((("%s all_gather_into_tensor of [32,%%d,62] f32 per 32-step chunk, %%d ranks"
                                                        if chunked else "%s all_gather_into_tensor of [%%d,62] f32 per step, %%d ranks")
                                                       % (test_transport or "RCCL")) % (n_local, world)) if gather else None,
                       "value_is": ("K-step launches of the rollout kernel (state resident in LDS between steps)" if multi_step else
                                    "32-step launches + one all-gather per 32-step chunk" if (chunked and gather) else
                                    "one launch%s per control step" % (" + one all-gather" if gather else "")),
                       "steps_per_launch": steps_in_launch, "prewarm_steps": PREWARM,
                       **({"test_transport": "%s, all ranks on ONE GPU: a functional run of the N > 1 path, not a measurement" % test_transport}
                          if test_transport else {})},
        }
    if not args.full:
        if rank == 0:
            sys.stdout.write(json.dumps(out) + "\n")          # one write: nothing can land inside the line
            sys.stdout.flush()
        PHASE["name"] = "final barrier"
        if use_dist:
            dist.barrier()
            dist.destroy_process_group()
        if watchdog is not None:
            watchdog.cancel()
        return

    # --full: everything beside the headline.  The headline region is repeated -- every repeat is again exactly K steps,
    # continuing the rollout -- and the median / min / max over all regions (the headline region included) are reported beside
    # `value`: at least 9 regions AND until the regions add up to MIN_TIMED_S = 5 s of timed work (at most MAX_REPEATS); a long
    # region (>= 50 ms) needs no minimum count of repeats.  `repeats` and `timed_region_s` say what was done.  The stop rule uses
    # the max-over-ranks times, so every rank runs the same number of regions.
    REPEAT_BELOW_S, MIN_REPEATS, MIN_TIMED_S, MAX_REPEATS = 0.05, 9, 5.0, 20000
    if test_transport:
        MIN_TIMED_S = 0.2          # a functional run of the N > 1 path (all ranks on one GPU): never a measurement
    PHASE["name"] = "repeated timed regions"
    samples = [(elapsed, None)]
    # The two HIP events that measure the kernel time for the roofline are instrumentation INSIDE the timed region (two marker packets
    # on the launch stream, ~9 us of a 20-step region's ~950): they are recorded in every EVENTS_EVERY-th repeat only (never in the
    # headline region); `roofline.kernel_ms` is the median over the instrumented regions.
    EVENTS_EVERY = 4
    for rep in range(1, MAX_REPEATS):
        el, ev = timed(lambda: run(K, t_next), events=(rep % EVENTS_EVERY == 1))
        t_next += K
        samples.append((reduce_max(el), ev))
        if (rep + 1 >= MIN_REPEATS or samples[0][0] >= REPEAT_BELOW_S) and sum(s_[0] for s_ in samples) >= MIN_TIMED_S:
            break
    timed_region_s = sum(s_[0] for s_ in samples)
    order = sorted(range(len(samples)), key=lambda i: samples[i][0])
    elapsed_median = samples[order[len(order) // 2]][0]
    evs = sorted(s_[1] for s_ in samples if s_[1] is not None)
    main_ev_ms = evs[len(evs) // 2]
    elapsed_min, elapsed_max = samples[order[0]][0], samples[order[-1]][0]
    devices = device_identity(torch, dist, dev, use_dist, world)
    # self-proof of the exchange, straight after the timed regions: every rank checksums its own block and each peer's block
    # as received, the checksums are compared across ranks (ShardedVecEnv.verify_last_exchange)
    PHASE["name"] = "exchange verification / side rows"
    gather_verified = None
    if use_dist and gather:
        try:
            gather_verified, _ = env.verify_last_exchange()
        except Exception as exc:
            gather_verified = "error: " + repr(exc)[:200]
    # the other launch granularity / the collective-free pass, on the same K steps (not the headline value)
    side = {}
    if multi_step:
        el1, ev1 = timed(lambda: local.rollout_random(K, t0=t_next, steps_per_launch=1))
        side["per_step_launch"] = {"ms_per_step": 1e3 * el1 / K, "value": n_local * K / el1, "kernel_ms": ev1 / K,
                                   "note": "same K steps, one kernel launch per control step (the path a policy-in-the-"
                                           "loop caller and the multi-GPU all-gather use)"}
        kernel_ms_per_step = main_ev_ms / K
    else:
        def side_row(key, fn, note):
            # a side row never takes the headline down with it; every rank runs the same rows in the same order
            nonlocal t_next
            try:
                el, _ = timed(fn)
                side[key] = {"ms_per_step": 1e3 * el / K, "note": note}
            except Exception as exc:
                side[key] = {"ms_per_step": None, "error": repr(exc)[:300]}
            t_next += K

        if use_dist and gather:
            if chunked:
                side_row("no_gather", lambda: env.rollout_random_chunked(K, t0=t_next, gather=False),
                         "same K steps, same 32-step launches, no collective")
                side_row("per_step_gather", lambda: env.rollout_random(K, t0=t_next, gather=True),
                         "one kernel launch and one all-gather of [N/G,62] per control step: SURVEY 8d-4's exchange as a "
                         "policy-in-the-loop caller pays it (playground/train.py:373 consumes every step)")
            else:
                side_row("no_gather", lambda: env.rollout_random(K, t0=t_next, gather=False),
                         "same K steps without the per-step all-gather")
                side_row("chunked_gather", lambda: env.rollout_random_chunked(K, t0=t_next, gather=True),
                         "32 control steps per launch, one all-gather per chunk")
            if args.peer_store:
                # the same exchange written by the step kernel itself into every peer's gather buffer (no collective in
                # the data path; steppingstone_amd/peer.py).  A side row: a failure here never touches the headline value.
                try:
                    penv = ShardedVecEnv(local, peer_gather=True)
                    penv.rollout_random(2, t0=t_next, gather=True)
                    if penv._peer.error():                      # a flag never arrived: do not spin through K more steps
                        raise RuntimeError("peer flags timed out in the first two steps")
                    penv.rollout_random(min(W, 50) or 8, t0=t_next + 2, gather=True)
                    el3, _ = timed(lambda: penv.rollout_random(K, t0=t_next + 52, gather=True))
                    err = penv._peer.error() if penv._peer is not None else -1
                    side["peer_store"] = {"ms_per_step": 1e3 * el3 / K, "wait_timeouts": err,
                                          "note": "same K steps, packed block stored by the step kernel into every peer's "
                                                  "gather buffer over xGMI + flag words instead of the RCCL all-gather"}
                    penv._peer.close(); penv._peer = None
                except Exception as exc:
                    side["peer_store"] = {"ms_per_step": None, "error": repr(exc)[:300]}
                t_next += K + 52
        kspl = 32 if chunked else 1
        _, ev1 = timed(lambda: local.rollout_random(K, t0=t_next, steps_per_launch=kspl))
        kernel_ms_per_step = ev1 / K                       # back-to-back launches on one stream: sum of durations

    keys = [k for k in ("no_gather", "per_step_gather", "chunked_gather", "peer_store") if side.get(k, {}).get("ms_per_step")]
    if use_dist and keys:
        t = torch.tensor([side[k]["ms_per_step"] for k in keys], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        for i, k in enumerate(keys):
            side[k]["ms_per_step"] = float(t[i].item())
    for k in keys:
        side[k]["value"] = n_local * world / (side[k]["ms_per_step"] * 1e-3)

    if rank == 0:
        # roofline.achieved uses SURVEY 8(d)'s per-unit figure recomputed for this layout (905 B per env-step: the state
        # round trip a step() implies) x the env-steps one launch processes.  The K-step kernel really moves less (the 376 B
        # of state are read once per launch): that figure is reported next to it, as is the PMC-measured traffic.
        #  `achieved` / `frac` are for the launch shape that is TIMED: a K-step launch reads the 376 B of state
        # once per launch, so its own algorithmic need is 529 + 376 / K B per env-step; 905 B (the state round trip every step()
        # implies) applies to one launch per step.  The 905-B figure stays beside it as a first-class field.
        algo_roundtrip = float(ALGO_WRITE_B + ALGO_READ_B)
        algo_per_env_step = ALGO_WRITE_B + ALGO_READ_B / float(steps_in_launch)
        launch_ms = kernel_ms_per_step * steps_in_launch
        algo_per_launch = algo_per_env_step * n_local * steps_in_launch
        achieved = algo_per_launch / (launch_ms * 1e-3) / 1e9
        achieved_roundtrip = algo_roundtrip * n_local * steps_in_launch / (launch_ms * 1e-3) / 1e9
        tag = "rollout_" if (multi_step or chunked) else ""
        tmodel, tinfo = traffic_model(n_local)
        traffic = tmodel(steps_in_launch) if tmodel else None      # per launch of THIS run's launch shape, like `achieved`
        pmc, pmc_src = recorded_pmc()
        helpers = 3 if n_local <= 8192 else (1 if n_local <= 16384 else 0)
        model = "ModelWalker3D" if "Walker3D" in args.env else "ModelMike"
        if multi_step or chunked:
            kernel = ("ss::rollout_kernel_helped<%s,%d>" % (model, helpers)) if helpers else "ss::rollout_kernel<%s>" % model
        else:
            kernel = ("ss::step_kernel_helped<%s,true,%d>" % (model, helpers)) if helpers else "ss::step_kernel<%s,true>" % model
        out.update({
            "repeats": len(samples), "timed_region_s": timed_region_s, "hip_events_in_regions": len(evs),
            "repeats_are": "the headline region and %d more regions of exactly %d steps each, continuing the rollout" % (len(samples) - 1, K),
            "ms_per_step_median": 1e3 * elapsed_median / K,
            "ms_per_step_min": 1e3 * elapsed_min / K, "ms_per_step_max": 1e3 * elapsed_max / K,
            "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_unit": "B/launch",
                         "traffic_model": tinfo,
                         "kernel": kernel, "kernel_ms": launch_ms, "kernel_ms_per_step": kernel_ms_per_step,
                         **launch_shape(W, K * len(samples), steps_in_launch, kernel_ms_per_step, PREWARM if multi_step else 0),
                         "algorithmic_bytes_per_env_step": algo_per_env_step,
                         "algorithmic_bytes_per_launch": algo_per_launch,
                         "algorithmic_bytes_is": ("%d B written + %d B of state read once per %d-step launch" % (ALGO_WRITE_B, ALGO_READ_B, steps_in_launch)),
                         "state_roundtrip_every_step": {"algorithmic_bytes_per_env_step": algo_roundtrip, "achieved": achieved_roundtrip,
                                                        "frac": achieved_roundtrip / HBM_PEAK_GBS,
                                                        "note": "the same kernel time priced at SURVEY 8(d)'s 905 B per env-step (state read AND "
                                                                "written every step): what a one-launch-per-step caller's traffic would be"},
                         "note": pmc_note(pmc), "note_source": pmc_src},
        })
        out.update(side)
        # the figure a policy-in-the-loop caller gets (one launch -- and at N > 1 one all-gather -- per control step), with the
        # same prominence as `value` (the reference's loop consumes every step: playground/train.py:373)
        pil = side.get("per_step_launch") or side.get("per_step_gather") or (
            {"ms_per_step": 1e3 * elapsed / K, "value": value} if not (multi_step or chunked) else None)
        if pil and pil.get("ms_per_step"):
            out["policy_in_the_loop"] = {"value": pil.get("value", total_envs / (pil["ms_per_step"] * 1e-3)), "unit": "env-steps/s",
                                         "ms_per_step": pil["ms_per_step"],
                                         "what": "one kernel launch%s per control step" % (" + one RCCL all-gather of [N/G,62]" if gather else "")}
        out["devices"] = devices
        if use_dist:
            out["gather_verified"] = gather_verified
            out["rccl_ranks"] = dist.get_world_size()
            try:
                out["rccl_version"] = ".".join(str(x) for x in torch.cuda.nccl.version())
            except Exception:
                out["rccl_version"] = None
            out["transport"] = test_transport or "nccl (RCCL)"
            #  the exchange north_star / SURVEY 8d-4 name -- one all-gather of [N/G,62] per control step, the
            # shape every policy-in-the-loop caller runs -- as a FIRST-CLASS value next to `value` (which, chunked, ships the same bytes
            # in 32 x fewer collectives): a 1 -> 8 scaling curve can be drawn of either
            pse = side.get("per_step_gather") if chunked else ({"ms_per_step": 1e3 * elapsed / K, "value": value} if gather else None)
            if pse and pse.get("ms_per_step"):
                out["value_per_step_exchange"] = pse["value"]
                out["ms_per_step_per_step_exchange"] = pse["ms_per_step"]
                out["value_per_step_exchange_is"] = ("whole-job env-steps/s with one kernel launch and one %s all_gather_into_tensor of [%d,62] f32 per "
                                                     "control step, same K steps" % (test_transport or "RCCL", n_local))
            # RCCL's own view of the job: what this process group is made of
            out["rccl"] = {"backend": dist.get_backend(), "ranks": dist.get_world_size(), "version": out["rccl_version"],
                           "devices_per_rank": devices, "env": {k: v for k, v in os.environ.items() if k.startswith(("NCCL_", "RCCL_", "HSA_ENABLE_IPC"))},
                           "peer_access_from_rank0": ([bool(torch.cuda.can_device_access_peer(0, j)) for j in range(1, torch.cuda.device_count())]
                                                      if torch.cuda.device_count() > 1 else [])}
        flop = None
        if pmc and pmc.get("per_wave_per_launch", {}).get("SQ_INSTS_VALU_FLOPS_FP32"):
            # per-wavefront mean x wavefronts per launch (main + helper wavefronts) x 64 lanes, per env-step of the launch
            flop = (float(pmc["per_wave_per_launch"]["SQ_INSTS_VALU_FLOPS_FP32"]) * float(pmc["waves_per_launch"]) * 64.0
                    / float(pmc["envs"]) / float(pmc.get("steps_per_launch", 1)))
            tf = flop * n_local / (kernel_ms_per_step * 1e-3) / 1e12
            out["roofline"]["valu_fp32"] = {"flop_per_env_step": flop, "source": pmc_src, "achieved": tf,
                                            "peak": VALU_FP32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / VALU_FP32_PEAK_TFLOPS,
                                            "note": "secondary roofline: packed-f32 vector peak of the chip; %d envs occupy "
                                                    "%d of its 1024 SIMDs" % (n_local, n_local // 32 * (1 + helpers))}
            # the bound that binds, at the top level of the line beside `roofline.frac` (the HBM fraction is small by construction)
            out["binding_roofline"] = {"bound": "valu_fp32", "frac": tf / VALU_FP32_PEAK_TFLOPS, "achieved": tf, "peak": VALU_FP32_PEAK_TFLOPS,
                                       "unit": "TFLOP/s", "hbm_frac": achieved / HBM_PEAK_GBS}
        if world == 1 and not use_dist and not args.no_extra:
            out["extra"] = extra_rows(torch, SteppingStoneVecEnv, dev, flop)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
        sys.stdout.write(json.dumps(out) + "\n")          # one write: nothing can land inside the line
        sys.stdout.flush()
    PHASE["name"] = "final barrier"
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if watchdog is not None:
        watchdog.cancel()


def ppo_e2e(args, torch, dist, dev, rank, world, use_dist, n_local):
    """BASELINE.json configs[4] as it words it: MikeStepperEnv-v0, curriculum sampler on, 4096 envs per MI355X, the loop of
    playground/train.py:363-521 (32-step rollouts, GAE, 10 PPO epochs of minibatch 1024, exponential lr decay, fixed-order
    curriculum gate) with the actor / critic on PyTorch-ROCm (autograd + torch.optim.Adam, steppingstone_amd.ppo.PPO).
    frames = env-steps collected; the value is
    steady-state frames/s over the updates after the first three (graph capture / allocator warm-up), the whole-run figure
    beside it.  One JSON line from rank 0."""
    from steppingstone_amd import ppo
    from steppingstone_amd.envs import SteppingStoneVecEnv
    U, T, MB = max(5, args.updates), 32, 1024
    # test transport only (tests/test_gpu_configs4.py): fewer PPO epochs per update, stated in the line; a real run is always 10
    EPOCHS = int(os.environ.get("SS_BENCH_TEST_PPO_EPOCHS", "10")) if os.environ.get("SS_BENCH_TEST_TRANSPORT") else 10
    # "minibatch 1024 kept or scaled -- state the choice".  Both, torch learner: row A keeps the reference's minibatch of
    # 1024 (playground/train.py:62; 128 minibatches per epoch of this rank's 131 072-frame rollout), row B keeps the reference's NUMBER
    # of minibatches per epoch instead (train.py:63: 40000 // 1024 = 39; the nearest divisor of the rollout is 32 -> minibatch 4096).
    MB_SCALED = max(MB, (T * n_local) // 32)
    rows = {}
    for key, mb in (("torch", MB), ("torch_scaled", MB_SCALED)):
        if key not in args.ppo_rows.split(","):
            continue
        PHASE["name"] = "ppo row %s (minibatch %d)" % (key, mb)
        envs = SteppingStoneVecEnv("MikeStepperEnv-v0", n_local, seed=8, device=dev, env_id_offset=rank * n_local, return_numpy=False)
        stamps = []

        def log(st):
            torch.cuda.synchronize(dev)
            stamps.append((time.perf_counter(), st["total_num_steps"], st["mean_rew"], st["curriculum"]))
        try:
            torch.cuda.synchronize(dev)
            if use_dist:
                dist.barrier()
            t0 = time.perf_counter()
            ppo.train(envs, U, num_steps=T, ppo_epoch=EPOCHS, mini_batch_size=mb, use_curriculum=True, log=log)
            torch.cuda.synchronize(dev)
            if use_dist:
                dist.barrier()
            t1 = time.perf_counter()
            steady = (stamps[-1][1] - stamps[2][1]) / (stamps[-1][0] - stamps[2][0])
            rows[key] = {"value": steady, "unit": "frames/s", "whole_run_frames_per_s": stamps[-1][1] / (t1 - t0), "mini_batch_size": mb,
                         "minibatches_per_epoch": (T * n_local) // mb,
                         "updates": U, "steady_state_updates": U - 3, "ms_per_update": 1e3 * (stamps[-1][0] - stamps[2][0]) / (U - 3),
                         "mean_episode_return_first_last": [stamps[0][2], stamps[-1][2]], "curriculum_level_end": stamps[-1][3]}
        except Exception as exc:
            rows[key] = {"value": None, "error": repr(exc)[:300]}
        envs.close()
    if rank == 0:
        main = rows["torch"]
        out = {"metric": "frames/sec (PPO end-to-end, BASELINE configs[4])", "value": main.get("value"), "unit": "frames/s",
               "n_gpus": world, "steps": U, "warmup": 3, "ms_per_step": main.get("ms_per_update"), "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
               "config": {"workload": "MikeStepperEnv-v0, %d envs per MI355X, fixed-order curriculum on, PPO: %d-step rollouts, 10 epochs, "
                                      "minibatch %d, actor / critic (SoftsignActor + critic) on PyTorch-ROCm, hipGraph replay of rollout and "
                                      "minibatch step at one rank; at several ranks the rollout is eager and the minibatch step a hipGraph "
                                      "with its RCCL all-reduce captured" % (n_local, T, MB),
                          "envs_total": n_local * world, "learner": "torch", "a_step_is": "one PPO update = %d frames" % (T * n_local * world),
                          "parallelism": "data-parallel x%d" % world},
               "learner_torch": main, "learner_torch_scaled_minibatch": rows.get("torch_scaled"),
               "minibatch_choice": "value = row A: the reference's minibatch 1024 kept (train.py:62); learner_torch_scaled_minibatch = row B: the "
                                   "reference's ~39 minibatches per epoch kept instead (train.py:63), i.e. minibatch %d" % MB_SCALED,
               "note": "random-init weights, synthetic rollouts of the env itself; the value is the torch-learner row A"}
        if os.environ.get("SS_BENCH_TEST_TRANSPORT"):
            out["config"]["test_ppo_epochs"] = EPOCHS
            out["config"]["test_transport"] = ("%s, all %d ranks on cuda:0 -- a FUNCTIONAL run of the N > 1 path on a one-GPU box, never a "
                                               "measurement" % (os.environ["SS_BENCH_TEST_TRANSPORT"], world))
        out["transport"] = os.environ.get("SS_BENCH_TEST_TRANSPORT") or ("nccl" if use_dist else "none")
        sys.stdout.write(json.dumps(out) + "\n")
        sys.stdout.flush()


def extra_rows(torch, SteppingStoneVecEnv, dev, flop):
    """Side measurements on the same GPU (never the headline value): BASELINE.json configs[2] (MikeStepperEnv-v0, 4096
    envs, curriculum sampler on: level 5, uniform grid, then the peaked grid softmax(-10 |v - 0.85|) of a fixed
    synthetic v) and the chip's capacity at 32768 envs."""
    import numpy as np

    def rate(env, steps, spl):
        env.rollout_random(64, 0, steps_per_launch=min(spl, 64))
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); env.rollout_random(steps, 64, steps_per_launch=spl); e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / steps

    rows = {}
    mike = SteppingStoneVecEnv("MikeStepperEnv-v0", ENVS_PER_GPU, seed=0, device=dev, return_numpy=False)
    mike.update_curriculum(5)
    mike.reset()
    for name, spl in (("uniform", 500), ("uniform_per_step_launch", 1)):
        ms = rate(mike, 500, spl)
        rows["mike_4096_curriculum5_" + name] = {"ms_per_step": ms, "value": ENVS_PER_GPU / (ms * 1e-3), "steps_per_launch": spl}
    v = np.random.default_rng(0).random((11, 11))
    logits = -10.0 * np.abs(v - 0.85)
    p = np.exp(logits - logits.max())
    mike.update_sample_prob(p / p.sum())
    mike.reset()
    ms = rate(mike, 500, 500)
    rows["mike_4096_curriculum5_peaked"] = {"ms_per_step": ms, "value": ENVS_PER_GPU / (ms * 1e-3), "steps_per_launch": 500,
                                            "grid": "softmax(-10|v-0.85|), v = default_rng(0).random((11,11))"}
    st = mike.get_state()
    rows["mike_4096_curriculum5_peaked"]["mean_next_step_index"] = float(st[:, 59].mean())
    mike.close()
    big = SteppingStoneVecEnv(ENV_ID, 32768, seed=0, device=dev, return_numpy=False)
    big.reset()
    bms = rate(big, 200, 200)
    rows["capacity_32768"] = {"envs_per_gpu": 32768, "ms_per_step": bms, "value": 32768 / (bms * 1e-3), "unit": "env-steps/s",
                              "roofline_frac": (ALGO_WRITE_B + ALGO_READ_B / 200.0) * 32768 / (bms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                              "valu_fp32_frac": (flop * 32768 / (bms * 1e-3) / 1e12 / VALU_FP32_PEAK_TFLOPS) if flop else None,
                              "note": "same kernel at 32768 envs on this GPU (all 1024 SIMDs occupied); not the BASELINE config"}
    big.close()
    return rows


if __name__ == "__main__":
    main()
