"""bench.py — MoCo-v2 ResNet-50 two-view training step on N MI355X GPUs (one process per GPU).

    python bench.py                                   # N=1, 50 timed steps after 5 warm-up steps
    python bench.py --full                            # + roofline loop, CPU baseline, HBM-traffic figures
    python bench.py --dump-outputs DIR                # + what the last timed step computed, as DIR/<name>.npy
    python bench.py --gpus 8                          # spawns 8 ranks itself (torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        --master-port 29500 bench.py --gpus 8 --steps 50 --warmup 5       # the driver's form

One "step" = the full hot path of BASELINE.json configs[1] on one resident synthetic batch:
q forward (train BN), key-encoder EMA, k forward, fused InfoNCE, enqueue, backward, gradient
all-reduce (N>1), momentum-SGD, lr step — driven through the Trainer's whole hook bus
(train_iter_begin / train_iter_end of OptimizerHook, IterTimerHook, LogHook, LRSchedulerHook, ...).

A plain run sets up, warms up and times:
  1. the TIMED loop: exactly --steps steps, nothing but the product path between a barrier +
     torch.cuda.synchronize() on both sides -> `value`, `ms_per_step`.
With --full, after it:
  2. an INSTRUMENTED loop (HIP events around every launch of the three MFMA kernels on
     their launch stream; the library sums each launch's algorithmic FLOPs / bytes from its
     descriptor) -> `roofline` (the dominant kernel) + the two next ones.  It never contributes to
     `value`;
  3. the HBM-traffic floor of the step from the committed PMC summary (`hbm`), the exposed part of the
     gradient all-reduce (N > 1: 3 extra steps) and the CPU oracle baseline (`cpu_baseline`).
--dump-outputs DIR writes what the last timed step computed (rank 0): every tensor the step returns and a fixed
sample of the model's state after it (parameters, running statistics, MoCo's queue), as float32 / float64 .npy
files, under 64 MB in all.  The inputs (synthetic batch, initial weights: seeded here) are the same for the same
arguments.
Prints ONE JSON line (rank 0).  `value` = images/s over all ranks, where one image = one two-view
sample (PASSL's own `ips`, passl/engine/loops/loop.py:102-104).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FLOP_PER_SAMPLE = 32.77e9      # 2*[(3+1)*(4.0871+0.00446) + 2*0.00839] GMAC
PEAK_BF16_TFLOPS = 2500.0      # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3
PEAK_HBM_GBS = 8000.0          # HBM3E spec (MI355X_MICROARCH.md; ~6.3 TB/s is the measured streaming ceiling)
PMC_TRAFFIC_FILE = os.path.join('profiles', 'r06_pmc_traffic.json')
STREAM_HBM_GBS = 6290.0        # measured float4-copy ceiling (MI355X_MICROARCH.md, chip-level parameters)
MIXED_HBM_GBS = 5500.0         # what a dependent read + 16-byte-store stream of the 1x1 layers' shape reaches on this pool:
                               # 5.2 - 5.9 TB/s for every occupancy / persistence tried (scratch/probe/store_probe.cpp,
                               # profiles/r06_store_probe.txt)

# workload -> (config, default per-GPU batch, algorithmic FLOP per sample, metric text, workload text)
WORKLOADS = {
    'moco': ('configs/moco/moco_v2_r50_synthetic.yaml', 256, FLOP_PER_SAMPLE,
             'images/sec/node (2-view), MoCo-v2 R50 bs%d/GPU',
             'MoCo-v2 ResNet-50 %s, bs=%d/GPU, 2x224^2 synthetic views, queue=65536, dim=128, T=0.2, '
             'm=0.999, momentum-SGD (BASELINE configs[1])'),
    # SimCLR: 2 views x (fwd + bwd = 3) x 15.99 GMAC x 2 FLOP per two-view sample
    'simclr': ('configs/simclr/simclr_r50_synthetic.yaml', 64, 2 * 3 * 15.99e9 * 2,
               'images/sec/node (2-view), SimCLR R50 (no stem max-pool) bs%d/GPU',
               'SimCLR ResNet-50 (no stem max-pool) %s, bs=%d/GPU, 2x224^2 synthetic views, '
               'NT-Xent+CO2 T=0.1, LARS (SimCLR row; BASELINE configs[2] shape)'),
    # MAE ViT-B/16: 3 x 9.78 GMAC x 2 FLOP per image
    'mae': ('configs/mae/mae_vit_b_synthetic.yaml', 256, 3 * 9.78e9 * 2,
            'images/sec/node, MAE ViT-B/16 mask 0.75 bs%d/GPU',
            'MAE ViT-B/16 %s, bs=%d/GPU, 224^2 synthetic images, mask 0.75 (50 encoder / 197 decoder '
            'tokens), norm_pix_loss, AdamW (MAE row; BASELINE configs[3])'),
    # CLIP ViT-B/32: 4.41 GMAC (image, 50 tokens) + 2.98 GMAC (text, 77 tokens) per pair
    'clip': ('configs/clip/vit-b-32_synthetic.yaml', 128, 3 * 7.39e9 * 2,
             'image-text pairs/sec/node, CLIP ViT-B/32 bs%d/GPU',
             'CLIP ViT-B/32 + 12-layer causal text transformer %s, bs=%d/GPU, 224^2 synthetic images + '
             '77-token synthetic captions, AdamW (CLIP row; configs/clip/vit-b-32.yaml)'),
    # CLIP ViT-B/16 (BASELINE configs[4]): 17.56 GMAC image (197 tokens) + 2.98 GMAC text per pair
    'clip16': ('configs/clip/vit-b-16_synthetic.yaml', 256, 3 * (17.56e9 + 2.98e9) * 2,
               'image-text pairs/sec/node, CLIP ViT-B/16 bs%d/GPU',
               'CLIP ViT-B/16 + 12-layer causal text transformer %s, bs=%d/GPU, 224^2 synthetic images '
               '+ 77-token synthetic captions, cross-rank InfoNCE, AdamW (BASELINE configs[4] shape)'),
    # frozen trunk forward only (4.087 GMAC) + the fc
    'linprobe': ('configs/moco/moco_clas_r50_synthetic.yaml', 256, 4.09e9 * 2,
                 'images/sec/node, linear probe on frozen R50 bs%d/GPU',
                 'linear probe: frozen ResNet-50 (fused inference BN) + fc 2048->1000 %s, bs=%d/GPU, '
                 '224^2 synthetic labelled images, momentum-SGD on the fc (configs/moco/moco_clas_r50.yaml)'),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=None,
                    help='per-GPU batch (default: 256 = BASELINE configs[1]; simclr: 64; clip: 128)')
    ap.add_argument('--workload', default='moco', choices=sorted(WORKLOADS),
                    help="moco = BASELINE.json's metric (default); the others are the SimCLR / MAE / CLIP / "
                         'linear-probe rows (extra measurements)')
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'fp32'])
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--graph', action='store_true',
                    help='replay the captured HIP graph of the step (passl_amd/hip/graph.py) instead of launching '
                         'it kernel by kernel from Python; same as PASSL_GRAPH=1')
    ap.add_argument('--eager', action='store_true',
                    help='launch every kernel of the step from Python (same as PASSL_PLAN=0): the default replays '
                         'the recorded native step plan (passl_amd/hip/replay.py)')
    ap.add_argument('--no-kernel-timing', action='store_true',
                    help='skip the instrumented loop (use under rocprofv3)')
    ap.add_argument('--dp-buckets', type=int, default=0,
                    help='number of EQUAL gradient all-reduce buckets (default: two buckets, a big one and a <= 6 MB tail: core/sync_utils.py)')
    ap.add_argument('--dp-wire', default='', choices=['', 'fp32', 'bf16'],
                    help='dtype of the gradient buckets on the wire (default fp32 = the reference; bf16 halves the bytes per '
                         'xGMI link, sums agree to bf16 rounding: core/sync_utils.py)')
    ap.add_argument('--dp-force', action='store_true',
                    help='N=1 only: run the DATA-PARALLEL code path on the one GPU (world-size-1 RCCL communicator, '
                         'start-up broadcast, every gradient bucket all-reduced from inside backward, the step plan cut at '
                         'every collective; same as PASSL_DP_FORCE=1 under a launcher) — what the DP machinery costs '
                         'when the wire is free')
    ap.add_argument('--fresh-batches', type=int, default=0, metavar='RING',
                    help='after the timed loop on the resident batch, time the same number of steps again with MOVING '
                         'inputs: a ring of RING (>= 3) pinned host batches, each copied host -> device one step ahead '
                         'on a copy stream (datasets/synthetic.py:HostRingLoader) -> value_fresh_inputs')
    ap.add_argument('--roofline-steps', type=int, default=10,
                    help='steps of the instrumented loop that follows the timed loop (--full)')
    ap.add_argument('--full', action='store_true',
                    help='besides the headline figure, also measure what takes runs of its own: the instrumented '
                         'roofline loop, the exposed gradient all-reduce (N > 1), the HBM-traffic floor of the '
                         'committed PMC passes and the CPU baseline (off by default: a plain run only times the steps)')
    ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                    help='write what the last timed step computed as DIR/<name>.npy (float32 / float64, < 64 MB)')
    return ap.parse_args()


def _free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks (one per GPU) under
    torch.distributed.run on this node and pass rank 0's JSON line through."""
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
           '--nproc-per-node', str(args.gpus), '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')     # dmabuf IPC (RCCL across processes)
    env.setdefault('OMP_NUM_THREADS', '8')
    return subprocess.call(cmd, env=env)


def cpu_baseline():
    """The oracle (CPU restatement of the reference step) on the host cores, cfg-1 shape:
    median of 5 steps after 2 warm-ups."""
    import torch
    from oracle.moco import MoCoOracle
    n = 32
    torch.set_num_threads(min(os.cpu_count() or 1, 64))
    o = MoCoOracle(K=65536, seed=0)
    gen = torch.Generator().manual_seed(1234)
    xq = torch.randn(n, 3, 224, 224, generator=gen)
    xk = torch.randn(n, 3, 224, 224, generator=gen)
    for _ in range(2):
        o.train_step(xq, xk)
    times = []
    for _ in range(5):
        t = time.perf_counter()
        o.train_step(xq, xk)
        times.append(time.perf_counter() - t)
    sec = sorted(times)[len(times) // 2]
    return {'value': round(n / sec, 3), 'unit': 'images/sec', 'cores': torch.get_num_threads(),
            'kind': 'port',
            'sample': 'oracle (torch-CPU fp32 restatement; Paddle is not installable) full step, '
                      'N=32 two-view 224^2, K=65536, median of 5 after 2 warm-ups, %.2f s/step '
                      '(min %.2f, max %.2f)' % (sec, min(times), max(times))}


def pmc_traffic(args):
    """{'ring' | 'igemm' | 'wgrad': {hbm_bytes_per_launch, source}} from the committed rocprofv3 --pmc
    passes of this same command (tools/pmc_summary.py).  PMC counters need the profiler, so these numbers
    are NOT measured by this run — the source string says so; None for any other workload / shape."""
    path = os.path.join(ROOT, PMC_TRAFFIC_FILE)
    if args.workload != 'moco' or args.batch != 256 or args.dtype != 'bf16' or not os.path.exists(path):
        return None
    with open(path) as f:
        z = json.load(f)
    src = ('%s (separate rocprofv3 --pmc passes of this command: FETCH_SIZE x2 + WRITE_SIZE; '
           'not measured by this run)' % PMC_TRAFFIC_FILE)
    out = {}
    for k in ('ring', 'g8p', 'igemm', 'wgrad'):
        if k in z.get('classes', {}):
            out[k] = {'hbm_bytes_per_launch': z['classes'][k]['hbm_bytes_per_launch'], 'source': src}
    if 'fetch_gb_per_step' in z and 'write_gb_per_step' in z:
        out['_step'] = {'fetch_gb': z['fetch_gb_per_step'], 'write_gb': z['write_gb_per_step'], 'source': src}
    return out


DUMP_SAMPLE = 16384            # elements kept of a larger state tensor (--dump-outputs)


def dump_outputs(trainer, out_dir):
    """--dump-outputs: the tensors the last step returned (trainer.outputs) in full, and the model's state after that
    step (parameters and buffers: running statistics, MoCo's queue), a tensor of more than DUMP_SAMPLE elements as a
    fixed sample of its flattened values (indices drawn from a generator seeded by the tensor's name, sorted; the
    indices go to <name>.idx.npy).  float32, integer tensors float64.  -> (files, bytes)"""
    import zlib
    import numpy as np
    import torch

    os.makedirs(out_dir, exist_ok=True)
    files, nbytes = 0, 0

    def save(name, t, sample):
        nonlocal files, nbytes
        t = t.detach().reshape(-1) if sample else t.detach()
        if sample and t.numel() > DUMP_SAMPLE:
            gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
            idx = torch.randint(0, t.numel(), (DUMP_SAMPLE,), generator=gen).sort().values
            np.save(os.path.join(out_dir, name + '.idx.npy'), idx.double().numpy())
            nbytes += DUMP_SAMPLE * 8
            t = t[idx.to(t.device)]
        a = t.cpu()
        a = a.double() if not (a.is_floating_point() or a.is_complex()) else a.float()
        np.save(os.path.join(out_dir, name + '.npy'), a.numpy())
        files, nbytes = files + 1, nbytes + a.numel() * a.element_size()

    for k, v in sorted((trainer.outputs or {}).items()):
        if torch.is_tensor(v):
            save('out.' + k, v, sample=False)
    model = trainer.model.module if hasattr(trainer.model, 'module') else trainer.model
    for k, v in model.state_dict().items():
        if torch.is_tensor(v) and v.numel() > 0:
            save('state.' + k, v, sample=True)
    assert nbytes < 64 * 2 ** 20, 'bench.py --dump-outputs: %d bytes' % nbytes
    return files, nbytes


def pin_rank_to_cores():
    """One rank per GPU on one node: give every rank its own contiguous slice of the host's cores (LOCAL_RANK-th of
    LOCAL_WORLD_SIZE equal slices of the cores this process may run on).  The step's host side is one Python thread
    (plus the autograd thread); without pinning 8 ranks migrate across sockets and a slow host stalls every rank at
    the next gradient bucket.  PASSL_PIN_CORES=0 switches it off.  -> the core list, or None."""
    if os.environ.get('PASSL_PIN_CORES', '1') == '0' or not hasattr(os, 'sched_setaffinity'):
        return None
    try:
        local_world = int(os.environ.get('LOCAL_WORLD_SIZE', os.environ.get('WORLD_SIZE', 1)))
        local_rank = int(os.environ.get('LOCAL_RANK', 0))
        if local_world <= 1:
            return None
        cores = sorted(os.sched_getaffinity(0))
        per = len(cores) // local_world
        if per < 1:
            return None
        mine = cores[local_rank * per:(local_rank + 1) * per]
        os.sched_setaffinity(0, mine)
        os.environ.setdefault('OMP_NUM_THREADS', str(max(1, min(per, 8))))
        return mine
    except (OSError, ValueError):
        return None


def step_launch(trainer):
    """How the timed steps were issued."""
    sg = trainer.step_graph
    if sg is None or not sg.captured:
        why = getattr(sg, 'failed', None)
        return 'eager (one launch per kernel from the host)' + (' — step plan refused: %s' % why if why else '')
    if type(sg).__name__ == 'StepPlan':
        i = sg.info
        return ('native step plan (passl_amd/hip/replay.py: forward + backward + optimizer recorded once = %d kernel '
                'launches, %d event records, %d stream waits on %d streams, %d segment(s); %d replays in this process)'
                % (i['kernels'], i['event_records'], i['stream_waits'], i['streams'], i['segments'], sg.replays))
    return ('HIP graph replay (forward + backward + optimizer captured once, %d replays in this process)'
            % sg.replays)


def main():
    args = parse()
    # multi-process GPU work on this stack needs dmabuf IPC (RCCL across ranks); set here too, not only in
    # self_launch: the driver starts the ranks with torch.distributed.run itself
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    if args.dp_buckets:
        os.environ['PASSL_DP_BUCKETS'] = str(args.dp_buckets)
    if args.dp_wire:
        os.environ['PASSL_DP_WIRE'] = args.dp_wire
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(self_launch(args))
    if args.dp_force:
        if args.gpus != 1:
            raise SystemExit('bench.py: --dp-force is the 1-GPU rehearsal of the data-parallel path')
        os.environ['PASSL_DP_FORCE'] = '1'
        for k, v in (('RANK', '0'), ('LOCAL_RANK', '0'), ('WORLD_SIZE', '1'), ('MASTER_ADDR', '127.0.0.1'),
                     ('MASTER_PORT', str(_free_port()))):
            os.environ.setdefault(k, v)

    # stdout carries exactly ONE line (the JSON): everything else that writes to file descriptor 1 — RCCL prints its
    # version banner there when a communicator is created — goes to stderr from here on
    sys.stdout.flush()
    json_out = os.fdopen(os.dup(1), 'w')
    os.dup2(2, 1)

    pinned = pin_rank_to_cores()

    import torch
    import torch.distributed as dist

    cfg_path, default_batch, flop_per_sample, metric_fmt, workload_fmt = WORKLOADS[args.workload]
    if args.batch is None:
        args.batch = default_batch
    rank = int(os.environ.get('RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    if world != args.gpus:
        raise SystemExit('bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks'
                         % (args.gpus, world))
    assert torch.cuda.is_available(), 'bench.py runs the HIP path: an MI355X is required'

    from passl_amd.engine.trainer import Trainer
    from passl_amd.hip import lib as L, ops
    from passl_amd.utils import logger as plog
    from passl_amd.utils.config import get_config

    # stdout carries exactly one JSON line: LogHook's lines (rank 0, every log_config.interval
    # iterations, one device->host transfer each) go to stderr
    import logging
    lg = logging.getLogger('passl')
    lg.propagate = False
    lg.setLevel(logging.INFO if rank == 0 else logging.WARNING)
    if 'passl' not in plog.logger_initialized:
        lg.addHandler(logging.StreamHandler(stream=sys.stderr))
        plog.logger_initialized.append('passl')

    cfg = get_config(os.path.join(ROOT, cfg_path),
                     ['dataloader.train.sampler.batch_size=%d' % args.batch,
                      'compute_dtype=%s' % args.dtype])
    cfg.timestamp = ''
    if args.graph:
        cfg.hip_graph = True
    if args.eager:
        cfg.step_plan = False
    # the same arguments give the same inputs: the Trainer seeds only a non-zero config seed (the synthetic batch has
    # its own generator), and torch's default generator otherwise starts from a fresh seed in every process, so the
    # initial weights and MoCo's initial queue would differ from run to run
    import random
    import numpy as np
    seed = int(cfg.get('seed', 0) or 0) + rank
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)
    trainer = Trainer(cfg)
    trainer.mode = 'train'
    trainer.model.train()
    data = next(iter(trainer.train_dataloader))
    trainer.call_hook('run_begin')
    trainer.call_hook('train_epoch_begin')

    def step():
        # the body of Trainer.train's loop (engine/trainer.py) on the resident batch
        trainer.inner_iter = trainer.current_iter % trainer.iters_per_epoch
        trainer.current_iter += 1
        trainer.call_hook('train_iter_begin')
        trainer.train_step(data)          # eager, or the captured HIP graph of the step (passl_amd/hip/graph.py)
        trainer.call_hook('train_iter_end')

    def barrier():
        if world > 1:
            # (the communicator is created lazily — engine/trainer.py — so the barrier names its device itself)
            if dist.get_backend() == 'nccl':
                dist.barrier(device_ids=[torch.cuda.current_device()])
            else:
                dist.barrier()
        torch.cuda.synchronize()

    # PASSL_MAIN_PRIORITY: the whole iteration (hooks included: they read the step's outputs) under a stream of that
    # priority, so that the dependency chain is served before the side / key streams' fill-in work
    from passl_amd.hip import streams as hip_streams
    main_stream = hip_streams.main_stream(torch.device('cuda', torch.cuda.current_device()))
    if main_stream is not None:
        torch.cuda.synchronize()
        _plain_step = step

        def step():
            with torch.cuda.stream(main_stream):
                _plain_step()

    for _ in range(args.warmup):
        step()
    # a native step plan (hip/replay.py) runs a few eager steps and then records one before it replays: with a very
    # short --warmup those preparatory steps continue here, still outside the timed region
    extra_warm = 0
    sg = trainer.step_graph
    while sg is not None and getattr(sg, 'enabled', False) and not sg.captured and \
            getattr(sg, 'failed', None) is None and extra_warm < 8:
        step()
        extra_warm += 1

    # ---- 1. timed loop: product path only
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    host_elapsed = time.perf_counter() - t0          # the host is done enqueueing; the GPU may still be running
    barrier()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(trainer, args.dump_outputs)
    loss = float(trainer.outputs['loss'].detach())
    mem = torch.cuda.memory_stats()
    launch_desc = step_launch(trainer)      # how the TIMED steps were issued (the instrumentation below may drop the plan)

    t = torch.tensor([elapsed], dtype=torch.float64, device='cuda')
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())

    # ---- 1b. the same number of steps with MOVING inputs (verdict r05 #8 / #6): every step consumes a batch whose
    # host -> device copy ran on a copy stream while the previous step computed; nothing else differs
    fresh = None
    if args.fresh_batches:
        from passl_amd.datasets.synthetic import HostRingLoader
        ring = HostRingLoader(trainer.train_dataloader.inner if isinstance(trainer.train_dataloader, HostRingLoader)
                              else trainer.train_dataloader, ring=max(3, args.fresh_batches))
        resident = data

        def fresh_step():
            nonlocal data
            data = ring.take()
            step()
        for _ in range(3):
            fresh_step()
        barrier()
        tf0 = time.perf_counter()
        for _ in range(args.steps):
            fresh_step()
        barrier()
        tf = torch.tensor([time.perf_counter() - tf0], dtype=torch.float64, device='cuda')
        if world > 1:
            dist.all_reduce(tf, op=dist.ReduceOp.MAX)
        data = resident
        step()                       # back on the resident batch for the instrumented loop
        barrier()
        fresh = {'elapsed': float(tf.item()), 'ring': len(ring._host), 'bytes': ring.bytes_per_batch}

    # ---- 2. instrumented loop (rank 0's kernels; every rank runs the steps so collectives match).
    # HIP events around every launch of the MFMA kernel classes on their launch stream; the library sums
    # the launches' algorithmic FLOPs / bytes itself.  The side stream is off here so that a kernel's
    # duration is its own (in the timed loop the weight gradients run next to the main chain).
    kern, rsteps, instr_elapsed, event_overhead_us = {}, 0, 0.0, 0.0
    if args.full and not args.no_kernel_timing and args.roofline_steps > 0:
        import ctypes
        from passl_amd.hip import config as hip_config
        lib = L.load()
        rsteps = args.roofline_steps
        overlap_was = hip_config.overlap()
        hip_config.set_flag('overlap', False)
        graph_was = trainer.step_graph.enabled if trainer.step_graph is not None else None
        if trainer.step_graph is not None:
            trainer.step_graph.enabled = False          # per-launch HIP events need the eager step
            # a recorded plan keeps its whole step's memory reserved; the eager step beside it needs the same again
            # (SimCLR R50 at 512 / GPU: 184 GB + 167 GB).  The timed loop is over: give the plan's pool back first.
            free_b, total_b = torch.cuda.mem_get_info()
            if torch.cuda.memory_reserved() > free_b and hasattr(trainer.step_graph, 'reset'):
                trainer.outputs = None
                trainer.step_graph.reset()
                torch.cuda.empty_cache()
        step()
        barrier()
        lib.passl_hip_prof_enable(1)
        t1 = time.perf_counter()
        for _ in range(rsteps):
            step()
        barrier()
        instr_elapsed = time.perf_counter() - t1
        for cls, name in ((0, 'ring'), (1, 'wgrad'), (2, 'igemm'), (3, 'g8p')):
            ms, n = ctypes.c_double(), ctypes.c_int64()
            fl, by = ctypes.c_double(), ctypes.c_double()
            lib.passl_hip_prof_collect(cls, ctypes.byref(ms), ctypes.byref(n))
            lib.passl_hip_prof_collect_work(cls, ctypes.byref(fl), ctypes.byref(by))
            kern[name] = dict(ms=ms.value, n=n.value, flops=fl.value, bytes=by.value)
        lib.passl_hip_prof_enable(0)
        ov = ctypes.c_double()
        lib.passl_hip_prof_event_overhead(256, L.stream(), ctypes.byref(ov))
        event_overhead_us = ov.value
        hip_config.set_flag('overlap', overlap_was)
        if trainer.step_graph is not None:
            trainer.step_graph.enabled = graph_was

    # ---- 3. who took part (every rank reports its device) and what the gradient all-reduce cost in the open
    dist_info = None
    if world > 1 or dist.is_initialized():
        props = torch.cuda.get_device_properties(torch.cuda.current_device())
        me = {'rank': rank, 'device': torch.cuda.current_device(), 'name': props.name,
              'uuid': str(getattr(props, 'uuid', '')), 'pci_bus_id': getattr(props, 'pci_bus_id', None),
              'host': socket.gethostname(), 'pid': os.getpid()}
        everyone = [None] * world
        dist.all_gather_object(everyone, me)
        exposed = None
        red = getattr(trainer, 'grad_reducer', None)
        host_ms = None
        if red is not None and args.full:
            red.measure = True
            for r_ in getattr(red, 'reducers', [red]):
                r_.host_ms, r_.host_calls = 0.0, 0
            for _ in range(3):
                step()
            exposed = red.exposed_ms()
            red.measure = False
            rs_ = getattr(red, 'reducers', [red])
            host_ms = (round(sum(r_.host_ms for r_ in rs_) / 3, 3), sum(r_.host_calls for r_ in rs_) // 3)
        ex = torch.tensor([exposed if exposed is not None else -1.0], dtype=torch.float64, device='cuda')
        dist.all_reduce(ex, op=dist.ReduceOp.MAX)
        dist_info = {'backend': dist.get_backend(), 'world': dist.get_world_size(), 'ranks': everyone,
                     'distinct_devices': len({(e['host'], e['uuid'] or e['device']) for e in everyone}),
                     'grad_buckets': len(red.buckets) if red is not None else 0,
                     'grad_bytes': int(red.grads.numel() * 4) if red is not None else 0,
                     'grad_wire_dtype': ('bf16' if red.wire is not None else 'fp32') if red is not None else None,
                     'grad_wire_bytes': int(red.grads.numel() * (2 if red.wire is not None else 4)) if red is not None else 0,
                     'allreduce_exposed_ms': round(float(ex.item()), 3) if float(ex.item()) >= 0 else None,
                     'collective_host_ms_per_step': host_ms[0] if host_ms else None,
                     'collective_host_calls_per_step': host_ms[1] if host_ms else None,
                     'allreduce_exposed_what': 'max over ranks of the time the compute stream waits for gradient '
                                               'collectives after backward has finished (3 extra steps, HIP events)'}

    if rank == 0:
        ips = args.batch * world * args.steps / elapsed
        peak = PEAK_BF16_TFLOPS if args.dtype == 'bf16' else PEAK_F32_TFLOPS
        out = {
            'metric': metric_fmt % args.batch,
            'value': round(ips, 2), 'unit': 'images/sec', 'n_gpus': world, 'steps': args.steps,
            'warmup': args.warmup, 'ms_per_step': round(1000 * elapsed / args.steps, 3),
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
            'dtype': args.dtype, 'data': 'synthetic',
            'config': {'workload': workload_fmt % (args.dtype, args.batch),
                       'global_batch': args.batch * world, 'parallelism': 'dp%d' % world,
                       'views_per_sec': round(2 * ips, 2), 'final_loss': round(loss, 4),
                       'hbm_allocated_gb': round(mem.get('allocated_bytes.all.peak', 0) / 2 ** 30, 1),
                       'hbm_reserved_gb': round(mem.get('reserved_bytes.all.peak', 0) / 2 ** 30, 1),
                       'allocator_retries': int(mem.get('num_alloc_retries', 0)),
                       'timed_region': 'product path only (full hook bus); kernel instrumentation (--full) '
                                       'runs in a separate loop afterwards',
                       'host_enqueue_ms_per_step': round(1000 * host_elapsed / args.steps, 3),
                       'step_launch': launch_desc, 'extra_untimed_steps': extra_warm,
                       'main_stream_priority': main_stream.priority if main_stream is not None else None},
            'step_flop_roofline': {
                'algorithmic_gflop_per_sample': flop_per_sample / 1e9,
                'achieved_tflops_per_gpu': round(ips / world * flop_per_sample / 1e12, 2),
                'frac_of_peak': round(ips / world * flop_per_sample / 1e12 / peak, 5)},
        }
        step_traffic = (pmc_traffic(args) or {}).get('_step') if args.full else None
        if step_traffic is not None:
            # the whole step against what its HBM traffic alone would cost (round-4 verdict: put the "x times its
            # traffic floor" claim into the record): counter bytes of the committed PMC passes of this command over
            # the measured streaming ceiling and over the spec
            gb = step_traffic['fetch_gb'] + step_traffic['write_gb']
            out['hbm_bytes_per_step'] = round(gb * 1e9)
            out['hbm_floor_ms'] = round(gb / STREAM_HBM_GBS * 1e3, 3)
            out['hbm'] = {'gb_per_step': round(gb, 2), 'fetch_gb': step_traffic['fetch_gb'],
                          'write_gb': step_traffic['write_gb'],
                          'floor_ms_at_measured_copy_ceiling_6.29TBs': round(gb / STREAM_HBM_GBS * 1e3, 3),
                          'floor_ms_at_spec_8TBs': round(gb / PEAK_HBM_GBS * 1e3, 3),
                          'floor_ms_at_measured_mixed_rw_ceiling_5.5TBs': round(gb / MIXED_HBM_GBS * 1e3, 3),
                          'step_over_floor': round(1000 * elapsed / args.steps / (gb / STREAM_HBM_GBS * 1e3), 3),
                          'average_tb_per_s': round(gb / (1000 * elapsed / args.steps), 3),
                          'average_over_mixed_rw_ceiling': round(gb / (1000 * elapsed / args.steps) / (MIXED_HBM_GBS / 1e3), 3),
                          'source': step_traffic['source']}
        if kern and kern['ring']['n'] + kern['igemm']['n'] + kern['g8p']['n'] > 0:
            traffic = pmc_traffic(args)

            def block(k, title, _unused=None):
                """Both roofs for the class: its launches' algorithmic FLOPs over the MFMA peak and their algorithmic
                bytes over the HBM spec, each as a time floor; the BINDING roof is the larger floor (verdict r05 #5:
                the bound used to be hard-coded per class) and `frac` = that floor / measured time."""
                d = kern[k]
                if d['n'] == 0:
                    return None
                sec = d['ms'] * 1e-3
                tf, gbs = d['flops'] / sec / 1e12, d['bytes'] / sec / 1e9
                frac_mfma, frac_hbm = tf / peak, gbs / PEAK_HBM_GBS
                bound = 'mfma' if frac_mfma >= frac_hbm else 'hbm'
                b = {'kernel': title, 'bound': bound,
                     'achieved': round(tf if bound == 'mfma' else gbs, 2),
                     'peak': peak if bound == 'mfma' else PEAK_HBM_GBS,
                     'unit': 'TFLOP/s' if bound == 'mfma' else 'GB/s',
                     'frac': round(max(frac_mfma, frac_hbm), 5),
                     'frac_mfma': round(frac_mfma, 5), 'frac_hbm': round(frac_hbm, 5),
                     'frac_hbm_of_measured_copy_ceiling': round(gbs / STREAM_HBM_GBS, 5),
                     'frac_hbm_of_measured_mixed_rw_ceiling_5.5TBs': round(gbs / MIXED_HBM_GBS, 5),
                     'floor_us_mfma': round(d['flops'] / d['n'] / (peak * 1e12) * 1e6, 2),
                     'floor_us_hbm': round(d['bytes'] / d['n'] / (PEAK_HBM_GBS * 1e9) * 1e6, 2),
                     'launches': int(d['n']), 'avg_launch_us': round(1000 * d['ms'] / d['n'], 2),
                     'algorithmic_gflop_per_launch': round(d['flops'] / d['n'] / 1e9, 3),
                     'algorithmic_mb_per_launch': round(d['bytes'] / d['n'] / 1e6, 2),
                     'achieved_tflops': round(tf, 2), 'achieved_algorithmic_gbs': round(gbs, 1),
                     'kernel_ms_per_step': round(d['ms'] / rsteps, 3)}
                t = (traffic or {}).get(k)
                b['traffic'] = t['hbm_bytes_per_launch'] if t else None
                b['traffic_unit'] = 'HBM bytes per launch'
                b['traffic_source'] = t['source'] if t else None
                return b
            # `roofline` = the kernel class that holds the largest share of the step's kernel time over ALL four
            # instrumented classes (round-3 verdict: the choice used to be between the two LDS-DMA kernels only, while
            # the register-staged HBM-bound kernel was the largest).  The other three are reported beside it.
            titles = {
                'ring': ('igemm_ring_kernel (LDS-DMA ring implicit GEMM, 128-row tiles: conv fwd / dgrad and Linear with '
                         'a reduction of >= 512 that the 8-phase kernel does not take)', 'mfma', 'roofline_ring_kernel'),
                'g8p': ('igemm_8p_kernel (LDS-DMA implicit GEMM, 256 x 256 tiles, 8-phase schedule: wide and deep conv '
                        'fwd / dgrad and Linear launches)', 'mfma', 'roofline_8p_kernel'),
                'igemm': ('igemm_kernel (register-staged implicit GEMM: 1x1 layers with a reduction < 512, stem)',
                          'hbm' if args.dtype == 'bf16' else 'mfma', 'roofline_hbm_kernel'),
                'wgrad': ('wgrad_pipe_kernel + wgrad_halo_kernel (weight gradients, split over M + fixed-order slab reduction; the 3x3 / stride-1 '
                          'layers on the spatially tiled kernel since round 5)', 'mfma',
                          'roofline_wgrad_kernel')}
            blocks = {k: block(k, t[0], t[1]) for k, t in titles.items()}
            dominant = max((k for k in blocks if blocks[k] is not None), key=lambda k: kern[k]['ms'])
            out['roofline'] = blocks[dominant]
            out['roofline']['dominant_of'] = {k: round(kern[k]['ms'] / rsteps, 3) for k in blocks if blocks[k] is not None}
            out['roofline']['measured_over'] = (
                '%d instrumented steps after the timed loop, eager launches, side stream off (%.3f ms/step with the HIP '
                'events in place); avg_launch_us is an (event, kernel, event) reading: the same bracket around nothing '
                'reads %.1f us on this stream, rocprofv3 kernel durations (profiles/) are shorter by about that'
                % (rsteps, 1000 * instr_elapsed / rsteps, event_overhead_us))
            out['roofline']['event_bracket_overhead_us'] = round(event_overhead_us, 2)
            for k, t in titles.items():
                if k != dominant and blocks[k] is not None:
                    out[t[2]] = blocks[k]
            ig = {k: kern['ring'][k] + kern['igemm'][k] + kern['g8p'][k] for k in ('ms', 'n', 'flops', 'bytes')}
            out['igemm_class'] = {
                'what': 'all implicit-GEMM kernels together (the r01 roofline definition)',
                'achieved_tflops': round(ig['flops'] / (ig['ms'] * 1e-3) / 1e12, 2),
                'frac_of_mfma_peak': round(ig['flops'] / (ig['ms'] * 1e-3) / 1e12 / peak, 5),
                'kernel_ms_per_step': round(ig['ms'] / rsteps, 3), 'launches': int(ig['n'])}
        if fresh is not None:
            ips_f = args.batch * world * args.steps / fresh['elapsed']
            out['value_fresh_inputs'] = round(ips_f, 2)
            out['fresh_inputs'] = {
                'ms_per_step': round(1000 * fresh['elapsed'] / args.steps, 3),
                'ratio_to_resident': round(ips_f / ips, 4),
                'host_ring_batches': fresh['ring'], 'h2d_bytes_per_step': fresh['bytes'],
                'h2d_gb_per_s_needed': round(fresh['bytes'] * args.steps / fresh['elapsed'] / 1e9, 2),
                'what': 'the same %d timed steps again, every step on a batch copied from a ring of pinned host batches '
                        'one step ahead on a copy stream (datasets/synthetic.py:HostRingLoader); `value` above is the '
                        'resident-batch number SURVEY 8(d) prescribes' % args.steps}
        if dist_info is not None:
            dist_info['rank0_cores'] = ('%d-%d' % (pinned[0], pinned[-1])) if pinned else None
            out['dist'] = dist_info
        if args.full and world == 1 and not args.no_cpu_baseline and args.workload == 'moco':
            out['cpu_baseline'] = cpu_baseline()
        json_out.write(json.dumps(out) + '\n')
        json_out.flush()
    if world > 1:
        barrier()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
