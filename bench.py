"""
bench.py -- rendered rays/s of the per-ray volume-rendering hot path on MI355X.

Workload (BASELINE.json configs[1]): Replica room0-sized synthetic box room, 640x480 full-frame
``Renderer.render_img`` (stage color, no_grad), 64 samples/ray = N_samples 48 + N_surface 16,
in the reference's 100 000-ray batches.  One "step" = one full frame (307 200 rays).  Inputs
(grids, 785 MB TSDF, decoder weights, pose, depth image) are resident in HBM before the timed
region; the per-call layout conversions of my path (grid relayout, weight packing) are
invalidated every step so that they are INSIDE the timed region.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run does only what the headline needs: it sets up, warms up, times the K steps, writes the outputs if ``--dump-outputs``
is given and prints the result line.  ``--full`` adds, after that and before the line is printed, every other leg this file knows
(`weak`, `config.shard_model`, `strong`, `train_allreduce`, `roofline`, the exact-f32 and x20-grid frames, `sustained`, the other
configurations, `torch_gpu_baseline`, `cpu_baseline` and the parity against the oracle); ``--no-extra``, ``--no-stage-timing``,
``--no-shard-model`` and ``--cpu-rays`` trim a ``--full`` run and change nothing in a plain one.

``--dump-outputs DIR``: after the timed steps, rank 0 writes the images the last timed step returned (what a caller of
``Renderer.render_img`` receives) as ``DIR/depth.npy``, ``DIR/uncertainty.npy`` and ``DIR/color.npy`` in float32 (6 MB).  The
inputs are seeded, so two builds run with the same arguments can be compared output for output.

``--gpus N`` with N > 1 and no WORLD_SIZE in the environment: this process touches no GPU, starts N worker
processes (one per GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT set, backend
"nccl" = RCCL) and relays rank 0's JSON line.  Under ``python -m torch.distributed.run --nproc-per-node N ...
bench.py --gpus N`` the environment is already there and every process is a worker.

Headline at every N ("strong" scaling: the work of a step is ONE 640x480 frame whatever N is): at N = 1 the frame is
``Renderer.render_img``; at N > 1 it is the same frame RAY-SHARDED (attentive_dfprior_amd.dist.render_img_sharded: rank r renders the
contiguous pixel range [r HW/N, (r+1) HW/N) with the far clamps of the reference's 100 000-ray batches taken over the whole frame, ONE
packed all-gather of 28 B per ray hands every rank the images -- bit for bit render_img's) with the all-gather INSIDE the timed region;
value = rays of the frame x steps / max-over-ranks time.  With ``--full``, `weak` (N > 1) keeps the round-1..4 headline beside it: one
whole frame per rank, no data-path collective.  `config.shard_model` (N = 1, ``--full``) times a 1/2, 1/4 and 1/8 shard of the frame on
the one GPU, per-step fixed costs included, and states the efficiency bound t(full) / (k t(1/k)) they imply for N = k.

Rank 0 prints ONE JSON line with the contract fields; with ``--full`` also
  roofline        dominant kernel (colour decoder): executed-MFMA FLOP and algorithmic FLOP per launch / HIP-event
                  time of that kernel alone on the launch stream
  roofline_tsdf   the HBM-side trilerp stage (k_tsdf): 32 algorithmic bytes per sample (room0: cache-resident)
  config5         the one configuration whose TSDF streams from HBM (1024^3 = 4.3 GB, 128 samples/ray, one GPU's
                  share of 1 M rays): rays/s and the trilerp stage's roofline there
  strong          ONE 640x480 frame sharded over the ranks (contiguous ray slices, full-batch depth max,
                  outputs all-gathered) -- the north star's "GPU g gets the contiguous ray slice"
  train_allreduce one 5 000-ray Mapper iteration per step with the rays sharded over the ranks and ONE flat-bucket
                  RCCL all-reduce of the loss gradients (48.6 MB at room0), and the frustum-masked bucket variant
  sustained       the headline loop run for >= 2 s
  torch_gpu_baseline  the reference's PyTorch ops (the oracle's functions) on the same GPU through PyTorch-ROCm
  cpu_baseline    the oracle (CPU PyTorch restatement == reference) timed on this host's cores on a bounded ray
                  sample of the same workload; parity_vs_oracle compares THE TIMED OUTPUT on those rays
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# algorithmic work per sample point (SURVEY.md section 8d / BASELINE.md section 3)
MAC_LOW, MAC_HIGH, MAC_COLOR, MAC_ATT = 15479, 20599, 15575, 33024
TSDF_BYTES_PER_SAMPLE = 32
PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, spec
PEAK_F16_MFMA_TFLOPS = 2500.0     # MI355X_MICROARCH.md: dense f16/bf16 MFMA, spec
F16X3_FLOP_COLOR = 90 * 32 * 32 * 16 * 2 / 32.0   # executed f16 MFMA FLOP per sample: 90 x 32x32x16 per 32-point tile
PEAK_HBM_GBPS = 8000.0            # MI355X_MICROARCH.md: HBM3E spec
CFG64 = {'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': 48, 'N_surface': 16, 'N_importance': 0},
         'scale': 1, 'occupancy': True, 'meshing': {'resolution': 256}}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--scene', default='room0')
    ap.add_argument('--full', action='store_true',
                    help='after the headline, also run every other leg (scaling, roofline, other precisions and configurations, baselines, parity)')
    ap.add_argument('--cpu-rays', type=int, default=20000, help='--full: ray sample of the CPU baseline leg (0 = skip)')
    ap.add_argument('--no-stage-timing', action='store_true', help='--full: skip the per-kernel timing (roofline)')
    ap.add_argument('--no-shard-model', action='store_true', help='--full: skip config.shard_model (its shard-sized launches would mix into a kernel-trace profile of the timed loop)')
    ap.add_argument('--no-extra', action='store_true', help='--full: headline + roofline only (skip sustained / config5 / torch-gpu / dist legs)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the last timed step\'s depth / uncertainty / colour images to DIR/<name>.npy (float32)')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    return args


def dump_outputs(out_dir, names, tensors):
    """The timed path's outputs as DIR/<name>.npy, float32 (float64 stays float64)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, t in zip(names, tensors):
        a = t.detach().cpu().numpy()
        np.save(os.path.join(out_dir, name + '.npy'), a if a.dtype == np.float64 else a.astype(np.float32))


# ----------------------------------------------------------------------------------------------------------
# launcher: --gpus N without a torch.distributed environment.  Nothing here may initialise the GPU.
# ----------------------------------------------------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_workers(args):
    import torch
    have = torch.cuda.device_count()                     # counting devices does not initialise HIP
    if os.environ.get('ADFP_BENCH_TEST_SAME_DEVICE') == '1':       # test hook (tests/test_gpu_bench_world2.py): all ranks on cuda:0
        have = max(have, args.gpus)
    if have < args.gpus:
        print(f'bench.py: --gpus {args.gpus} but this node exposes {have} GPU(s)', file=sys.stderr)
        sys.exit(2)
    port = free_port()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    # Rank 0's stdout (the ONE JSON line) is drained by a thread while the parent watches all ranks: a rank that dies would leave
    # the others waiting in a collective until the 30-minute process-group timeout, so the first failure ends the whole job.
    import threading
    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    deadline = time.time() + 3600
    failed = None
    while any(p.poll() is None for p in procs):
        bad = [p.returncode for p in procs if p.poll() is not None and p.returncode != 0]
        if bad or time.time() > deadline:
            failed = bad[0] if bad else -9
            for p in procs:
                if p.poll() is None:
                    p.kill()                      # the exact children this parent started
            break
        time.sleep(0.2)
    for p in procs:
        p.wait()
    reader.join(timeout=10)
    out = b''.join(c for c in chunks if c)
    rcs = [failed] if failed is not None else [p.returncode for p in procs]
    sys.stdout.write(out.decode())
    sys.stdout.flush()
    sys.exit(max(abs(rc) for rc in rcs))


# ----------------------------------------------------------------------------------------------------------
def strip_c_comments(text):
    """C / C++ source without its comments and with white space collapsed: what the compiler sees of it, near enough.  The stamp
    below is taken over THIS, so that correcting a comment does not mark every committed profile stale (round 4 left a wrong
    'PARITY UNPINNED' comment in place for that reason)."""
    out, i, n = [], 0, len(text)
    while i < n:
        ch = text[i]
        if ch == '/' and i + 1 < n and text[i + 1] == '/':
            j = text.find('\n', i)
            i = n if j < 0 else j
        elif ch == '/' and i + 1 < n and text[i + 1] == '*':
            j = text.find('*/', i + 2)
            i = n if j < 0 else j + 2
            out.append(' ')
        elif ch in '"\'':
            j = i + 1
            while j < n and text[j] != ch:
                j += 2 if text[j] == '\\' else 1
            out.append(text[i:j + 1])
            i = j + 1
        else:
            out.append(ch)
            i += 1
    return ' '.join(''.join(out).split())


def source_hash():
    """sha256 of the kernel sources + C header, comments and white space stripped: stamps profile-derived numbers with the build
    they belong to."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, 'attentive_dfprior_amd', 'csrc')
    for f in sorted(os.listdir(d)) + ['../../include/adfp.h']:
        p = os.path.join(d, f)
        if os.path.isfile(p) and p.endswith(('.h', '.hip')):
            h.update(strip_c_comments(open(p, 'r', errors='replace').read()).encode())
    return h.hexdigest()[:16]


def pmc_traffic(kernel_prefix, samples_per_launch, fname='r05_pmc_hbm_traffic.csv', exact=False):
    """HBM bytes per launch of one kernel from the committed PMC passes (rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE,
    separate runs; the csv holds bytes per sample): the counters cannot be read from inside this process, so the figure
    is the PROFILED bytes/sample x this run's samples per launch.  Returns (bytes or None, provenance dict); the csv's
    header carries the source hash of the build it was taken from and `stale` says whether that is this build."""
    import csv
    stem = fname.split('_', 1)[1]                       # the newest round's file of that name, unless `exact`
    names = (fname,) if exact else tuple(f'r{r:02d}_{stem}' for r in range(6, 0, -1))
    for name in names:
        path = os.path.join(ROOT, 'profiles', name)
        if os.path.exists(path):
            break
    else:
        return None, {'file': None}
    head = open(path).readline()
    stamp = head.split('source_hash=')[1].split()[0].strip() if 'source_hash=' in head else None
    prov = {'file': 'profiles/' + os.path.basename(path), 'profiled_source_hash': stamp, 'this_source_hash': source_hash(),
            'stale': stamp != source_hash()}
    with open(path) as f:
        rows = [r for r in csv.reader(l for l in f if not l.startswith('#'))]
    for r in rows[1:]:
        if r[0].startswith(kernel_prefix):
            return (float(r[3]) + float(r[4])) * samples_per_launch, prov
    return None, prov


# Feature-grid scale of the bench scene.  The HEADLINE runs at SURVEY.md section 8d's prescription: the grids initialised like
# src/DF_Prior.py:247-263 -- N(0, 0.01) low / colour, N(0, 1e-4) high (GRID_STD_SCALE = 1).  At that scale the seeded random
# decoders output an almost constant occupancy, so the same frame is ALSO timed and checked against the oracle with the grids
# multiplied (x 20, the high grid x 100 on top: std 0.2 everywhere; rounds 1-5 ran the headline there), where occupancy, attention
# weights and colour vary along a ray like with a trained map: `config.value_at_x20_grids`, `config.parity_max_rel_*_at_x20`.  Kernel
# time does not depend on the values (tests/test_gpu_scale.py covers the init scale and a trained scale for parity).
GRID_STD_SCALE, GRID_HIGH_EXTRA = 1.0, 1.0
X20_STD_SCALE, X20_HIGH_EXTRA = 20.0, 100.0


def isa_mix_lc16(fname='r06_isa_mix_lc16.txt'):
    """Instruction counts of ONE 32-point tile of k_decode_lc16 (both networks): the TILE LOOP of the compiled kernel
    (tools/gen_isa_mix.py -> tools/isa_mix.py --loop), read from the committed file whose header carries the source hash of the
    build it was taken from; `stale` = that is not this build."""
    import re
    path = os.path.join(ROOT, 'profiles', fname)
    out = {'file': 'profiles/' + fname, 'this_source_hash': source_hash()}
    if not os.path.exists(path):
        return dict(out, file=None)
    text = open(path).read()
    m = re.search(r'source_hash=(\w+)', text)
    out['profiled_source_hash'] = m.group(1) if m else None
    out['stale'] = out['profiled_source_hash'] != out['this_source_hash']
    m = re.search(r'\[tile loop only\]: (\d+) instr, VALU (\d+) \(packed \d+\), MFMA (\d+), LDS (\d+), VMEM (\d+), SALU (\d+)', text)
    if m:
        out.update(instructions=int(m.group(1)), valu=int(m.group(2)), mfma=int(m.group(3)), lds=int(m.group(4)), vmem=int(m.group(5)), salu=int(m.group(6)))
    return out


def pmc_sq(kernel_prefix, fname='r05_pmc_sq_forward.txt'):
    """MFMA-busy fraction and delivered clock of one kernel from the committed SQ counter summary (tools/pmc_summary.py output)."""
    out = {'file': None}
    stem = fname.split('_', 1)[1]
    for r in range(6, 3, -1):                            # the newest round's summary
        fname = f'r{r:02d}_{stem}'
        path = os.path.join(ROOT, 'profiles', fname)
        if os.path.exists(path):
            break
    else:
        return out
    out['file'] = 'profiles/' + fname
    take = False
    for line in open(path):
        if line.startswith('=='):
            take = kernel_prefix in line
        elif take and 'mfma busy frac' in line:
            parts = line.replace('=', ' ').split()
            try:
                out['mfma_busy_frac'] = float(parts[parts.index('frac') + 1])
                out['clock_ghz'] = float(parts[parts.index('GHz') + 1])
            except (ValueError, IndexError):
                pass
            break
    return out


def build_scene(A, synthetic, name, dev, H=480, W=640, std_scale=X20_STD_SCALE, high_extra=X20_HIGH_EXTRA):
    """(scene, state dict, decoders).  Default grids: the x20 variant (what the tools profile); the headline passes the reference's init."""
    scene = synthetic.Scene(name, H=H, W=W, device=dev, grid_std_scale=std_scale)
    if high_extra != 1.0:
        scene.c['grid_high'] = scene.c['grid_high'] * high_extra
    sd = synthetic.seeded_state_dict(0)
    dec = A.DF()
    dec.load_state_dict(sd)
    dec.bound = scene.bound
    dec = dec.to(dev)
    return scene, sd, dec


def main():
    args = parse()
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        launch_workers(args)                                         # never returns
    import torch
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    # Test hooks (never set by the driver): ADFP_BENCH_TEST_SAME_DEVICE=1 puts every rank on cuda:0 and
    # ADFP_BENCH_TEST_BACKEND=gloo replaces RCCL, so that the N > 1 control flow of this file -- self-launch, barriers, the
    # max over ranks, the sharded legs -- can be exercised on a box with ONE GPU (RCCL refuses two ranks on one device).
    backend = os.environ.get('ADFP_BENCH_TEST_BACKEND', 'nccl')
    if os.environ.get('ADFP_BENCH_TEST_SAME_DEVICE') == '1':
        local_rank = 0
    dev = torch.device(f'cuda:{local_rank}')
    torch.cuda.set_device(dev)
    dist = None
    if world > 1:
        import datetime
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29533')
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=dev, timeout=datetime.timedelta(minutes=30))
        else:       # test hook (gloo on one device): a stuck collective should raise within minutes, not hold the suite for half an hour
            dist.init_process_group(backend, timeout=datetime.timedelta(minutes=3))
    n_gpus = dist.get_world_size() if dist is not None else 1
    if args.gpus != n_gpus and rank == 0:
        print(f'bench.py: --gpus {args.gpus} but the process group has {n_gpus} rank(s); reporting n_gpus={n_gpus}', file=sys.stderr)

    import attentive_dfprior_amd as A
    from attentive_dfprior_amd import synthetic, _lib
    L = _lib.lib()

    H, W, NS, NF = 480, 640, 48, 16
    S = NS + NF
    scene, sd, dec = build_scene(A, synthetic, args.scene, dev, std_scale=GRID_STD_SCALE, high_extra=GRID_HIGH_EXTRA)
    rend = A.Renderer(CFG64, None, scene)
    tsdf_bnds = scene.tsdf_bnds.to(dev)
    # one pose per rank (weak scaling: every rank renders a full frame)
    c2w = scene.default_c2w(offset=(0.3 * rank, 0.1 * rank, 0.0), yaw=0.3 + 0.4 * rank, pitch=-0.1)
    gt_depth = scene.depth_image(c2w)
    n_rays = H * W

    def frame_step():
        rend._engine._grid_cache.clear()      # relayout + packing inside the timed region
        dec._packed.clear()
        return rend.render_img(scene.c, dec, c2w, dev, scene.tsdf_volume, tsdf_bnds, 'color', gt_depth=gt_depth)

    # N > 1: ONE frame (rank 0's pose on every rank), ray-sharded, outputs all-gathered inside the step
    c2w0 = scene.default_c2w(offset=(0.0, 0.0, 0.0), yaw=0.3, pitch=-0.1)
    gt_depth0 = scene.depth_image(c2w0)

    def sharded_step():
        from attentive_dfprior_amd import dist as adist
        rend._engine._grid_cache.clear()
        dec._packed.clear()
        return adist.render_img_sharded(rend, scene.c, dec, c2w0, dev, scene.tsdf_volume, tsdf_bnds, 'color', gt_depth0)

    step = frame_step if dist is None or n_gpus == 1 else sharded_step

    def barrier():
        torch.cuda.synchronize(dev)
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)

    def timed_loop(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = fn()
        barrier()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, out

    elapsed, out = timed_loop(step, args.steps, args.warmup)
    depth_img, unc_img, color_img = out
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, ('depth', 'uncertainty', 'color'), out)
    assert torch.isfinite(depth_img).all() and torch.isfinite(color_img).all()
    rend.check_overflow(dev)

    ms_per_step = elapsed / args.steps * 1e3
    value = n_rays * args.steps / elapsed                # ONE frame per step at every N (strong scaling)

    result = {
        'metric': 'rendered rays/sec (64 samples/ray), Replica room0',
        'value': value, 'unit': 'rays/s', 'n_gpus': n_gpus, 'steps': args.steps, 'warmup': args.warmup,
        'ms_per_step': ms_per_step, 'higher_is_better': True, 'scaling': 'strong', 'vs_baseline': None,
        # the arithmetic the timed path computes in: f32 values; in the default mode every decoder product is formed on f16 MFMA
        # from a hi + lo split of both f32 operands (3 f16 products, 22-bit product mantissa, f32 accumulate, |x| < 65504 or the
        # call repairs itself in f32); ADFP_MATH=f32 = exact f32-input MFMA, reported beside it as `value_f32`
        'dtype': ('f32 via f16x3 split (3 f16 MFMA products per f32 product: 22-bit products, f32 accumulate)'
                  if os.environ.get('ADFP_MATH', 'f16x3') == 'f16x3' else 'f32'),
        'data': 'synthetic', 'math': os.environ.get('ADFP_MATH', 'f16x3'),
        # the first ~120 characters carry what qualifies the number (the driver's record cuts the string there)
        'config': {'workload': f'{args.scene} 640x480 render_img, 64 spp (48+16), synthetic box room, seed-0 random decoders, grids at the REFERENCE init '
                               '(N(0,.01), high N(0,1e-4)); stage color, ray_batch_size 100000 (per-batch far clamp, '
                               'rendered as one call with a depth maximum per 100 000-ray segment), ONE frame per step' + ('' if n_gpus == 1 else f', ray-sharded over the {n_gpus} GPUs (contiguous pixel ranges, one packed all-gather inside the step)'),
                   'grid_std_scale': GRID_STD_SCALE,     # 1 = src/DF_Prior.py:247-263; the x20 variant is value_at_x20_grids
                   'rays_per_step': n_rays, 'rays_per_step_per_gpu': (n_rays + n_gpus - 1) // n_gpus, 'samples_per_ray': S,
                   'tsdf_voxels': list(scene.tsdf_volume.shape[2:]),
                   'grid_high': list(scene.c['grid_high'].shape[2:])},
        'source_hash': source_hash(),
    }

    # ---- --full only, from here to the result line: every leg beyond the headline ---------------------------
    if args.full and n_gpus > 1:
        # the round-1..4 headline, kept beside the sharded one: one whole frame PER RANK (its own pose), no data-path collective
        el_w, _ = timed_loop(frame_step, max(2, min(args.steps, 5)), 1)
        result['weak'] = {'value': n_gpus * n_rays * max(2, min(args.steps, 5)) / el_w, 'unit': 'rays/s', 'n_gpus': n_gpus, 'scaling': 'weak',
                          'ms_per_step': el_w / max(2, min(args.steps, 5)) * 1e3,
                          'workload': 'one whole 640x480 frame per rank per step (one pose per rank), no data-path collective'}
    elif args.full and rank == 0 and not args.no_shard_model:
        try:
            result['config']['shard_model'] = shard_model(rend, dec, scene, tsdf_bnds, c2w, gt_depth, dev, n_rays, ms_per_step)
            result['config']['k8_speedup_bound_incl_gather'] = result['config']['shard_model']['k8']['speedup_bound_incl_gather']
        except Exception as e:
            result['config']['shard_model'] = {'error': repr(e)[:300]}

    # ---- legs every rank takes part in ---------------------------------------------------------------------
    if args.full and not args.no_extra:
        own_group = False
        # RCCL prints its version banner on C-level stdout when the first communicator comes up: keep stdout = the ONE
        # JSON line by pointing fd 1 at stderr for the duration of these legs (and flushing libc's buffer before it returns)
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            if dist is None:                       # single process: a world of one rank, so that the RCCL path runs here too
                import torch.distributed as dist1
                os.environ['MASTER_ADDR'] = '127.0.0.1'
                os.environ['MASTER_PORT'] = str(free_port())
                dist1.init_process_group('nccl', rank=0, world_size=1, device_id=dev)
                own_group = True
                dd = dist1
            else:
                dd = dist
            legs = dist_legs(dd, A, synthetic, rend, dec, scene, tsdf_bnds, dev, args)
        except Exception as e:                      # extra information, never the reason a bench fails
            legs = {'dist_legs_error': repr(e)[:300]}
        finally:
            if own_group:
                try:
                    dist1.destroy_process_group()
                except Exception:
                    pass
            try:
                C.CDLL(None).fflush(None)
            except Exception:
                pass
            os.dup2(saved_fd, 1)
            os.close(saved_fd)
        if rank == 0:
            result.update(legs)

    # ---- rank-0 legs -----------------------------------------------------------------------------------------
    if args.full and rank == 0 and not args.no_stage_timing:
        result.update(stage_timing(L, _lib, rend, dec, scene, tsdf_bnds, c2w, gt_depth, dev, NS, NF))
    if args.full and rank == 0 and n_gpus == 1 and not args.no_extra:
        if os.environ.get('ADFP_MATH', 'f16x3') == 'f16x3':
            # the same frame with every product on the exact f32-input MFMA (ADFP_MATH=f32), for reference:
            # the f16x3 split reproduces f32 products to 2^-22, this is the bit-exact mode
            os.environ['ADFP_MATH'] = 'f32'
            try:
                for _ in range(2):
                    step()
                torch.cuda.synchronize(dev)
                ts = []
                for _ in range(5):                 # each step timed on its own, the median reported: three steps in one bracket once
                    t1 = time.perf_counter()       # came out at 31.6 ms per step where every other run has 13.4 (one stalled step)
                    out32 = step()
                    torch.cuda.synchronize(dev)
                    ts.append(time.perf_counter() - t1)
                dt = sorted(ts)[len(ts) // 2]
            finally:
                os.environ['ADFP_MATH'] = 'f16x3'
            result['value_f32'] = n_rays / dt          # the headline workload with exact f32-input MFMA everywhere (ADFP_MATH=f32)
            result['exact_f32_mode'] = {
                'value': n_rays / dt, 'unit': 'rays/s', 'ms_per_step': dt * 1e3, 'n_gpus': 1,
                'max_abs_diff_color_vs_default_mode': float((out32[2] - color_img).abs().max()),
                'max_rel_diff_depth_vs_default_mode': float(((out32[0] - depth_img).abs() / depth_img.abs().clamp_min(1e-3)).max())}
        # the same frame with the grids multiplied (x 20, high x 100 more: the scene rounds 1-5 ran the headline on, where occupancy /
        # attention weights / colour vary along a ray): backs the statement that kernel time does not depend on the feature values,
        # and holds the timed path to the oracle where the values are not almost constant
        try:
            result['x20_grids'] = x20_leg(A, synthetic, rend, dec, sd, scene, tsdf_bnds, c2w, gt_depth, dev, NS, NF, args, min(4000, args.cpu_rays))
        except Exception as e:
            result['x20_grids'] = {'error': repr(e)[:200]}
        # sustained: the same loop for >= 2 s (the contract's 10-20 steps are ~0.1 s of GPU time)
        n_sus = max(50, int(2.2 / (ms_per_step * 1e-3)))
        el, _ = timed_loop(step, n_sus, 0)
        result['sustained'] = {'value': n_rays * n_sus / el, 'unit': 'rays/s', 'steps': n_sus, 'seconds': el,
                               'ms_per_step': el / n_sus * 1e3}
        result['sustained']['note'] = 'the sanity bound of `value`: the same step for >= 2 s, insensitive to clock ramp and launch jitter'
        import bench_extra as BX
        for name, leg in (('torch_gpu_baseline', lambda: torch_gpu_leg(rend, dec, sd, scene, tsdf_bnds, c2w, gt_depth, dev, NS, NF)),
                          ('config5', lambda: config5_leg(A, synthetic, _lib, L, dev)),
                          ('config1', lambda: BX.config1_leg(A, synthetic, scene, sd, dec, dev)),
                          ('tracker_iteration', lambda: BX.tracker_leg(A, synthetic, scene, sd, dec, dev)),
                          ('mesher_query', lambda: BX.mesher_leg(A, synthetic, scene, sd, dec, dev)),
                          ('tsdf_fusion', lambda: BX.fusion_leg(synthetic, scene, dev)),
                          ('replica_native_frame', lambda: BX.replica_native_leg(A, synthetic, scene, dec, dev)),
                          ('config3', lambda: BX.config3_leg(dev)),
                          ('allreduce_model', lambda: BX.allreduce_model(scene))):
            try:
                result[name] = leg()
            except Exception as e:
                result[name] = {'error': repr(e)[:300]}
    if args.full and rank == 0 and n_gpus == 1 and args.cpu_rays > 0:
        result.update(cpu_leg(rend, dec, sd, scene, tsdf_bnds, c2w, gt_depth, depth_img, color_img, dev, NS, NF, args.cpu_rays))
    if rank == 0:
        # the evidence a reader of the line needs, inside the objects the driver's record keeps whole (`config`, `roofline`)
        # -- as SCALARS directly under `config`: the driver's record drops dict-valued keys
        cfgd = result['config']
        if 'value_f32' in result:
            cfgd['exact_f32_value'] = result['value_f32']
        if 'parity_vs_oracle' in result:
            pv = result['parity_vs_oracle']
            cfgd['parity_max_rel_depth'], cfgd['parity_max_rel_color'], cfgd['parity_rays'] = pv['max_rel_depth'], pv['max_rel_color'], pv['rays']
            cfgd['parity_psnr_color_db'], cfgd['parity_psnr_depth_db'] = pv['psnr_color_db'], pv['psnr_depth_db']
        xg = result.get('x20_grids')
        if isinstance(xg, dict) and 'value' in xg:
            cfgd['value_at_x20_grids'] = xg['value']
            for k in ('parity_max_rel_depth', 'parity_max_rel_color'):
                if k in xg:
                    cfgd[k + '_at_x20'] = xg[k]
        tg = result.get('torch_gpu_baseline')
        if isinstance(tg, dict) and 'speedup' in tg:
            cfgd['speedup_vs_torch_gpu'] = tg['speedup']
        if 'in_band_fraction' in result:
            cfgd['in_band_fraction'] = result['in_band_fraction']
        rn = result.get('replica_native_frame')
        if isinstance(rn, dict) and 'rays_per_s' in rn:
            cfgd['replica_native_rays_per_s'], cfgd['replica_native_ms_per_frame'] = rn['rays_per_s'], rn['ms_per_frame']
        c3 = result.get('config3')
        if isinstance(c3, dict) and 'ms_per_iteration' in c3:
            cfgd['config3_ms_per_iteration'] = c3['ms_per_iteration']
        print(json.dumps(result))
        sys.stdout.flush()
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


# ----------------------------------------------------------------------------------------------------------
def x20_leg(A, synthetic, rend, dec, sd, scene, tsdf_bnds, c2w, gt_depth, dev, NS, NF, args, n_cpu):
    """The headline frame on the x20 grids (X20_STD_SCALE / X20_HIGH_EXTRA): rays/s over args.steps steps with the headline's cache
    clearing, and the parity of THAT timed output against the oracle on n_cpu evenly strided rays (0 = timing only)."""
    import torch
    H, W = scene.H, scene.W
    n_rays = H * W
    sx = synthetic.Scene(args.scene, H=H, W=W, device=dev, grid_std_scale=X20_STD_SCALE)
    sx.c['grid_high'] = sx.c['grid_high'] * X20_HIGH_EXTRA

    def step():
        rend._engine._grid_cache.clear()
        dec._packed.clear()
        return rend.render_img(sx.c, dec, c2w, dev, scene.tsdf_volume, tsdf_bnds, 'color', gt_depth=gt_depth)
    for _ in range(2):
        step()
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t1) / args.steps
    res = {'value': n_rays / dt, 'unit': 'rays/s', 'ms_per_step': dt * 1e3, 'steps': args.steps,
           'grids': f'the reference init x {X20_STD_SCALE:g}, high grid x {X20_HIGH_EXTRA:g} more (N(0, 0.2) everywhere)'}
    if n_cpu > 0:
        from oracle import adfp_oracle as O
        from attentive_dfprior_amd.common import get_rays
        ro, rd = get_rays(H, W, scene.fx, scene.fy, scene.cx, scene.cy, c2w, dev)
        pick = torch.arange(0, n_rays, max(1, n_rays // n_cpu), device=dev)[:n_cpu]
        bsz = rend.ray_batch_size
        gflat = gt_depth.reshape(-1)
        c_cpu = {k: v.cpu() for k, v in sx.c.items()}
        tsdf_cpu = scene.tsdf_volume.cpu()
        od = torch.empty(len(pick), dtype=torch.float64)
        oc = torch.empty(len(pick), 3)
        batch_of = (pick // bsz).cpu()
        with torch.no_grad():
            for b in range((n_rays + bsz - 1) // bsz):
                idx = torch.nonzero(batch_of == b).reshape(-1)
                if idx.numel():
                    sel = pick[idx.to(dev)]
                    a, _, cc, _ = O.render_batch_ray(sd, c_cpu, rd.reshape(-1, 3)[sel].cpu(), ro.reshape(-1, 3)[sel].cpu(), tsdf_cpu, scene.tsdf_bnds,
                                                     scene.bound, 'color', gflat[sel].cpu(), NS, NF, depth_max=gflat[b * bsz:(b + 1) * bsz].max().cpu())
                    od[idx], oc[idx] = a, cc
        d, c = out[0].reshape(-1)[pick].cpu(), out[2].reshape(-1, 3)[pick].cpu()
        res['parity_max_rel_depth'] = float((d - od).abs().max() / od.abs().max())
        res['parity_max_rel_color'] = float((c - oc).abs().max() / oc.abs().max())
        res['parity_rays'] = len(pick)
    return res


# ----------------------------------------------------------------------------------------------------------
XGMI_LINK_GBPS, RING_HOP_US = 153.0, 5.0       # MI355X_MICROARCH.md: one xGMI link, per direction; a hop's launch / link latency (bench_extra.allreduce_model)


def allgather_model_ms(nbytes, k):
    """Ring all-gather of `nbytes` in total over k GPUs: (k-1) steps, each moving nbytes / k over ONE xGMI link, + a hop latency per step
    (the form of bench_extra.allreduce_model, without the reduce-scatter half)."""
    return ((k - 1) / k * nbytes / (XGMI_LINK_GBPS * 1e9) + (k - 1) * RING_HOP_US * 1e-6) * 1e3


def shard_model(rend, dec, scene, tsdf_bnds, c2w, gt_depth, dev, n_rays, headline_ms, steps=10, reps=3):
    """What ONE GPU says about the ray-sharded frame at N = 2 / 4 / 8 (no multi-GPU node needed), measured THE WAY THE HEADLINE IS: every
    1/k shard of the headline frame through Renderer.render_img_shard -- the call a rank of dist.render_img_sharded makes -- `steps`
    steps back to back with the headline step's cache clearing (the grid re-layouts and weight-image packs every rank repeats) and ONE
    synchronisation at the end; median of `reps` such runs.  A k-GPU step takes at least the slowest shard + the all-gather of 28 B
    per ray, which is MODELLED (ring over xGMI, allgather_model_ms) because it cannot be measured here:
        speedup_bound_incl_gather(N = k) = headline ms_per_step / (max_r t(shard r of k) + t_gather(k))
    The numerator is the headline's own ms_per_step (what a SCALE run divides by), not a separately synchronised k = 1 call."""
    import torch
    from attentive_dfprior_amd import dist as adist

    def t_shard(lo, hi):
        def step():
            rend._engine._grid_cache.clear()
            dec._packed.clear()
            rend.render_img_shard(scene.c, dec, c2w, dev, scene.tsdf_volume, tsdf_bnds, 'color', gt_depth, lo, hi)
        ts = []
        for it in range(reps):
            step()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) / steps)
        return sorted(ts)[len(ts) // 2]

    nbytes = n_rays * 28
    out = {'unit': 'ms', 'steps': steps, 'reps': reps, 'headline_ms_per_step': headline_ms,
           'what': 'pipelined time per step of Renderer.render_img_shard for every shard of the headline frame: `steps` steps back to back, caches '
                   'cleared as in the headline step, one synchronisation; median of `reps` runs',
           'allgather_bytes': nbytes,
           'allgather_model': f't = (k-1)/k x bytes / {XGMI_LINK_GBPS:g} GB/s (ring, one xGMI link per neighbour) + (k-1) x {RING_HOP_US:g} us; MODELLED, not measured'}
    out['k1'] = {'ms': t_shard(0, n_rays) * 1e3}
    for k in (2, 4, 8):
        ts = [t_shard(*adist.shard_range(n_rays, r, k)) for r in range(k)]
        g = allgather_model_ms(nbytes, k)
        out[f'k{k}'] = {'ms_slowest_shard': max(ts) * 1e3, 'ms_fastest_shard': min(ts) * 1e3, 'ms_allgather_model': g,
                        'speedup_bound': headline_ms / (max(ts) * 1e3), 'speedup_bound_incl_gather': headline_ms / (max(ts) * 1e3 + g),
                        'efficiency_bound_incl_gather': headline_ms / (max(ts) * 1e3 + g) / k}
    out['fixed_cost_ms'] = t_shard(0, 0) * 1e3
    out['fixed_cost_what'] = 'an EMPTY shard (host-side cost of a call that launches nothing)'
    out['north_star_target'] = '>= 6x at 8 GPUs'
    b8 = out['k8']['speedup_bound_incl_gather']
    out['verdict'] = (f'reachable on this frame: {b8:.2f}x at 8 GPUs incl. the modelled all-gather' if b8 >= 6.0 else
                      f'NOT reachable on a 640x480 x 64 frame (5 ms of work): {b8:.2f}x at 8 GPUs incl. the modelled all-gather -- the per-rank fixed '
                      'costs and the gather cap the speed-up below 6x; config 5 (1 M rays x 128 samples, ~35 ms per GPU at 8 GPUs) is the '
                      'configuration where it is')
    return out


# ----------------------------------------------------------------------------------------------------------
def dist_legs(dist, A, synthetic, rend, dec, scene, tsdf_bnds, dev, args):
    """`strong` and `train_allreduce` (module docstring).  Every rank runs this; timing = barrier + synchronize on
    both sides, max over ranks."""
    import torch
    from attentive_dfprior_amd import dist as adist, mapping
    from attentive_dfprior_amd.common import get_rays
    world, rank = dist.get_world_size(), dist.get_rank()
    out = {}

    def barrier():
        torch.cuda.synchronize(dev)
        dist.barrier()
        torch.cuda.synchronize(dev)

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        barrier()
        t0 = time.perf_counter()
        for _ in range(steps):
            r = fn()
        barrier()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item()) / steps, r

    one = torch.ones(1, device=dev)
    dist.all_reduce(one)
    out['rccl'] = {'backend': dist.get_backend(), 'world_size': world, 'allreduce_of_ones': float(one.item())}

    # ---- strong: ONE frame, contiguous ray slices, full-batch depth max, outputs all-gathered (28 B/ray)
    c2w = scene.default_c2w(yaw=0.3, pitch=-0.1)
    gd = scene.depth_image(c2w).reshape(-1)
    ro, rd = get_rays(scene.H, scene.W, scene.fx, scene.fy, scene.cx, scene.cy, c2w, dev)
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    n = ro.shape[0]

    def render_fn(o, d, z, m):
        return rend.render_batch_ray(scene.c, dec, d, o, dev, scene.tsdf_volume, tsdf_bnds, 'color', z, depth_max=m)[:3]

    def strong_step():
        with torch.no_grad():
            return adist.render_rays_sharded(render_fn, ro, rd, gd, gather=True)
    t_strong, frame = timed(strong_step, max(5, args.steps), 2)
    assert frame[0].shape[0] == n and torch.isfinite(frame[0]).all()
    out['strong'] = {'value': n / t_strong, 'unit': 'rays/s', 'n_gpus': world, 'scaling': 'strong', 'ms_per_frame': t_strong * 1e3,
                     'workload': 'ONE 640x480 x 64-sample frame as a single ray batch, rank r renders the contiguous slice '
                                 '[r N/world, (r+1) N/world) with the full-batch depth max, depth/uncertainty/colour all-gathered '
                                 '(28 B/ray) inside the timed region',
                     'allgather_bytes': n * 28}

    # ---- train_allreduce: one 5 000-ray Mapper iteration (stage color), rays sharded, ONE flat gradient all-reduce
    n_train = 5000
    g = torch.Generator().manual_seed(1)
    pick = torch.randint(n, (n_train,), generator=g).to(dev)
    lo, hi = adist.shard_range(n_train, rank, world)
    tro, trd, tgd = ro[pick][lo:hi].contiguous(), rd[pick][lo:hi].contiguous(), gd[pick][lo:hi].contiguous()
    tgc = torch.rand(n_train, 3, generator=g).to(dev)[lo:hi]
    dmax = gd[pick].max().reshape(1)
    frozen = list(dec.low_decoder.parameters()) + list(dec.high_decoder.parameters())
    for p in frozen:
        p.requires_grad_(False)                          # low is never optimised, fix_high: True (src/Mapper.py:364-371)
    params = list(dec.color_decoder.parameters()) + list(dec.mlp.parameters())
    params_before = [p.detach().clone() for p in params]           # the later legs compare against the seeded weights
    grids = {k: v.detach().clone().requires_grad_(True) for k, v in scene.c.items()}
    masks = {k: mapping.frustum_mask(c2w, tuple(v.shape[2:]), gd.reshape(scene.H, scene.W), scene.bound, scene.H, scene.W,
                                     scene.fx, scene.fy, scene.cx, scene.cy) for k, v in grids.items()}
    opt = torch.optim.Adam(params, lr=0.005)
    buckets = {'dense': None, 'frustum_masked': adist.MaskedGradBucket(grids, masks, extra=params)}
    res = {}
    try:
        for mode in ('dense', 'frustum_masked'):
            opt_g = mapping.MaskedGridAdam(grids, masks if mode == 'frustum_masked' else None)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

            def it():
                opt.zero_grad()
                opt_g.zero_grad()
                d, u, col, w = rend.render_batch_ray(grids, dec, trd, tro, dev, scene.tsdf_volume, tsdf_bnds, 'color', tgd, depth_max=dmax)
                m = tgd > 0
                (torch.abs(tgd[m] - d[m]).sum() + 0.2 * torch.abs(tgc - col).sum()).backward()
                ev[0].record()
                if mode == 'dense':
                    nbytes = adist.allreduce_grads(list(grids.values()) + params, skip_single=False)
                else:
                    buckets[mode].allreduce(skip_single=False)
                    nbytes = buckets[mode].numel() * 4
                ev[1].record()
                opt.step()
                opt_g.step({'grid_low': 0.005, 'grid_high': 0.005, 'grid_color': 0.005})
                return nbytes
            t_it, nbytes = timed(it, 20, 3)
            torch.cuda.synchronize(dev)
            # the collective alone (pack + all-reduce + unpack), HIP events on the launch stream, last iteration
            res[mode] = {'ms_per_iteration': t_it * 1e3, 'rays_per_s': n_train / t_it, 'bucket_bytes': int(nbytes),
                         'allreduce_ms_incl_pack_unpack': ev[0].elapsed_time(ev[1])}
        # the same iteration as ONE device-side call (mapping.MapperIteration, distributed mode): keep-mask pre-filter, loss and
        # backward without autograd, the gradients written straight into one contiguous bucket that is all-reduced as it stands,
        # Adam with device-side step state
        import copy
        dec_f = copy.deepcopy(dec)
        cf = {k: v.detach().clone() for k, v in scene.c.items()}
        lrs = {'color': dict(low=0.005, high=0.005, color=0.005, decoders=0.005, mlp=0.005)}
        for mode in ('dense', 'frustum_masked'):
            itf = mapping.MapperIteration(rend, dec_f, cf, masks if mode == 'frustum_masked' else None, scene.tsdf_volume, tsdf_bnds, lrs,
                                          use_graph=False, distributed=True)
            t_it, _ = timed(lambda: itf.step(tro, trd, tgd, tgc, 'color'), 20, 3)
            res['fused_' + mode] = {'ms_per_iteration': t_it * 1e3, 'rays_per_s': n_train / t_it, 'bucket_bytes': int(itf.bucket_bytes),
                                    'note': 'the bucket is dense either way (zero-copy: the backward writes into it); the mask only restricts Adam'}
    finally:
        with torch.no_grad():
            for p, p0 in zip(params, params_before):
                p.copy_(p0)                                          # bumps _version: the packed images are rebuilt
        for p in dec.parameters():
            p.grad = None
        for p in frozen:
            p.requires_grad_(True)
    out['train_allreduce'] = {'rays_per_iteration': n_train, 'rays_per_rank': hi - lo, 'n_gpus': world, 'stage': 'color',
                              'samples_per_ray': 64, **res,
                              'note': 'render forward + Mapper loss + backward on the rank\'s ray shard, ONE flat-bucket all-reduce (SUM, '
                                      'fp32) of the three grids\' dense gradients + the trainable decoder parameters, then Adam on every '
                                      'rank; frustum_masked = the bucket restricted to the frustum-selected voxels (SURVEY.md section 8e)'}
    return out


# ----------------------------------------------------------------------------------------------------------
def stage_timing(L, _lib, rend, dec, scene, tsdf_bnds, c2w, gt_depth, dev, NS, NF, reps=5):
    """HIP-event time of the individual kernels, each launched alone on torch's current stream
    (the stream the library launches on), over EXACTLY the launch mix of one frame -- since round 3 ONE
    launch per kernel for the whole 307 200-ray frame (render_img carries the reference's 100 000-ray
    batches as depth-max segments) -- so that the average launch duration equals what
    `rocprofv3 --kernel-trace --stats` reports for the same command."""
    import torch
    from attentive_dfprior_amd.common import get_rays
    eng = rend._engine
    S = NS + NF
    ro_all, rd_all = get_rays(scene.H, scene.W, scene.fx, scene.fy, scene.cx, scene.cy, c2w, dev)
    ro_all, rd_all, gd_all = ro_all.reshape(-1, 3), rd_all.reshape(-1, 3), gt_depth.reshape(-1)
    sc, keep = eng.scene(dec, scene.c, scene.tsdf_volume, tsdf_bnds, scene.bound, 'color', images='hg')
    batches, n_band, n_pts = [], 0, 0
    # the launch structure of render_img: ONE call for the whole frame, the reference's ray batches carried as depth-max segments
    # (a frame too large for one call would fall back to the batch loop)
    nseg = (ro_all.shape[0] + rend.ray_batch_size - 1) // rend.ray_batch_size
    one_call = nseg <= 48 and ro_all.shape[0] * S < 2 ** 31
    step_rays = ro_all.shape[0] if one_call else rend.ray_batch_size
    seg = rend.ray_batch_size if one_call else 0
    for i in range(0, ro_all.shape[0], step_rays):
        ro = ro_all[i:i + step_rays].contiguous()
        rd = rd_all[i:i + step_rays].contiguous()
        gd = gd_all[i:i + step_rays].contiguous()
        with torch.no_grad():
            d, u, c, w, aux = eng.render_forward(dec, scene.c, ro, rd, gd, scene.tsdf_volume, tsdf_bnds, scene.bound,
                                                 'color', NS, NF, want_aux=True, depth_max_segment=seg)
        P = ro.shape[0] * S
        n_band += int((w != 1).sum())
        n_pts += P
        ap = _lib.AdfpPoints()
        ap.mode = _lib.PTS_RAYS
        ap.n_points = P
        ap.rays_o, ap.rays_d, ap.z_vals, ap.S = ro.data_ptr(), rd.data_ptr(), aux['z_vals'].data_ptr(), S
        batches.append((ap, ro, rd, gd, aux['z_vals']))
    Pmax = max(b[0].n_points for b in batches)
    raw = torch.empty((Pmax, 4), dtype=torch.float32, device=dev)
    wbuf = torch.empty((Pmax,), dtype=torch.float32, device=dev)
    flags = torch.empty((Pmax,), dtype=torch.uint8, device=dev)
    lst = torch.empty((Pmax,), dtype=torch.int32, device=dev)
    attu = torch.empty((Pmax,), dtype=torch.float32, device=dev)
    cnt = torch.zeros((4,), dtype=torch.int32, device=dev)
    tile_cnt = torch.zeros((1,), dtype=torch.int32, device=dev)      # the fused launch's chip-wide tile counter (in the frame: a word of the workspace)
    st = _lib.current_stream(dev)
    band_frac = n_band / n_pts
    nl = len(batches)

    def timed(fn):
        """average duration of ONE launch (s) over reps x the frame's launch mix"""
        for b in batches:
            fn(b)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            for b in batches:
                fn(b)
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / (reps * nl) * 1e-3

    t_color = timed(lambda b: _lib.check(L.adfp_decode_stage(C.byref(sc), C.byref(b[0]), 2, _lib.ptr(raw), _lib.ptr(wbuf), _lib.ptr(tile_cnt), st), 'decode'))
    t_low = timed(lambda b: _lib.check(L.adfp_decode_stage(C.byref(sc), C.byref(b[0]), 0, _lib.ptr(raw), _lib.ptr(wbuf), _lib.ptr(tile_cnt), st), 'decode'))
    # the launch stage color actually uses in the default mode: low + colour decoder fused (k_decode_lc)
    t_lc = timed(lambda b: _lib.check(L.adfp_decode_stage(C.byref(sc), C.byref(b[0]), 3, _lib.ptr(raw), _lib.ptr(wbuf), _lib.ptr(tile_cnt), st), 'decode')) \
        if sc.h_low and sc.h_color else None
    t_tsdf = timed(lambda b: _lib.check(L.adfp_tsdf_stage(C.byref(sc), C.byref(b[0]), _lib.ptr(flags), _lib.ptr(lst), _lib.ptr(attu),
                                                          None, _lib.ptr(cnt), st), 'tsdf'))
    t_all = timed(lambda b: eng.render_forward(dec, scene.c, b[1], b[2], b[3], scene.tsdf_volume, tsdf_bnds, scene.bound,
                                               'color', NS, NF, depth_max_segment=seg))
    pts_per_launch = n_pts / nl
    fl_color = 2.0 * MAC_COLOR * pts_per_launch
    ach = fl_color / t_color / 1e12
    by = float(TSDF_BYTES_PER_SAMPLE) * pts_per_launch
    useful = 2.0 * (MAC_LOW + MAC_COLOR + band_frac * (MAC_HIGH + MAC_ATT)) * pts_per_launch
    from attentive_dfprior_amd.engine import math_mode
    if math_mode() == 'f32':
        roof = {'kernel': 'k_decode<32,4,COLOR> (colour decoder, exact f32-input MFMA)', 'bound': 'mfma',
                'achieved': ach, 'peak': PEAK_F32_MFMA_TFLOPS, 'unit': 'TFLOP/s', 'frac': ach / PEAK_F32_MFMA_TFLOPS,
                'frac_algorithmic': ach / PEAK_F32_MFMA_TFLOPS, 'traffic': None}
    else:
        # dominant kernel of the default mode: the fused low + colour launch (2 x 90 f16 MFMAs per 32-point tile)
        fl_color = 2.0 * (MAC_LOW + MAC_COLOR) * pts_per_launch
        # a network latched to its exact image (f16-range event) has no fused launch: the stage is then the two decoders in turn
        t_color_alone, t_color = t_color, (t_lc if t_lc else t_color + t_low)
        ach = fl_color / t_color / 1e12
        ex = 2.0 * F16X3_FLOP_COLOR * pts_per_launch / t_color / 1e12
        roof = {'kernel': 'k_decode_lc16<768> (low + colour decoder in one launch, v_mfma_f32_16x16x32_f16 with 3-product f32 operand split)',
                'bound': 'mfma', 'achieved': ach, 'peak': PEAK_F16_MFMA_TFLOPS, 'unit': 'TFLOP/s',
                'frac': ach / PEAK_F16_MFMA_TFLOPS, 'frac_algorithmic': ach / PEAK_F16_MFMA_TFLOPS,
                'executed_tflops': ex, 'frac_executed': ex / PEAK_F16_MFMA_TFLOPS, 'traffic': None,
                'note': 'achieved / frac = ALGORITHMIC FLOP (2 x (15 479 + 15 575) per sample, SURVEY.md section 8d) per launch / the '
                        'kernel\'s average launch duration, against the dense-f16 MFMA peak -- the pipe the kernel executes on; '
                        'executed_tflops / frac_executed = the f16 MFMA FLOP actually issued (3 products per f32 product + K padding = '
                        '2.97 x algorithmic); algorithmic_f32_tflops / frac_of_f32_mfma_peak = the same algorithmic FLOP against the '
                        'f32-input MFMA peak the exact mode is bound by',
                'algorithmic_f32_tflops': ach, 'f32_mfma_peak_tflops': PEAK_F32_MFMA_TFLOPS,
                'frac_of_f32_mfma_peak': ach / PEAK_F32_MFMA_TFLOPS}
    kname = 'void k_decode<32, 4, 2' if math_mode() == 'f32' else 'void k_decode_lc16<'
    roof['traffic'], prov = pmc_traffic(kname, pts_per_launch)
    roof['traffic_source'] = dict(prov, note='PROFILED bytes/sample (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes) x this run\'s '
                                             'samples per launch; stale = the csv was taken from a different build of the kernels')
    roof.update({'algorithmic_flop_per_launch': fl_color, 'avg_launch_ms': t_color * 1e3, 'launches_per_frame': nl,
                 'points_per_launch': pts_per_launch})
    if math_mode() != 'f32':
        # What actually limits the kernel.  The contract's `bound` offers hbm | mfma and the kernel runs on the MFMA pipe, but its
        # time is the SUM of its MFMA pipe time and its VALU issue time (they do not overlap on this machine: DESIGN.md section 4.1,
        # one product dropped = exactly its pipe cycles saved).  Per 32-point tile (both networks; instruction counts of the
        # compiled kernel, tools/isa_mix.py): 360 MFMAs x 16 pipe cycles + ~2 380 VALU instructions at ~3.3 issue cycles + LDS.
        tiles = pts_per_launch / 32.0
        simds = 256 * 4
        sq = pmc_sq('k_decode_lc16')
        clock = sq.get('clock_ghz') or 2.0
        cyc_per_tile = t_color * clock * 1e9 * simds / tiles
        mix = isa_mix_lc16()
        if 'valu' in mix:
            n_mfma, n_valu, n_lds = mix['mfma'], mix['valu'], mix['lds']
            ceil_cycles = n_mfma * 16 + 2.2 * n_valu
            roof['limiter'] = {
                'what': 'VALU issue + MFMA pipe, additive (not HBM, not the MFMA peak)',
                'per_tile_budget': {'mfma_instructions': n_mfma, 'mfma_pipe_cycles': n_mfma * 16, 'valu_instructions': n_valu,
                                    'lds_instructions': n_lds, 'source': 'the TILE LOOP of the compiled k_decode_lc16 (tools/gen_isa_mix.py: tools/isa_mix.py --loop)',
                                    'file': mix['file'], 'profiled_source_hash': mix['profiled_source_hash'], 'this_source_hash': mix['this_source_hash'],
                                    'stale': mix['stale']},
                'simd_cycles_per_tile': cyc_per_tile, 'clock_ghz_used': clock,
                'mfma_pipe_frac': n_mfma * 16 / cyc_per_tile,
                'valu_issue_frac': 1.0 - n_mfma * 16 / cyc_per_tile,
                'valu_issue_cycles_per_instruction': (cyc_per_tile - n_mfma * 16) / n_valu,
                'ceiling': f'with the {n_valu} VALU instructions of the tile loop at the 2.2-cycle full-rate floor and the {n_mfma} MFMAs (16 pipe cycles each) on '
                           f'top the tile would take {ceil_cycles:.0f} cycles: frac_of_that_ceiling',
                'frac_of_that_ceiling': ceil_cycles / cyc_per_tile,
                'pmc': sq}
        else:
            roof['limiter'] = {'error': 'profiles/r06_isa_mix_lc16.txt missing or unreadable (python tools/gen_isa_mix.py)', 'pmc': sq,
                               'valu_issue_frac': None}
        roof['valu_issue_frac'] = roof['limiter']['valu_issue_frac']
        roof['in_band_fraction'] = band_frac
    tsdf_traffic, _ = pmc_traffic('k_tsdf', pts_per_launch)
    return {
        'roofline': roof,
        'roofline_tsdf': {'kernel': 'k_tsdf (TSDF trilerp + band mask + compaction), room0: the 785 MB volume is mostly cache-resident '
                                    'along the frame\'s frustum; config5.roofline_tsdf is the streaming case',
                          'bound': 'hbm', 'achieved': by / t_tsdf / 1e9, 'peak': PEAK_HBM_GBPS, 'unit': 'GB/s',
                          'frac': by / t_tsdf / 1e9 / PEAK_HBM_GBPS, 'traffic': tsdf_traffic,
                          'real_hbm_gbps': (tsdf_traffic / t_tsdf / 1e9) if tsdf_traffic else None,
                          'bytes_per_launch': by, 'avg_launch_ms': t_tsdf * 1e3},
        'stage_avg_launch_ms': {'low_color_decoder_fused': (t_lc * 1e3) if t_lc else None,
                                'color_decoder_alone': (t_color_alone if math_mode() != 'f32' else t_color) * 1e3,
                                'low_decoder_alone': t_low * 1e3, 'tsdf': t_tsdf * 1e3, 'whole_render_batch_ray': t_all * 1e3},
        'in_band_fraction': band_frac,
        'useful_tflops_whole_frame': useful / t_all / 1e12,
    }


def config5_leg(A, synthetic, _lib, L, dev, n_rays=131072, NS=96, NF=32):
    """BASELINE.json configs[4] at one GPU's share: 16 m cube, 1024^3 TSDF (4.3 GB: beyond L2 and the Infinity Cache),
    128 samples/ray, rays of 8 poses.  Whole render_batch_ray rays/s and the trilerp stage alone."""
    import torch
    from attentive_dfprior_amd.common import get_rays
    sc = synthetic.Scene('cube16', device=dev, grid_std_scale=20.0, voxel=16.0 / 1024, inset=2.0)
    sc.c['grid_high'] = sc.c['grid_high'] * 100
    dec = A.DF()
    dec.load_state_dict(synthetic.seeded_state_dict(0))
    dec.bound = sc.bound
    dec = dec.to(dev)
    cfg = {'rendering': {'lindisp': False, 'perturb': 0.0, 'N_samples': NS, 'N_surface': NF, 'N_importance': 0},
           'scale': 1, 'occupancy': True, 'meshing': {'resolution': 256}}
    rend = A.Renderer(cfg, None, sc, ray_batch_size=n_rays)
    tb = sc.tsdf_bnds.to(dev)
    S = NS + NF
    eng = rend._engine
    P = n_rays * S
    flags = torch.empty((P,), dtype=torch.uint8, device=dev)
    lst = torch.empty((P,), dtype=torch.int32, device=dev)
    attu = torch.empty((P,), dtype=torch.float32, device=dev)
    cnt = torch.zeros((4,), dtype=torch.int32, device=dev)
    st = _lib.current_stream(dev)

    def ev_time(fn, reps):
        fn()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1) / reps * 1e-3

    def measure(order):
        """order 'pixel': every pose contributes a contiguous run of pixels (what render_img feeds: neighbouring rays are
        neighbouring pixels); 'random': a random subset of each image (no coherence between consecutive rays)."""
        g = torch.Generator().manual_seed(0)
        ros, rds, gds = [], [], []
        per = n_rays // 8
        for k in range(8):
            c2w = sc.default_c2w(offset=(0.5 * k - 2, 0.3 * k - 1, 0.2 * k), yaw=0.7 * k, pitch=-0.2 + 0.05 * k)
            gd = sc.depth_image(c2w)
            ro, rd = get_rays(sc.H, sc.W, sc.fx, sc.fy, sc.cx, sc.cy, c2w, dev)
            if order == 'random':
                pick = torch.randperm(sc.H * sc.W, generator=g)[:per].to(dev)
            else:
                start = (sc.H * sc.W - per) // 2
                pick = torch.arange(start, start + per, device=dev)
            ros.append(ro.reshape(-1, 3)[pick]); rds.append(rd.reshape(-1, 3)[pick]); gds.append(gd.reshape(-1)[pick])
        ro, rd, gd = torch.cat(ros).contiguous(), torch.cat(rds).contiguous(), torch.cat(gds).contiguous()

        def whole():
            with torch.no_grad():
                return eng.render_forward(dec, sc.c, ro, rd, gd, sc.tsdf_volume, tb, sc.bound, 'color', NS, NF, want_aux=True)
        d, u, c, w, aux = whole()
        assert torch.isfinite(d).all() and torch.isfinite(c).all()
        scn, keep = eng.scene(dec, sc.c, sc.tsdf_volume, tb, sc.bound, 'color')
        ap = _lib.AdfpPoints()
        ap.mode, ap.n_points = _lib.PTS_RAYS, P
        ap.rays_o, ap.rays_d, ap.z_vals, ap.S = ro.data_ptr(), rd.data_ptr(), aux['z_vals'].data_ptr(), S
        t_all = ev_time(whole, 5)

        def tsdf_time(scene_desc, pts):
            return ev_time(lambda: _lib.check(L.adfp_tsdf_stage(C.byref(scene_desc), C.byref(pts), _lib.ptr(flags), _lib.ptr(lst), _lib.ptr(attu),
                                                                None, _lib.ptr(cnt), st), 'tsdf'), 10)
        t_tsdf = tsdf_time(scn, ap)
        extra = None
        if order == 'random':
            # what Renderer.render_batch_ray does with such a batch: the order probe's verdict makes it read the CORNER-BLOCK copy of
            # the volume (Engine.tsdf_blocks), in the caller's order; sorting on top (round 4's answer, Renderer.sort_incoherent) is
            # timed beside it -- the whole call incl. keys, radix sort, gathers and the outputs' way back -- and the TSDF stage alone
            # in the four combinations of (as given | sorted) x (volume as it stands | corner blocks)
            def auto():
                with torch.no_grad():
                    return rend.render_batch_ray(sc.c, dec, rd, ro, dev, sc.tsdf_volume, tb, 'color', gt_depth=gd)
            for _ in range(3):
                auto()
                torch.cuda.synchronize(dev)
            t_auto = ev_time(auto, 5)
            rend.sort_incoherent = True
            for _ in range(2):
                auto()
            t_auto_sorted = ev_time(auto, 5)
            rend.sort_incoherent = 'auto'

            def whole_blocks():
                with torch.no_grad():
                    return eng.render_forward(dec, sc.c, ro, rd, gd, sc.tsdf_volume, tb, sc.bound, 'color', NS, NF, tsdf_blocks=True)
            t_all_blocks = ev_time(whole_blocks, 5)
            scn_b, keep_b = eng.scene(dec, sc.c, sc.tsdf_volume, tb, sc.bound, 'color', tsdf_blocks=True)
            assert scn_b.tsdf.corner_blocks
            perm = rend._coherent_order(ro, rd, gd, sc.tsdf_volume, tb, wait=True)
            assert perm is not None
            ro_s, rd_s, gd_s = ro.index_select(0, perm).contiguous(), rd.index_select(0, perm).contiguous(), gd.index_select(0, perm).contiguous()
            with torch.no_grad():
                aux_s = eng.render_forward(dec, sc.c, ro_s, rd_s, gd_s, sc.tsdf_volume, tb, sc.bound, 'color', NS, NF, want_aux=True)[4]
            ap_s = _lib.AdfpPoints()
            ap_s.mode, ap_s.n_points = _lib.PTS_RAYS, P
            ap_s.rays_o, ap_s.rays_d, ap_s.z_vals, ap_s.S = ro_s.data_ptr(), rd_s.data_ptr(), aux_s['z_vals'].data_ptr(), S
            extra = {'t_auto': t_auto, 't_auto_sorted': t_auto_sorted, 't_all_blocks': t_all_blocks, 'given_blocks': tsdf_time(scn_b, ap), 'sorted_plain': tsdf_time(scn, ap_s),
                     'sorted_blocks': tsdf_time(scn_b, ap_s)}
        return t_all, t_tsdf, float((w != 1).float().mean()), extra
    t_all, t_tsdf, band, _ = measure('pixel')
    t_all_r, t_tsdf_r, band_r, ex = measure('random')
    by = float(TSDF_BYTES_PER_SAMPLE) * P
    traffic, prov = pmc_traffic('k_tsdf', P, 'r05_pmc_hbm_config5.csv')
    gb = lambda t: by / t / 1e9
    return {'workload': '16 m cube, 1024^3 TSDF (4.29 GB), 128 samples/ray (96 + 32), 131 072 rays = 8 poses x 16 384 consecutive pixels '
                        '(render_img order) = one GPU\'s share of BASELINE.json configs[4]', 'value': n_rays / t_all, 'unit': 'rays/s',
            'ms_per_batch': t_all * 1e3, 'in_band_fraction': band,
            'roofline_tsdf': {'kernel': 'k_tsdf', 'bound': 'hbm', 'achieved': gb(t_tsdf), 'peak': PEAK_HBM_GBPS, 'unit': 'GB/s',
                              'frac': gb(t_tsdf) / PEAK_HBM_GBPS, 'traffic': traffic,
                              'real_hbm_gbps': (traffic / t_tsdf / 1e9) if traffic else None,
                              'traffic_source': prov, 'bytes_per_launch': by, 'avg_launch_ms': t_tsdf * 1e3},
            'random_ray_order': {'value': n_rays / ex['t_auto'], 'unit': 'rays/s', 'ms_per_batch': ex['t_auto'] * 1e3, 'in_band_fraction': band_r,
                                 'tsdf_algorithmic_gbps': gb(ex['given_blocks']), 'tsdf_avg_launch_ms': ex['given_blocks'] * 1e3,
                                 'tsdf_frac_of_hbm_peak': gb(ex['given_blocks']) / PEAK_HBM_GBPS,
                                 'as_given': {'value': n_rays / ex['t_all_blocks'], 'ms_per_batch': ex['t_all_blocks'] * 1e3,
                                              'tsdf_algorithmic_gbps': gb(ex['given_blocks']), 'tsdf_avg_launch_ms': ex['given_blocks'] * 1e3,
                                              'tsdf_frac_of_hbm_peak': gb(ex['given_blocks']) / PEAK_HBM_GBPS,
                                              'tsdf_counter_bytes_per_sample': pmc_traffic('k_tsdf', 1, 'r05_pmc_hbm_config5_random.csv')[0]},
                                 'sorted': {'value': n_rays / ex['t_auto_sorted'], 'ms_per_batch': ex['t_auto_sorted'] * 1e3,
                                            'tsdf_algorithmic_gbps': gb(ex['sorted_blocks']), 'tsdf_avg_launch_ms': ex['sorted_blocks'] * 1e3,
                                            'tsdf_frac_of_hbm_peak': gb(ex['sorted_blocks']) / PEAK_HBM_GBPS,
                                            'what': 'Renderer.sort_incoherent = True: the same batch rendered sorted by (origin cell, surface cell) on top of the corner blocks; '
                                                    'value / ms_per_batch include keys, radix sort, gathers and the outputs\' way back'},
                                 'plain_volume': {'what': 'the same batches with the TSDF read as it stands (the round-4 path: four 8-byte column pieces per lookup)',
                                                  'as_given': {'value': n_rays / t_all_r, 'ms_per_batch': t_all_r * 1e3, 'tsdf_algorithmic_gbps': gb(t_tsdf_r),
                                                               'tsdf_avg_launch_ms': t_tsdf_r * 1e3,
                                                               'tsdf_counter_bytes_per_sample': pmc_traffic('k_tsdf', 1, 'r04_pmc_hbm_config5_random.csv', exact=True)[0],
                                                               'tsdf_counter_file': 'profiles/r04_pmc_hbm_config5_random.csv (round 4, the plain volume rendered as given)'},
                                                  'sorted': {'tsdf_algorithmic_gbps': gb(ex['sorted_plain']), 'tsdf_avg_launch_ms': ex['sorted_plain'] * 1e3}},
                                 'tsdf_layout': 'corner blocks: [X][Y][Z][8] float32, one aligned 32-byte piece per trilinear lookup (adfp_relayout_tsdf, 34 GB for this volume, built once)',
                                 'note': 'the same volume and sample count with each pose\'s rays drawn at random from its image: consecutive rays share no '
                                         'cache lines, and in the volume as it stands every 8-corner lookup costs four 64-byte sectors (plain_volume.as_given).  '
                                         'Renderer.render_batch_ray notices the incoherent order of such a batch (adfp_ray_order_probe, no sync) and reads the '
                                         'corner-block copy of the volume, in the caller\'s order: `value` / `ms_per_batch` = that call, tsdf_* = its TSDF stage '
                                         'alone (= as_given; as_given.value is the engine call without the probe); `sorted` = the same with round 4\'s ray sort on top'}}


def torch_gpu_leg(rend, dec, sd, scene, tsdf_bnds, c2w, gt_depth, dev, NS, NF, n=100000):
    """"the same restatement on 1 GPU via PyTorch-ROCm as the reference single-GPU PyTorch
    denominator": the oracle's functions (== the reference's torch ops) on GPU tensors, with Renderer.eval_points'
    500 000-point chunk loop (src/utils/Renderer.py:38), one reference ray batch (100 000 rays x 64 samples)."""
    import torch
    from oracle import adfp_oracle as O
    from attentive_dfprior_amd.common import get_rays
    ro, rd = get_rays(scene.H, scene.W, scene.fx, scene.fy, scene.cx, scene.cy, c2w, dev)
    pick = torch.arange(0, scene.H * scene.W, 3, device=dev)[:n]
    ro, rd, gd = ro.reshape(-1, 3)[pick].contiguous(), rd.reshape(-1, 3)[pick].contiguous(), gt_depth.reshape(-1)[pick].contiguous()
    sd_g = {k: v.to(dev) for k, v in sd.items()}
    bound_g = scene.bound.to(dev)

    def torch_gpu():
        with torch.no_grad():
            z = O.sample_z(ro, rd, gd, bound_g, NS, NF, False, 0.0, None, None)
            N, S = z.shape
            pts = (ro[..., None, :] + rd[..., None, :] * z[..., :, None]).reshape(-1, 3)
            raws = [O.eval_points(sd_g, pts[i:i + 500000], scene.c, scene.tsdf_volume, tsdf_bnds, bound_g, 'color')[0]
                    for i in range(0, pts.shape[0], 500000)]
            return O.raw2outputs(torch.cat(raws).reshape(N, S, 4), z)

    def product():
        with torch.no_grad():
            return rend.render_batch_ray(scene.c, dec, rd, ro, dev, scene.tsdf_volume, tsdf_bnds, 'color', gt_depth=gd)

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(reps):
            o = fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / reps, o
    t_p, (d, u, c, w) = timed(product, 10)
    t_t, (od, ov, oc, _) = timed(torch_gpu, 3)
    return {'value': n / t_t, 'unit': 'rays/s', 'ms_per_100k_ray_batch': t_t * 1e3, 'product_ms_per_100k_ray_batch': t_p * 1e3,
            'product_rays_per_s': n / t_p, 'speedup': t_t / t_p, 'kind': 'port (oracle functions on cuda tensors through PyTorch-ROCm)',
            'max_rel_depth_product_vs_torch_gpu': float(((d - od).abs() / od.abs().clamp_min(1e-3)).max()),
            'max_rel_color_product_vs_torch_gpu': float((c - oc).abs().max() / oc.abs().max())}


def cpu_leg(rend, dec, sd, scene, tsdf_bnds, c2w, gt_depth, depth_img, color_img, dev, NS, NF, n_cpu):
    """The oracle on this host's cores on a bounded ray sample of the SAME workload; parity of THE TIMED OUTPUT (the
    images the last timed step produced) on exactly those rays.  render_img clamps `far` with each 100 000-ray batch's
    own max depth (src/utils/Renderer.py:294-313), so the oracle gets every picked ray's batch max."""
    import torch
    from oracle import adfp_oracle as O
    from attentive_dfprior_amd.common import get_rays
    ro, rd = get_rays(scene.H, scene.W, scene.fx, scene.fy, scene.cx, scene.cy, c2w, dev)
    tot = scene.H * scene.W
    pick = torch.arange(0, tot, max(1, tot // n_cpu), device=dev)[:n_cpu]
    ro, rd, gd = ro.reshape(-1, 3)[pick].contiguous(), rd.reshape(-1, 3)[pick].contiguous(), gt_depth.reshape(-1)[pick].contiguous()
    d = depth_img.reshape(-1)[pick]
    c = color_img.reshape(-1, 3)[pick]
    bsz = rend.ray_batch_size
    batch_of = (pick // bsz).cpu()
    batch_max = [gt_depth.reshape(-1)[b * bsz:(b + 1) * bsz].max().cpu() for b in range((tot + bsz - 1) // bsz)]
    ncpu = os.cpu_count() or 1
    c_cpu = {k: v.cpu() for k, v in scene.c.items()}
    tsdf_cpu = scene.tsdf_volume.cpu()
    ro_c, rd_c, gd_c = ro.cpu(), rd.cpu(), gd.cpu()

    def oracle(sl_idx, dmax):
        return O.render_batch_ray(sd, c_cpu, rd_c[sl_idx], ro_c[sl_idx], tsdf_cpu, scene.tsdf_bnds, scene.bound, 'color',
                                  gd_c[sl_idx], NS, NF, depth_max=dmax)

    def oracle_all():
        outs = []
        for b in range(len(batch_max)):
            idx = torch.nonzero(batch_of == b).reshape(-1)
            if idx.numel():
                outs.append((idx, oracle(idx, batch_max[b])))
        od = torch.empty(len(pick), dtype=torch.float64)
        oc = torch.empty(len(pick), 3)
        for idx, (a, _, b_, _) in outs:
            od[idx] = a
            oc[idx] = b_
        return od, oc
    # thread count: big hosts oversubscribe badly with all cores, so pick the faster of {all cores, 32}
    # on a 2 000-ray probe, then time the whole sample with it
    probe = torch.arange(0, min(2000, ro_c.shape[0]))
    cores, tprobe = ncpu, None
    for threads in sorted({ncpu, min(32, ncpu)}):
        torch.set_num_threads(threads)
        with torch.no_grad():
            t0 = time.perf_counter()
            oracle(probe, batch_max[0])
            dt = time.perf_counter() - t0
        if tprobe is None or dt < tprobe:
            tprobe, cores = dt, threads
    torch.set_num_threads(cores)
    best = None
    with torch.no_grad():
        for it in range(3):          # 1 warm-up + best of 2
            t0 = time.perf_counter()
            od, oc = oracle_all()
            dt = time.perf_counter() - t0
            if it > 0 and (best is None or dt < best):
                best = dt
    # forward + backward of the Mapper loss (src/Mapper.py:457-473) on a 2 000-ray subset: the oracle with autograd on
    # the host cores beside the product path's autograd on the GPU, same rays, gradients to grids + colour / attention nets
    nt = min(2000, ro_c.shape[0])
    gcol = torch.rand(nt, 3, generator=torch.Generator().manual_seed(0))
    train = {}
    try:
        c_req = {k: v.clone().requires_grad_(True) for k, v in c_cpu.items()}
        sd_req = {k: (v.clone().requires_grad_(True) if k.startswith(('color_decoder', 'mlp')) else v) for k, v in sd.items()}
        tb = None
        for it in range(2):
            for v in list(c_req.values()) + [v for v in sd_req.values() if v.requires_grad]:
                v.grad = None
            t0 = time.perf_counter()
            td, tu, tc, tw = O.render_batch_ray(sd_req, c_req, rd_c[:nt], ro_c[:nt], tsdf_cpu, scene.tsdf_bnds, scene.bound,
                                                'color', gd_c[:nt], NS, NF)
            O.mapper_loss(td, tc, tw, gd_c[:nt], gcol, 'color').backward()
            dt = time.perf_counter() - t0
            tb = dt if tb is None or dt < tb else tb
        c_g = {k: v.detach().clone().requires_grad_(True) for k, v in scene.c.items()}
        ro_t, rd_t, gd_t, gc_t = ro[:nt], rd[:nt], gd[:nt], gcol.to(dev)
        for p_ in list(dec.low_decoder.parameters()) + list(dec.high_decoder.parameters()):
            p_.requires_grad_(False)

        def gpu_it():
            for v in c_g.values():
                v.grad = None
            dd, uu, cc, ww = rend.render_batch_ray(c_g, dec, rd_t, ro_t, dev, scene.tsdf_volume, tsdf_bnds, 'color', gt_depth=gd_t)
            m = gd_t > 0
            (torch.abs(gd_t[m] - dd[m]).sum() + 0.2 * torch.abs(gc_t - cc).sum()).backward()
        for _ in range(3):
            gpu_it()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(10):
            gpu_it()
        torch.cuda.synchronize(dev)
        tg = (time.perf_counter() - t0) / 10
        gl = c_g['grid_color'].grad.cpu()
        train = {'train_fwd_bwd': {'rays': nt, 'unit': 'rays/s', 'value': nt / tg, 'ms_per_iteration': tg * 1e3,
                                   'cpu_baseline': nt / tb, 'cpu_cores': cores,
                                   'max_rel_grad_grid_color_vs_oracle': float((gl - c_req['grid_color'].grad).abs().max()
                                                                              / c_req['grid_color'].grad.abs().max())}}
        for p_ in dec.parameters():
            p_.grad = None
            p_.requires_grad_(True)
    except Exception as e:                      # the training leg is extra information, never the reason a bench fails
        train = {'train_fwd_bwd': {'error': repr(e)[:200]}}
    mse = float(((c.cpu().double() - oc.double()) ** 2).mean())
    peak = float(oc.abs().max())
    psnr = 10.0 * torch.log10(torch.tensor(peak * peak / max(mse, 1e-300))).item()
    dmse = float(((d.cpu() - od) ** 2).mean())
    dpeak = float(od.abs().max())
    return {
        'cpu_baseline': {'value': len(pick) / best, 'unit': 'rays/s', 'cores': cores, 'kind': 'port',
                         'sample': f'{len(pick)} evenly strided rays of the same frame, 64 samples/ray, stage color, '
                                   f'no_grad, torch CPU with {cores} threads (faster of {ncpu} / {min(32, ncpu)} on a probe), best of 2 after 1 warm-up '
                                   f'({best:.2f} s)'},
        'parity_vs_oracle': {'psnr_color_db': psnr, 'psnr_depth_db': 10.0 * torch.log10(torch.tensor(dpeak * dpeak / max(dmse, 1e-300))).item(),
                             'max_rel_depth': float(((d.cpu() - od).abs().max() / od.abs().max())),
                             'max_rel_color': float(((c.cpu() - oc).abs().max() / oc.abs().max())),
                             'rays': len(pick), 'of': 'the images produced by the last TIMED step, indexed at the sampled rays'},
        **train,
    }


if __name__ == '__main__':
    main()
