"""What the closed-form metric timing tools share (frmetrics_bench.py, gmsd_bench.py, vifp_bench.py): the frame pairs, device-event
timing, the alternating repeat loop, one child process per shape under a time limit, and the JSON line.  A tool is a table of
runs per shape plus the ratios it derives from their best times."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12           # bytes/s, the part's specification
SHAPES = ((260, 346), (480, 640), (624, 970))
STEP_TIMEOUT_S = 180


def pairs(n, H, W):
    """A smooth texture in [0, 1] and a copy 6 % of noise away: edges in every tile, structure in every window."""
    import torch
    g = torch.Generator(device='cuda').manual_seed(H * 1000 + W)
    yy = torch.arange(H, device='cuda', dtype=torch.float32)[:, None]
    xx = torch.arange(W, device='cuda', dtype=torch.float32)[None, :]
    base = 0.5 + 0.25 * torch.sin(xx / 5.0) * torch.cos(yy / 6.0)
    ref = (base[None] + 0.02 * torch.randn((n, H, W), device='cuda', generator=g)).clamp_(0.0, 1.0).contiguous()
    img = (ref + 0.06 * torch.randn((n, H, W), device='cuda', generator=g)).clamp_(0.0, 1.0).contiguous()
    return img, ref


def timed(fn, iters):
    """Microseconds per call: device events around `iters` calls."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def alternate(runs, iters, reps, warmup=5):
    """{name: fn} -> {name: [us per call of every repeat]}: all warmed up first, then `reps` rounds, the runs alternating."""
    import torch
    for fn in runs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            us[k].append(timed(fn, iters))
    return us


def entries(us, n, repeats=True, digits=2):
    """-> ({name: best us per call}, {name: its JSON entry})."""
    best = {k: min(v) for k, v in us.items()}
    entry = {k: dict(us_per_call=round(best[k], 1), us_per_frame=round(best[k] / n, digits)) for k in us}
    if repeats:
        for k in us:
            entry[k]['repeats_us_per_call'] = [round(v, 1) for v in us[k]]
    return best, entry


def read_floor(best_us, n, H, W):
    """The fraction of the read floor (8 H W algorithmic bytes per frame at the HBM peak) a time stands for."""
    floor_us = 8 * H * W * n / HBM_PEAK * 1e6
    return dict(bytes_per_frame=8 * H * W, read_floor_us_per_call=round(floor_us, 3), read_floor_fraction=round(floor_us / best_us, 4))


def parser(frames, iters, reps=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=frames)
    ap.add_argument('--iters', type=int, default=iters)
    if reps is not None:
        ap.add_argument('--reps', type=int, default=reps)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--shape', default=None, help='(internal) HxW: time this one shape in this process and print its entry')
    return ap


def run(script, a, run_shape, head, shapes=SHAPES):
    """With --shape: run_shape(a, H, W) in this process.  Without: one child process per shape, each under its own time limit
    (a shape that fails or runs out of time ends the run: nothing more is started on the GPU), then the line json(head(entries))."""
    if a.shape:
        H, W = (int(v) for v in a.shape.split('x'))
        print(json.dumps(run_shape(a, H, W)))
        return
    res = {}
    for H, W in shapes:
        cmd = [sys.executable, os.path.abspath(script), '--frames', str(a.frames), '--iters', str(a.iters), '--shape', f'{H}x{W}']
        if hasattr(a, 'reps'):
            cmd += ['--reps', str(a.reps)]
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)     # (raises at the limit: the run ends)
        if done.returncode != 0:
            sys.stderr.write(done.stderr)
            sys.exit(f'{W}x{H}: exit status {done.returncode}; nothing more is started')
        res[f'{W}x{H}'] = json.loads(done.stdout.strip().splitlines()[-1])
    line = json.dumps(head(res))
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')
