"""VIFp kernel timing: evr_vifp beside evr_fr_metrics with ms_ssim (the nearest existing kernel: a Gaussian pyramid in fp64) on
the same 16 frame pairs of 346x260, 640x480 and 970x624 -- device events around `--iters` calls of each, alternating, `--reps`
times after a warm-up.  One process per shape, each started by this script under its own time limit (a shape that fails or runs
out of time ends the run: nothing more is started on the GPU).  Prints one JSON line and writes it to --out: microseconds per
call and per frame of both (the best and every repeat), their ratio, and the fraction of VIFp's read floor (8 H W algorithmic
bytes per frame at the 8.0 TB/s HBM peak) its time stands for.

    python tools/vifp_bench.py [--frames 16] [--iters 200] [--reps 5] [--out profiles/vifp_bench.json]
"""
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
    """A smooth texture in [0, 1] and a copy 6 % of noise away: structure in every window."""
    import torch
    g = torch.Generator(device='cuda').manual_seed(H * 1000 + W)
    yy = torch.arange(H, device='cuda', dtype=torch.float32)[:, None]
    xx = torch.arange(W, device='cuda', dtype=torch.float32)[None, :]
    base = 0.5 + 0.25 * torch.sin(xx / 5.0) * torch.cos(yy / 6.0)
    ref = (base[None] + 0.02 * torch.randn((n, H, W), device='cuda', generator=g)).clamp_(0.0, 1.0).contiguous()
    img = (ref + 0.06 * torch.randn((n, H, W), device='cuda', generator=g)).clamp_(0.0, 1.0).contiguous()
    return img, ref


def timed(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def run_shape(n, H, W, iters, reps):
    import torch
    from evreal_amd.prepost import VIFP, FullRefMetrics
    vifp, fr = VIFP(), FullRefMetrics()
    img, ref = pairs(n, H, W)
    vo = torch.empty((n, 9), dtype=torch.float64, device='cuda')
    mo = torch.empty((n, 2), dtype=torch.float64, device='cuda')
    runs = {'vifp': lambda: vifp.stats(img, ref, out=vo), 'ms_ssim': lambda: fr(img, ref, psnr=False, ms_ssim=True, out=mo)}
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():              # alternating
            us[k].append(timed(fn, iters))
    best = {k: min(v) for k, v in us.items()}
    floor_us = 8 * H * W * n / HBM_PEAK * 1e6
    entry = {k: dict(us_per_call=round(best[k], 1), us_per_frame=round(best[k] / n, 2),
                     repeats_us_per_call=[round(v, 1) for v in us[k]]) for k in runs}
    return dict(entry, vifp_over_ms_ssim=round(best['vifp'] / best['ms_ssim'], 3), bytes_per_frame=8 * H * W,
                read_floor_us_per_call=round(floor_us, 3), read_floor_fraction=round(floor_us / best['vifp'], 4),
                mean_score=round(float(vo[:, 0].mean()), 5), mean_ms_ssim=round(float(mo[:, 1].mean()), 5),
                finite=[int(torch.isfinite(vo).all()), int(torch.isfinite(mo).all())])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    ap.add_argument('--shape', default=None, help='(internal) HxW: time this one shape in this process and print its entry')
    a = ap.parse_args()
    if a.shape:
        H, W = (int(v) for v in a.shape.split('x'))
        print(json.dumps(run_shape(a.frames, H, W, a.iters, a.reps)))
        return
    res = {}
    for H, W in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), '--frames', str(a.frames), '--iters', str(a.iters), '--reps', str(a.reps),
               '--shape', f'{H}x{W}']
        done = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT_S)     # (raises at the limit: the run ends)
        if done.returncode != 0:
            sys.stderr.write(done.stderr)
            sys.exit(f'{W}x{H}: exit status {done.returncode}; nothing more is started')
        res[f'{W}x{H}'] = json.loads(done.stdout.strip().splitlines()[-1])
    line = json.dumps(dict(frames=a.frames, iters=a.iters, reps=a.reps, hbm_peak_bytes_per_s=HBM_PEAK,
                           launches_per_call=dict(vifp=5, ms_ssim=6), shapes=res))
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
