"""LPIPS-VGG timing: LPIPSVGG beside LPIPS (AlexNet) on the same 16 frame pairs of 346x260, 640x480 and 970x624 in the same run --
device events around `--iters` calls of each, alternating, `--reps` times after a warm-up of every shape; one process.  Prints
one JSON line and writes it to --out: microseconds per call and per pair of both (the best and every repeat), their ratio, the
algorithmic TFLOP/s of LPIPS-VGG (evr_lpips_vgg_flops over its time: the thirteen convolutions, the streaming kernels' time
included in the denominator -- the figure to hold against the ConvLSTM kernel's rate in VERDICT.md), and the byte floor of the two
new streaming kernels (vgg_conv1_1_kernel, vgg_pool_score_kernel: the bytes they must read and write at 4 B per channel, at the
8.0 TB/s HBM peak).

Their own time comes from a profiler run, one shape at a time, because event timing sees whole calls only:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/lpips_vgg_bench.py --profile 20 --shapes 346x260
    python tools/lpips_vgg_bench.py --kernel-stats <dir>/.../*_kernel_stats.csv --profiled-calls 22 --stats-shape 346x260 --out ...

(--profile N makes 2 + N plain calls of LPIPSVGG and times nothing; the second command runs the timing of every shape and adds,
for the profiled shape, the two kernels' microseconds per call from the table and the fraction of their floor that stands for.)
Without --kernel-stats, and for the other shapes, the kernel times are reported as "not measured".

    python tools/lpips_vgg_bench.py [--pairs 16] [--iters 20] [--reps 5] [--out profiles/lpips_vgg_bench.json]
"""
import argparse
import csv
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12           # bytes/s, the part's specification
SHAPES = ((260, 346), (480, 640), (624, 970))
TAP_C = (64, 128, 256, 512, 512)


def pairs(n, H, W):
    """A smooth texture in [0, 1] and a copy 6 % of noise away."""
    g = torch.Generator(device='cuda').manual_seed(H * 1000 + W)
    yy = torch.arange(H, device='cuda', dtype=torch.float32)[:, None]
    xx = torch.arange(W, device='cuda', dtype=torch.float32)[None, :]
    base = 0.5 + 0.25 * torch.sin(xx / 5.0) * torch.cos(yy / 6.0)
    ref = (base[None] + 0.02 * torch.randn((n, H, W), device='cuda', generator=g)).clamp_(0.0, 1.0).contiguous()
    img = (ref + 0.06 * torch.randn((n, H, W), device='cuda', generator=g)).clamp_(0.0, 1.0).contiguous()
    return img, ref


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def byte_floors(n, H, W):
    """Algorithmic bytes per call of the two streaming kernels (both frames of n pairs, 4 B per channel in every format)."""
    conv1_1 = 2 * n * H * W * 4 + 2 * n * H * W * 64 * 4
    pool_score, h, w = 0, H, W
    for l, c in enumerate(TAP_C):
        pool_score += 2 * n * h * w * c * 4 + (2 * n * (h // 2) * (w // 2) * c * 4 if l < 4 else 0)
        h, w = h // 2, w // 2
    return {'vgg_conv1_1_kernel': conv1_1, 'vgg_pool_score_kernel': pool_score}


def kernel_table(path):
    """rocprofv3 --stats kernel table -> {kernel name: total nanoseconds}."""
    out = {}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            out[row['Name']] = out.get(row['Name'], 0.0) + float(row['TotalDurationNs'])
    return out


def models():
    from evreal_amd import weights
    from evreal_amd.lpips import LPIPS, LPIPSVGG
    return LPIPS(weights.synth_lpips_state_dict(seed=3)), LPIPSVGG(weights.synth_lpips_vgg_state_dict(seed=3))


def profile(n, calls, shapes):
    _, vgg = models()
    for H, W in shapes:
        img, ref = pairs(n, H, W)
        out = torch.empty(n, dtype=torch.float64, device='cuda')
        for _ in range(2 + calls):
            vgg(img, ref, out=out)
        torch.cuda.synchronize()
    print(json.dumps(dict(profiled_calls=2 + calls, shapes=[f'{W}x{H}' for H, W in shapes])))


def run(n, iters, reps, shapes, table, profiled_calls, stats_shape):
    alex, vgg = models()
    res = {}
    data = {}
    for H, W in shapes:
        data[(H, W)] = pairs(n, H, W)
    for H, W in shapes:          # (every shape is warmed up before its own windows: buffers, plans, code objects)
        img, ref = data[(H, W)]
        ao = torch.empty(n, dtype=torch.float64, device='cuda')
        vo = torch.empty(n, dtype=torch.float64, device='cuda')
        runs = {'lpips_vgg': lambda: vgg(img, ref, out=vo), 'lpips_alex': lambda: alex(img, ref, out=ao)}
        for fn in runs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in runs}
        for _ in range(reps):
            for k, fn in runs.items():              # alternating
                us[k].append(timed(fn, iters))
        best = {k: min(v) for k, v in us.items()}
        flops = vgg.flops()
        entry = {k: dict(us_per_call=round(best[k], 1), us_per_pair=round(best[k] / n, 2),
                         repeats_us_per_call=[round(v, 1) for v in us[k]]) for k in runs}
        kernels = {}
        for name, nbytes in byte_floors(n, H, W).items():
            floor_us = nbytes / HBM_PEAK * 1e6
            k = dict(bytes_per_call=nbytes, floor_us_per_call=round(floor_us, 2), us_per_call='not measured', floor_fraction='not measured')
            if table is not None and stats_shape == f'{W}x{H}':
                ns = sum(v for key, v in table.items() if name in key)
                if ns > 0:
                    k['us_per_call'] = round(ns / profiled_calls / 1e3, 1)
                    k['floor_fraction'] = round(floor_us / (ns / profiled_calls / 1e3), 4)
            kernels[name] = k
        res[f'{W}x{H}'] = dict(
            entry, vgg_over_alex=round(best['lpips_vgg'] / best['lpips_alex'], 2), gflop_per_call=round(flops / 1e9, 2),
            algorithmic_tflops=round(flops / (best['lpips_vgg'] * 1e-6) / 1e12, 1), kernels=kernels,
            saturation=vgg.saturation(), mean_score=round(float(vo.mean()), 5), mean_alex=round(float(ao.mean()), 5),
            finite=[int(torch.isfinite(vo).all()), int(torch.isfinite(ao).all())])
    return dict(pairs=n, iters=iters, reps=reps, arith=os.environ.get('EVR_ARITH', 'h3'), hbm_peak_bytes_per_s=HBM_PEAK, shapes=res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=16)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--shapes', nargs='*', default=None, help='a subset of 346x260 640x480 970x624 (W x H)')
    ap.add_argument('--profile', type=int, default=0, help='make 2 + N plain calls per shape for a profiler and time nothing')
    ap.add_argument('--kernel-stats', default=None, help='rocprofv3 --stats kernel table (csv) of a --profile run of ONE shape')
    ap.add_argument('--stats-shape', default='346x260', help='the shape of that run')
    ap.add_argument('--profiled-calls', type=int, default=0, help='calls of that run (what it printed)')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    shapes = SHAPES if not a.shapes else tuple((int(s.split('x')[1]), int(s.split('x')[0])) for s in a.shapes)
    if a.profile:
        profile(a.pairs, a.profile, shapes)
        return
    table = kernel_table(a.kernel_stats) if a.kernel_stats and a.profiled_calls > 0 else None
    line = json.dumps(run(a.pairs, a.iters, a.reps, shapes, table, a.profiled_calls, a.stats_shape))
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
