"""Colour post-process normalisation timing: evr_color_percentile_normalize (histogram + byte table, uint8 in, uint8 out) beside
the composition of the pieces that existed before it -- bgr.float().div(255) viewed as [n,H,3W], prepost.post_process_normalization
(evr_percentile_normalize), then torch clamp / mul(255) / round / to(uint8) -- on the same frames in the same run.  n = 16 frames of
970x624 and of 346x260, uniform random bytes and one constant level (every byte in one histogram bin: the contention worst case).
Device events around `--iters` calls after a warm-up, the two forms alternating, `--repeats` times; prints one JSON line with the
median and the spread of the microseconds per call, their ratios, and how many bytes of the random frames the two forms disagree
on.  Under `rocprofv3 --kernel-trace --stats` (with --only new) the same run gives the per-kernel table of
profiles/color_norm_kernel_stats.md.

    python tools/color_norm_bench.py [--frames 16] [--iters 50] [--repeats 5] [--norm robust] [--only new|composition]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(624, 970), (260, 346)]


def composition(bgr, norm):
    from evreal_amd.prepost import post_process_normalization
    n, H, W, _ = bgr.shape
    img = bgr.float().div(255).view(n, H, 3 * W)
    post_process_normalization(img, norm)
    return img.clamp_(0, 1).mul_(255).round_().to(torch.uint8).view(n, H, W, 3)


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--norm', default='robust', choices=['robust', 'standard', 'exprobust'])
    ap.add_argument('--only', default=None, choices=['new', 'composition'], help='run one form only (for a kernel trace)')
    a = ap.parse_args()
    from evreal_amd.prepost import color_post_process_normalization
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    g = torch.Generator(device='cuda').manual_seed(0)
    cases = []
    for H, W in SIZES:
        shape = (a.frames, H, W, 3)
        frames = {'random': torch.randint(0, 256, shape, dtype=torch.uint8, device='cuda', generator=g),
                  'constant': torch.full(shape, 255, dtype=torch.uint8, device='cuda')}
        for content, x in frames.items():
            out = torch.empty_like(x)
            forms = {'new': lambda: color_post_process_normalization(x, a.norm, out=out),
                     'composition': lambda: composition(x, a.norm)}
            if a.only:
                forms = {a.only: forms[a.only]}
            us = {k: [] for k in forms}
            for fn in forms.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.repeats):
                for k, fn in forms.items():                 # alternating
                    us[k].append(timed(fn, a.iters))
            case = dict(size=f'{W}x{H}', content=content, frames=a.frames, bytes=x.numel(),
                        us_per_call={k: dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1))
                                     for k, v in us.items()})
            if not a.only:
                case['new_over_composition'] = round(statistics.median(us['new']) / statistics.median(us['composition']), 3)
                if content == 'random':
                    case['bytes_differing_from_composition'] = int((forms['new']() != forms['composition']()).sum())
            cases.append(case)
    res = dict(norm=a.norm, iters=a.iters, repeats=a.repeats, cases=cases)
    if not a.only:
        med = {(c['size'], c['content']): c['us_per_call']['new']['median'] for c in cases}
        res['constant_over_random'] = {s: round(med[(s, 'constant')] / med[(s, 'random')], 3) for s in sorted({c['size'] for c in cases})}
    print(json.dumps(res))


if __name__ == '__main__':
    main()
