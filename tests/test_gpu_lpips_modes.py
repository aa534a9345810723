"""LPIPS (AlexNet, evr_lpips_*, evreal_amd.lpips.LPIPS) in the arithmetic modes that tests/test_gpu_prepost.py does not reach: the
fp32 / Winograd path and the mx path of its conv2..conv5 (mx6 runs them as mx), with the set-up they share with LPIPS-VGG
(csrc/lpips_host.h) and the networks (csrc/conv.h).  The form of test_arithmetic_modes in tests/test_gpu_lpips_vgg.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

H, W = 64, 80      # feature maps 15x19 -> 7x9 -> 3x4: conv2 (5x5) has several tiles, conv3..conv5 less than one (split-K, Winograd edge tiles)
_REF = {}


def _frames():
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    ref = np.stack([0.5 + 0.4 * np.sin(xx / (7.0 + i)) * np.cos(yy / (9.0 + i)) for i in range(3)]).astype(np.float32)
    img = np.clip(ref + 0.1 * rng.standard_normal(ref.shape), 0, 1).astype(np.float32)
    img[0] = ref[0]
    return img, ref


def _reference():
    """(img, ref, want64, want32): computed once, never modified."""
    if not _REF:
        from evreal_amd import weights
        from oracle import lpips as ol
        sd = weights.synth_lpips_state_dict(seed=3)
        img, ref = _frames()
        _REF['r'] = (img, ref, ol.lpips(sd, img, ref, torch.float64), ol.lpips(sd, img, ref, torch.float32))
    return _REF['r']


_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
from evreal_amd import weights
from evreal_amd.lpips import LPIPS
f = np.load(sys.argv[2])
a, b = torch.from_numpy(f['img']).cuda(), torch.from_numpy(f['ref']).cuda()
m = LPIPS(weights.synth_lpips_state_dict(seed=3))
first = m(a, b).cpu().numpy().tolist()
one = m(a[1:2], b[1:2]).cpu().numpy().tolist()
again = m(a, b).cpu().numpy().tolist()
print('RESULT ' + json.dumps({'first': first, 'one': one, 'again': again}))
'''


def run_mode(root, mode, frames_file):
    """The child's scores in `mode` from the build under `root`: 3 pairs, pair 1 alone, the 3 pairs again on the same handle."""
    env = dict(os.environ, EVR_ARITH=mode)
    env.pop('EVR_FP32', None)
    r = subprocess.run([sys.executable, '-c', _CHILD, root, frames_file], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])


def bound(want64, want32, scale):
    """This project's LPIPS gate (2e-4 relative + 1e-7), or eight times the reference arithmetic's own fp32-against-fp64 error on
    the same inputs where that is larger; `scale` as in tests/test_gpu_lpips_vgg.py."""
    return scale * np.maximum(2e-4 * np.abs(want64) + 1e-7, 8.0 * np.abs(want32 - want64))


@pytest.mark.parametrize('mode,scale', [('fp32', 1.0), ('mx', 10.0), ('mx6', 10.0)])
def test_arithmetic_modes(tmp_path, mode, scale):
    """One fresh child process per mode (the library reads EVR_ARITH once), 64 x 80 with 3 pairs; pair 0 is identical and scores
    exactly 0.  |got - want64| <= scale * max(2e-4 |want64| + 1e-7, 8 |want32 - want64|) for every total: scale 1 for fp32, 10 for mx
    and mx6 (the ratio between this project's image gates for those modes and for h3, 1e-4 against 1e-5).  The handle then serves 1
    pair and the 3 pairs again: the plan cache in that mode, the second 3-pair result equal to the first bit for bit.
    Worst measured error / bound on an MI355X: fp32 0.00026, mx and mx6 0.00093 of their ten-fold bound (the default h3 arithmetic,
    which tests/test_gpu_prepost.py gates, 0.0149 of the fp32 bound) -- the same figures before and after conv2..conv5 moved onto the
    set-up shared with LPIPS-VGG: the scores of the two builds are equal bit for bit."""
    img, ref, want64, want32 = _reference()
    frames_file = str(tmp_path / 'frames.npz')
    np.savez(frames_file, img=img, ref=ref)
    got = run_mode(ROOT, mode, frames_file)
    first, one, again = (np.array(got[k]) for k in ('first', 'one', 'again'))
    ratio = np.abs(first - want64) / bound(want64, want32, scale)
    print(f'{mode}: error / bound (worst {ratio.max():.4f}) {ratio}')
    assert first.shape == (3,) and first[0] == 0.0
    assert (np.abs(first - want64) <= bound(want64, want32, scale)).all(), (mode, first, want64)
    assert np.array_equal(again, first)
    assert (np.abs(one - want64[1:2]) <= bound(want64[1:2], want32[1:2], scale)).all(), (mode, one, want64[1])
