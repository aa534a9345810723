"""The AlexNet LPIPS kernels (csrc/lpips.hip, evr_lpips_forward) against the float64 oracle one layer at a time, at borders and tile
seams, in every arithmetic mode and under the three documented switches that no other test runs.

Inputs, lin-head variants and references are tests/lpips_probe.py's: three shapes (35x47, 71x99, 135x139), five pairs, ten state dicts
(only_l: layer l alone; tail_l: its last four channels alone).  tests/test_lpips_probe_cpu.py shows on the CPU that each of fourteen
deliberate errors (a border tap, a tile seam, a pool window, a lost pixel or channel run, ...) moves one of these scores by at least ten
times the gate, most by a thousand times; the totals that tests/test_gpu_prepost.py and tests/test_gpu_lpips_modes.py gate move by less
than the gate under several of them.

The gate is test_gpu_lpips_modes.bound: |got - want64| <= scale * max(2e-4 |want64| + 1e-7, 8 |want32 - want64|), scale 1 for h3 (the
default) and fp32, 10 for mx and mx6.  Pair 0 is identical and must score exactly 0.  The library reads its switches once per process:
one child interpreter per mode and per switch, each running the whole shape x variant x pair matrix on one handle per variant.

Measured on an MI355X, worst |got - want64| / bound over the gated pairs of every shape and variant, and the case that gave it (no
case exceeded the bound, so no kernel changed):
  h3 (default)             0.0698  35x47/tail_4 pair 3      per shape: 35x47 0.0698, 71x99 0.0195 (tail_3), 135x139 0.0253 (tail_0)
  h3, pair 1 alone (n = 1) 0.0654  35x47/tail_4
  h3, 65 pairs             0.0167  35x47/only_4             (only_2: 0.0070)
  fp32                     0.0126  35x47/tail_4 pair 3      (the fp32 oracle itself: 0.0064 of the bound from float64)
  mx, mx6                  0.0273  35x47/tail_2 pair 1      of their ten-fold bound
  EVR_LPIPS_CONV1_VALU=1   0.0063  135x139/tail_1 pair 3    30 of the 30 (shape, variant) cases differ in bits from the default
  EVR_LPIPS_BAND5=-1       0.0690  35x47/tail_3 pair 2
  EVR_LPIPS_SCORE_SPLIT=0 and =2: every score equal to the default's bit for bit.
The only_l variants stay under 0.02 in h3; the 4-channel tails carry the larger figures (0.07 of the bound is 1.4e-5 relative), and
most of that is the three-bf16-product conv1: with the direct conv1 the same cases fall below 0.007.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
import lpips_probe as lp
from test_gpu_lpips_modes import bound

pytestmark = pytest.mark.gpu

_SWITCHES = ('EVR_ARITH', 'EVR_FP32', 'EVR_LPIPS_CONV1_VALU', 'EVR_LPIPS_BAND5', 'EVR_LPIPS_SCORE_SPLIT')
_HANDLES = {}


def _key(shape, name):
    return f'{shape[0]}x{shape[1]}/{name}'


def _handle(name):
    """One LPIPS handle per variant, serving the three shapes in turn (its buffers are rebuilt when the shape changes)."""
    if name not in _HANDLES:
        from evreal_amd.lpips import LPIPS
        _HANDLES[name] = LPIPS(lp.variant(name))
    return _HANDLES[name]


def _score_matrix(shapes, names, single=False):
    """{'HxW/variant': scores of the five pairs} (single: of pair 1 alone, n = 1) on this process's GPU and arithmetic."""
    out = {}
    for shape in shapes:
        img, ref = (torch.from_numpy(a).cuda() for a in lp.pairs(shape))
        for name in names:
            m = _handle(name)
            out[_key(shape, name)] = (m(img[1:2], ref[1:2]) if single else m(img, ref)).cpu().numpy().tolist()
    return out


_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_lpips_probe as t
job = json.load(open(sys.argv[2]))
print('RESULT ' + json.dumps(t._score_matrix([tuple(s) for s in job['shapes']], job['variants'])))
'''


def _child(tmp_path, env):
    """The score matrix from a fresh interpreter with `env` on top of an environment without any LPIPS switch."""
    job = str(tmp_path / 'job.json')
    with open(job, 'w') as f:
        json.dump({'shapes': lp.SHAPES, 'variants': lp.VARIANTS}, f)
    e = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    e.update(env)
    r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, job], env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (env, r.stdout[-2000:] + r.stderr[-4000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])


def _check(label, got, scale, shapes=lp.SHAPES, names=lp.VARIANTS, pairs=range(lp.NPAIRS)):
    """Every score of `got` within the bound of its float64 oracle value, pair 0 exactly 0; prints the worst error / bound per case."""
    bad, lines, worst = [], [], (0.0, None)
    for shape in shapes:
        for name in names:
            want64, want32 = (w[list(pairs)] for w in lp.reference(shape, name))
            g = np.asarray(got[_key(shape, name)], dtype=np.float64)
            assert g.shape == want64.shape, (label, shape, name, g.shape)
            lim = bound(want64, want32, scale)
            ratio = np.abs(g - want64) / lim
            for i, p in enumerate(pairs):
                if p == 0:
                    ok = g[i] == 0.0
                else:
                    ok = bool(np.isfinite(g[i])) and abs(g[i] - want64[i]) <= lim[i]
                    if ratio[i] > worst[0]:
                        worst = (float(ratio[i]), f'{_key(shape, name)} pair {p}')
                if not ok:
                    bad.append(f'{_key(shape, name)} pair {p}: got {g[i]!r} want {want64[i]!r} error / bound {ratio[i]:.3f}')
            gated = [i for i, p in enumerate(pairs) if p != 0]
            lines.append(f'  {label:12s} {_key(shape, name):16s} worst error / bound {ratio[gated].max():.4f}')
    print(f'\n[{label}] worst error / bound {worst[0]:.4f} at {worst[1]}\n' + '\n'.join(lines))
    assert not bad, (label, bad)


@pytest.fixture(scope='module')
def default_scores():
    """The whole matrix in this process (default arithmetic, no switch), five pairs at once."""
    return _score_matrix(lp.SHAPES, lp.VARIANTS)


@pytest.mark.parametrize('shape', lp.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_default_arithmetic_per_layer(default_scores, shape):
    """h3, in process: the ten variants on the five pairs, then pair 1 alone on the same handles (n = 1: 256 score work-groups per
    image, most of them without a pixel)."""
    _check('h3', default_scores, 1.0, shapes=[shape])
    _check('h3 n=1', _score_matrix([shape], lp.VARIANTS, single=True), 1.0, shapes=[shape], pairs=[1])


def test_batch_of_65_pairs():
    """35x47 with relu3 and relu5 alone: 65 pairs (the five, tiled) make score_blocks(65) = 32 work-groups per image for two pixels."""
    from evreal_amd.lpips import LPIPS
    shape, reps = lp.SHAPES[0], 13
    img, ref = (torch.from_numpy(np.tile(a, (reps, 1, 1))).cuda() for a in lp.pairs(shape))
    assert img.shape[0] == 65
    for name in ('only_2', 'only_4'):
        got = LPIPS(lp.variant(name))(img, ref).cpu().numpy()
        want64, want32 = (np.tile(w, reps) for w in lp.reference(shape, name))
        ratio = np.abs(got - want64) / bound(want64, want32, 1.0)
        print(f'\n[h3 n=65] {_key(shape, name)} worst error / bound {ratio.max():.4f}')
        assert (got[0::5] == 0.0).all(), (name, got[0::5])
        assert (np.abs(got - want64) <= bound(want64, want32, 1.0)).all(), (name, got, want64)


@pytest.mark.parametrize('mode,scale', [('fp32', 1.0), ('mx', 10.0), ('mx6', 10.0)])
def test_arithmetic_modes_per_layer(tmp_path, mode, scale):
    """fp32 at 135x139 is the only run of lpips_conv1_kernel's interior branch (the folded bias) in the suite; mx and mx6 see the
    matrix-core conv1 beyond two tiles."""
    _check(mode, _child(tmp_path, {'EVR_ARITH': mode}), scale)


def _differing(a, b):
    return [k for k in a if not np.array_equal(np.asarray(a[k], np.float64).view(np.uint64), np.asarray(b[k], np.float64).view(np.uint64))]


def test_switch_conv1_valu(tmp_path, default_scores):
    """EVR_LPIPS_CONV1_VALU=1: the direct conv1 in the default arithmetic.  Within the bound, and not the same bits as the matrix-core
    conv1 (identical bits everywhere would mean the switch selected nothing)."""
    got = _child(tmp_path, {'EVR_LPIPS_CONV1_VALU': '1'})
    _check('CONV1_VALU', got, 1.0)
    diff = _differing(got, default_scores)
    print(f'CONV1_VALU: {len(diff)} of {len(got)} cases differ in bits from the default')
    assert diff, 'EVR_LPIPS_CONV1_VALU=1 and the default gave identical bits: the direct conv1 kernel was not reached'


def test_switch_band5_off(tmp_path):
    """EVR_LPIPS_BAND5=-1: conv2 on the implicit GEMM instead of the band kernel."""
    _check('BAND5=-1', _child(tmp_path, {'EVR_LPIPS_BAND5': '-1'}), 1.0)


@pytest.mark.parametrize('split', ['0', '2'])
def test_switch_score_split_is_bit_identical(tmp_path, default_scores, split):
    """EVR_LPIPS_SCORE_SPLIT=0 (one score launch for the five layers) and =2 (one per layer): lpips.hip states the same partial sums
    and the same final reduction as the default, so the same bits."""
    got = _child(tmp_path, {'EVR_LPIPS_SCORE_SPLIT': split})
    assert sorted(got) == sorted(default_scores)
    diff = _differing(got, default_scores)
    assert not diff, (split, [(k, got[k], default_scores[k]) for k in diff[:5]])
