"""The skewed loop of the 256 x 256 ConvLSTM gate kernel (csrc/conv.hip conv3x3_wide16_kernel<2, true>: the block's wave halves alternate
load and MFMA segments) against its lock-step loop (EVR_WIDE16_ALT=0).

Every accumulator sees the same MFMAs in the same order in both loops, so the results are equal bit for bit: the images of every frame and
the final h / c of all three levels, compared as uint32.  EVR_WIDE_MIN=1 EVR_WIDE=3 put the 256 x 256 form on every ConvLSTM layer of
the two smallest cases of test_gpu_wide16.CASES, three frames each:
    24x40 x 3    M = 720 / 180 / 45: a single tile mostly past M, widths 20 / 10 / 5 no multiple of 16, blocks straddle rows and images
    50x70 x 2    several tiles, an image boundary inside a 16-pixel block
with nchunks = 4, 8 and 16 at the three levels.  Equal bits cannot show which loop ran: evr_model_profile_read's "kernel.wide16_alt" row
counts the launches of the skewed loop, 3 levels x 3 frames per case in the default interpreter and none under EVR_WIDE16_ALT=0.
(test_gpu_wide16.py compares the default loop, now this one, with the float64 oracle.)  The switches are read once per process: one
interpreter per variant.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_IDS = [0, 1]               # of test_gpu_wide16.CASES
ALT_ROW = 'kernel.wide16_alt'

_CHILD = r"""
import json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_wide16 as t
from evreal_amd import model, weights
out, launches = {}, {}
for ci in json.loads(sys.argv[3]):
    H, W, n, frames = t.CASES[ci]
    sd, vox = t._inputs(ci)
    m = model.E2VIDRecurrent(dict(weights.E2VID_KWARGS))
    m.load_state_dict(sd)
    assert m.arith == 'h3', m.arith
    m.reset_states()
    m.profile(sys.argv[4])
    for f in range(frames):
        out[f'{ci}.img{f}'] = m(torch.from_numpy(vox[f]).cuda())['image'].cpu().numpy()
    for k, shp in t._state_shapes(H, W, n).items():
        out[f'{ci}.{k}'] = m.read_tensor(k).cpu().numpy().reshape(shp)
    launches[str(ci)] = {r['name']: int(r['launches']) for r in m.profile_read()}
    m.profile(None)
np.savez(sys.argv[2], **out)
json.dump(launches, open(sys.argv[2] + '.json', 'w'))
"""


def _child(tmp_path, name, env):
    out = str(tmp_path / f'{name}.npz')
    drop = ('EVR_MFMA16', 'EVR_WIDE', 'EVR_WIDE_MIN', 'EVR_WIDE16_ALT', 'EVR_ARITH', 'EVR_FP32', 'EVR_LIB')
    e = {k: v for k, v in os.environ.items() if k not in drop}
    e.update(env)
    r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, out, json.dumps(CASE_IDS), ALT_ROW], env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (name, r.stdout[-2000:] + r.stderr[-3000:])
    z = np.load(out)
    return {k: z[k] for k in z.files}, json.load(open(out + '.json'))


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp('wide16_alt')
    env = {'EVR_WIDE_MIN': '1', 'EVR_WIDE': '3'}
    return {'alt': _child(d, 'alt', env), 'lockstep': _child(d, 'lockstep', dict(env, EVR_WIDE16_ALT='0'))}


def test_skewed_loop_equals_lockstep_loop_bit_for_bit(runs):
    import test_gpu_wide16 as t
    a, b = runs['alt'][0], runs['lockstep'][0]
    want = {f'{ci}.{k}' for ci in CASE_IDS for k in [f'img{f}' for f in range(t.CASES[ci][3])] + list(t._state_shapes(*t.CASES[ci][:3]))}
    assert set(a) == want and set(b) == want, (sorted(set(a) ^ want), sorted(set(b) ^ want))
    bad = []
    for k in sorted(want):
        assert a[k].dtype == np.float32 and a[k].shape == b[k].shape and np.isfinite(a[k]).all(), k
        ndiff = int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum())
        print(f'  {k:8s} {a[k].size:8d} values, {ndiff} differ, max|x| {float(np.abs(a[k]).max()):.3e}')
        if ndiff:
            bad.append((k, ndiff, float(np.abs(a[k].astype(np.float64) - b[k]).max())))
    assert not bad, bad


def test_the_skewed_loop_is_what_ran(runs):
    import test_gpu_wide16 as t
    for ci in CASE_IDS:
        frames = t.CASES[ci][3]
        alt, lock = runs['alt'][1][str(ci)], runs['lockstep'][1][str(ci)]
        print(f'  case {ci}: skewed-loop launches {alt} (default), {lock} (EVR_WIDE16_ALT=0)')
        assert alt == {ALT_ROW: 3 * frames}, alt            # three ConvLSTM levels per frame, nothing else in the filtered read-out
        assert lock == {ALT_ROW: 0}, lock
