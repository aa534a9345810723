"""The trimmed prologue / epilogue of the 16x16x32 ConvLSTM gate kernel (csrc/conv.hip conv3x3_wide16_kernel<.., .., TAIL = true>: the
first requests ahead of the prologue's arithmetic, the c_prev warm-up piece in the last step, 16-B h stores after a lane exchange, static
priority for the late half) against the kernel as it was (EVR_WIDE16_TAIL=0).

Nothing in the tail touches an accumulator's MFMA order, the cell update or the H2 split, so the results are equal bit for bit: the images
of every frame and the final h / c of all three levels, compared as uint32, zero differing words allowed.  Three loops carry the tail and
each is compared with its own EVR_WIDE16_TAIL=0 run, EVR_WIDE_MIN=1 putting the form on every ConvLSTM layer:
    EVR_WIDE=3                      the skewed loop of the 256 x 256 form
    EVR_WIDE=3 EVR_WIDE16_ALT=0     its lock-step loop
    EVR_WIDE=2                      the twin 256 x 128 form
on three shapes of three frames each, nchunks = 4 / 8 / 16 at the three levels:
    24x40 x 3    (test_gpu_wide16.CASES[0]) M = 720 / 180 / 45: a tile mostly past M -- the warm-up piece and the lane exchange meet
                 inactive pixels -- and widths 20 / 10 / 5
    50x70 x 2    (CASES[1]) several tiles, an image boundary inside a 16-pixel block
    32x32 x 4    M = 1024 / 256 / 64: tiles exactly full at two levels, no lane masked, four images inside one tile
Equal bits cannot show which code ran: evr_model_profile_read's "kernel.wide16_tail" row counts the launches with the tail, 3 levels x 3
frames per shape by default and none under EVR_WIDE16_TAIL=0.  The switches are read once per process: one interpreter per variant.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL_ROW = 'kernel.wide16_tail'
# (H, W, sequences, frames, weight seed, voxel seed): the first two are test_gpu_wide16._inputs(0) and (1)
SHAPES = [(24, 40, 3, 3, 160, 16000), (50, 70, 2, 3, 161, 16001), (32, 32, 4, 3, 164, 16004)]
LOOPS = {'skewed': {'EVR_WIDE': '3'}, 'lockstep': {'EVR_WIDE': '3', 'EVR_WIDE16_ALT': '0'}, 'twin': {'EVR_WIDE': '2'}}

_CHILD = r"""
import json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_wide16 as t
from evreal_amd import model, weights
out, launches = {}, {}
for si, (H, W, n, frames, wseed, vseed) in enumerate(json.loads(sys.argv[3])):
    sd, vox = t._sd(wseed), t._voxels(vseed, frames, n, H, W)
    m = model.E2VIDRecurrent(dict(weights.E2VID_KWARGS))
    m.load_state_dict(sd)
    assert m.arith == 'h3', m.arith
    m.reset_states()
    m.profile(sys.argv[4])
    for f in range(frames):
        out[f'{si}.img{f}'] = m(torch.from_numpy(vox[f]).cuda())['image'].cpu().numpy()
    for k, shp in t._state_shapes(H, W, n).items():
        out[f'{si}.{k}'] = m.read_tensor(k).cpu().numpy().reshape(shp)
    launches[str(si)] = {r['name']: int(r['launches']) for r in m.profile_read()}
    m.profile(None)
np.savez(sys.argv[2], **out)
json.dump(launches, open(sys.argv[2] + '.json', 'w'))
"""


def _child(tmp_path, name, env):
    out = str(tmp_path / f'{name}.npz')
    drop = ('EVR_MFMA16', 'EVR_WIDE', 'EVR_WIDE_MIN', 'EVR_WIDE16_ALT', 'EVR_WIDE16_TAIL', 'EVR_ARITH', 'EVR_FP32', 'EVR_LIB')
    e = {k: v for k, v in os.environ.items() if k not in drop}
    e.update(env)
    r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, out, json.dumps(SHAPES), TAIL_ROW], env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (name, r.stdout[-2000:] + r.stderr[-3000:])
    z = np.load(out)
    return {k: z[k] for k in z.files}, json.load(open(out + '.json'))


@pytest.fixture(scope='module')
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp('wide16_tail')


@pytest.fixture(scope='module', params=sorted(LOOPS))
def runs(request, tmp):
    env = dict(LOOPS[request.param], EVR_WIDE_MIN='1')
    return {'tail': _child(tmp, request.param + '_tail', env), 'plain': _child(tmp, request.param + '_plain', dict(env, EVR_WIDE16_TAIL='0'))}


def test_tail_equals_the_untrimmed_kernel_bit_for_bit(runs):
    import test_gpu_wide16 as t
    a, b = runs['tail'][0], runs['plain'][0]
    want = {f'{si}.{k}' for si, s in enumerate(SHAPES) for k in [f'img{f}' for f in range(s[3])] + list(t._state_shapes(*s[:3]))}
    assert set(a) == want and set(b) == want, (sorted(set(a) ^ want), sorted(set(b) ^ want))
    bad = []
    for k in sorted(want):
        assert a[k].dtype == np.float32 and a[k].shape == b[k].shape and np.isfinite(a[k]).all(), k
        assert float(np.abs(a[k]).max()) > 0.0, k            # (a run that wrote nothing would compare equal too)
        ndiff = int((a[k].view(np.uint32) != b[k].view(np.uint32)).sum())
        print(f'  {k:8s} {a[k].size:8d} values, {ndiff} differ, max|x| {float(np.abs(a[k]).max()):.3e}')
        if ndiff:
            bad.append((k, ndiff, float(np.abs(a[k].astype(np.float64) - b[k]).max())))
    assert not bad, bad


def test_the_tail_is_what_ran(runs):
    for si, s in enumerate(SHAPES):
        frames = s[3]
        tail, plain = runs['tail'][1][str(si)], runs['plain'][1][str(si)]
        print(f'  shape {si}: launches with the tail {tail} (default), {plain} (EVR_WIDE16_TAIL=0)')
        assert tail == {TAIL_ROW: 3 * frames}, tail          # three ConvLSTM levels per frame, nothing else in the filtered read-out
        assert plain == {TAIL_ROW: 0}, plain
