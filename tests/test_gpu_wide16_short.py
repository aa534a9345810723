"""192-pixel tiles in the skewed 256 x 256 ConvLSTM gate kernel (csrc/conv.hip conv3x3_wide16_kernel<2, true, true, SHORT = true> with the
plan's tile map, csrc/conv_route.cpp wide16_tile_map) against the uniform map of 256-pixel tiles in grid order (EVR_WIDE16_SHORT=0).

A pixel's accumulators see the same MFMAs in the same order whichever tile and wave hold them, and the cell update and the H2 split are
untouched, so the results are equal bit for bit: the images of every frame and the final h / c of all three levels, compared as uint32,
zero differing words allowed.  EVR_WIDE=3 EVR_WIDE_MIN=1 puts the form on every ConvLSTM layer; the rule itself keeps out of launches
under an explicit EVR_WIDE_MIN, so the two forced maps are what runs here:
    EVR_WIDE16_SHORT=all       every tile 192 pixels: a wave's three pixel blocks at a stride of 48, set D never touched
    EVR_WIDE16_SHORT=last=1    the last M tile of every XCD range 192 pixels, the others 256: both tile heights in one launch
on four shapes of three frames each, nchunks = 4 / 8 / 16 at the three levels (M = pixels per level):
    24x40 x 3    (test_gpu_wide16.CASES[0]) M = 720 / 180 / 45: under `all` tiles end inside an image (192, 384, 576 of 240-pixel images), the
                 last one past M; at the two deep levels fewer than eight tiles, so XCD ranges are empty and their blocks leave at once
    50x70 x 2    (CASES[1]) M = 2016 / 504 / 126: several tiles per range under last=1 (256 + 192), M ends inside a 16-pixel block (126)
    32x32 x 4    M = 1024 / 256 / 64: uniform tiles exactly full at two levels; under `all` 1024 = 5.33 tiles
    16x24 x 2    M = 192 / 48 / 12: one M tile at every level -- exactly one full 192-pixel tile at the first -- seven of eight ranges empty
Equal bits cannot show which code ran: evr_model_profile_read's "kernel.wide16_short" row counts the launches whose map held a short
tile, 3 levels x 3 frames per shape under both forced maps and none under EVR_WIDE16_SHORT=0.  The switches are read once per process:
one interpreter per variant.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT_ROW = 'kernel.wide16_short'
# (H, W, sequences, frames, weight seed, voxel seed): the first two are test_gpu_wide16._inputs(0) and (1)
SHAPES = [(24, 40, 3, 3, 160, 16000), (50, 70, 2, 3, 161, 16001), (32, 32, 4, 3, 164, 16004), (16, 24, 2, 3, 165, 16005)]
VARIANTS = {'off': '0', 'all': 'all', 'last1': 'last=1'}

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
    drop = ('EVR_MFMA16', 'EVR_WIDE', 'EVR_WIDE_MIN', 'EVR_WIDE16_ALT', 'EVR_WIDE16_TAIL', 'EVR_WIDE16_SHORT', 'EVR_ARITH', 'EVR_FP32', 'EVR_LIB')
    e = {k: v for k, v in os.environ.items() if k not in drop}
    e.update(env)
    r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, out, json.dumps(SHAPES), SHORT_ROW], env=e, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (name, r.stdout[-2000:] + r.stderr[-3000:])
    z = np.load(out)
    return {k: z[k] for k in z.files}, json.load(open(out + '.json'))


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('wide16_short')
    return {name: _child(tmp, name, {'EVR_WIDE': '3', 'EVR_WIDE_MIN': '1', 'EVR_WIDE16_SHORT': v}) for name, v in VARIANTS.items()}


@pytest.mark.parametrize('variant', ['all', 'last1'])
def test_short_tiles_equal_the_uniform_map_bit_for_bit(runs, variant):
    import test_gpu_wide16 as t
    a, b = runs[variant][0], runs['off'][0]
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


def test_the_short_tiles_are_what_ran(runs):
    for si, s in enumerate(SHAPES):
        frames = s[3]
        got = {name: runs[name][1][str(si)] for name in VARIANTS}
        print(f'  shape {si}: launches with a short tile {got}')
        assert got['all'] == {SHORT_ROW: 3 * frames}, got     # three ConvLSTM levels per frame, nothing else in the filtered read-out
        assert got['last1'] == {SHORT_ROW: 3 * frames}, got   # (last=1: the first range's last tile is short whatever M is)
        assert got['off'] == {SHORT_ROW: 0}, got
