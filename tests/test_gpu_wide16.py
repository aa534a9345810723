"""The ConvLSTM gate kernel on 16x16x32 MFMAs (csrc/conv.hip conv3x3_wide16_kernel, h3 arithmetic) against a float64 oracle and against
its 32x32x16 form (EVR_MFMA16=0).

Both forms multiply the same f16 halves and accumulate in fp32; they differ only in summation order (one K = 32 instruction where the
other has two of K = 16), which cannot systematically double the error.  So for the images of every frame and the final h / c of every
level, from the same inputs,

    e16 = max|T_16 - T_64|  <=  max(2 * e32, REL * max|T_64|)        e32 = max|T_32x32 - T_64|

with T_64 = oracle.model.UNetRecurrentOracle in float64 and REL = 2^-20 (tests/test_gpu_wino.py), and every image within the h3 image
gate of 1e-5 of T_64.  EVR_WIDE_MIN=1 lets the small shapes reach the wide kernels; EVR_WIDE=2 / 3 force the twin (256 x 128 tiles, two
blocks per CU) and the 256 x 256 form on every ConvLSTM layer.  The switches are read once per process: one interpreter per variant.

Measured on the MI355X (both forms of EVR_WIDE give the same figures: the tile changes, the summation order does not), worst
e16 / e32 over the tensors of a case: 24x40 x 3: 1.30 (c1), 50x70 x 2: 1.19 (h2), 180x240 x 3: 1.11 (c2), 260x346 x 2: 1.14 (img1);
smallest 0.81.  e16 is 0.9e-7 .. 1.9e-7 on images (gate 1e-5), 1.3e-7 .. 2.4e-7 on h and 2.4e-7 .. 4.6e-7 on c.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL = 2.0 ** -20
IMAGE_GATE = 1e-5
OKEYS = ['num_bins', 'base_num_channels', 'num_encoders', 'num_residual_blocks', 'kernel_size', 'norm', 'use_upsample_conv',
         'recurrent_block_type', 'final_activation']
# (H, W, n_seq, frames).  Gate-layer grids are the padded size / 2, / 4, / 8 and M = n_seq * rows * cols:
#   24x40 x 3:   12x20, 6x10, 3x5 -- M = 720, 180, 45: no multiple of 256 (one tile is mostly past the end), widths 20 / 10 / 5 are no
#                multiple of 16, and 16-pixel blocks straddle image rows and the three images
#   50x70 x 2:   28x36, 14x18, 7x9 -- M = 2016, 504, 126: several tiles, the image boundary inside a 16-pixel block at / 8 (63 = 3 * 16 + 15)
#   180x240 x 3: 92x120, 46x60, 23x30 -- widths 120 / 60 / 30 (8-, 4- and 2-aligned only), M % 256 != 0 at every level
#   260x346 x 2: the headline size (132x176, 66x88, 33x44), two sequences: M = 46464 = 181.5 tiles at / 2, image 1 starts inside tile 90
# Three frames: the cell state and h written by the new epilogue are read back by the next frame's launches, twice.
CASES = [(24, 40, 3, 3), (50, 70, 2, 3), (180, 240, 3, 3), (260, 346, 2, 3)]


def _sd(seed):
    from evreal_amd import weights
    return weights.synth_state_dict(weights.unet_recurrent_schema(**weights.E2VID_KWARGS), seed=seed)


def _voxels(seed, frames, n_seq, H, W):
    from evreal_amd import synth
    v = np.stack([synth.sparse_voxels(seed + 97 * s, frames, 5, H, W, density=0.1) for s in range(n_seq)], 1)
    return np.ascontiguousarray(v, dtype=np.float32)


def _inputs(ci):
    H, W, n, frames = CASES[ci]
    return _sd(160 + ci), _voxels(16000 + ci, frames, n, H, W)


def _state_shapes(H, W, n):
    return {f'{s}{i}': (n, 64 << i, (H + 7) // 8 * 4 >> i, (W + 7) // 8 * 4 >> i) for s in 'hc' for i in range(3)}


def _gpu_run(sd, vox, H, W):
    """Images of every frame and the final ConvLSTM states of a default (h3) model."""
    from evreal_amd import model, weights
    m = model.E2VIDRecurrent(dict(weights.E2VID_KWARGS))
    m.load_state_dict(sd)
    assert m.arith == 'h3', m.arith
    m.reset_states()
    out = {}
    for f in range(vox.shape[0]):
        out[f'img{f}'] = m(torch.from_numpy(vox[f]).cuda())['image'].cpu().numpy()
    for k, shp in _state_shapes(H, W, vox.shape[1]).items():
        out[k] = m.read_tensor(k).cpu().numpy().reshape(shp)
    return out


def _oracle_run(sd, vox, H, W):
    from evreal_amd import weights
    from oracle import model as omod
    from oracle import prepost as op
    kw = weights.E2VID_KWARGS
    o = omod.UNetRecurrentOracle({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, **{k: kw[k] for k in OKEYS},
                                 dtype=torch.float64)
    crop = op.CropParams(W, H, 3)
    o.reset_states()
    out = {}
    with torch.no_grad():
        for f in range(vox.shape[0]):
            out[f'img{f}'] = crop.crop(o(torch.from_numpy(crop.pad(vox[f])), None).numpy()).astype(np.float64)
    for i, (h, c) in enumerate(o.states):
        out[f'h{i}'] = h.numpy().astype(np.float64); out[f'c{i}'] = c.numpy().astype(np.float64)
    return out


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_wide16 as t
out = {}
for ci, (H, W, n, frames) in enumerate(t.CASES):
    sd, vox = t._inputs(ci)
    out.update({f'{ci}.{k}': v for k, v in t._gpu_run(sd, vox, H, W).items()})
np.savez(sys.argv[2], **out)
"""


def _child(tmp_path, name, env):
    out = str(tmp_path / f'{name}.npz')
    e = {k: v for k, v in os.environ.items() if k not in ('EVR_MFMA16', 'EVR_WIDE', 'EVR_WIDE_MIN', 'EVR_ARITH', 'EVR_FP32')}
    e.update(env)
    r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, out], env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (name, r.stdout[-2000:] + r.stderr[-3000:])
    z = np.load(out)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def refs():
    torch.set_num_threads(min(16, os.cpu_count() or 1, torch.get_num_threads()))
    r64 = {}
    for ci, (H, W, n, frames) in enumerate(CASES):
        sd, vox = _inputs(ci)
        r64.update({f'{ci}.{k}': v for k, v in _oracle_run(sd, vox, H, W).items()})
    return r64


@pytest.mark.parametrize('wide', ['2', '3'], ids=['twin', '256x256'])
def test_wide16_vs_float64_oracle_and_the_32x32_form(tmp_path, refs, wide):
    env = {'EVR_WIDE_MIN': '1', 'EVR_WIDE': wide}
    t16 = _child(tmp_path, 'mfma16', env)
    t32 = _child(tmp_path, 'mfma32', dict(env, EVR_MFMA16='0'))
    report, bad, worst = [], [], {}
    changed = 0
    for k in sorted(refs):
        t64 = refs[k]
        e16 = float(np.abs(t16[k].astype(np.float64) - t64).max())
        e32 = float(np.abs(t32[k].astype(np.float64) - t64).max())
        s = float(np.abs(t64).max())
        lim = max(2.0 * e32, REL * s)
        ok = bool(np.isfinite(t16[k]).all()) and e16 <= lim
        if '.img' in k:
            ok = ok and e16 <= IMAGE_GATE
        changed += int(not np.array_equal(t16[k].view(np.uint32), t32[k].view(np.uint32)))
        ratio = e16 / e32 if e32 > 0 else float('inf')
        ci = k.split('.')[0]
        worst[ci] = max(worst.get(ci, 0.0), ratio)
        report.append(f'  {k:8s} e16 {e16:.3e}  e32 {e32:.3e}  ratio {ratio:5.2f}  max|T| {s:.3e}  limit {lim:.3e}' + ('' if ok else '   <-- FAIL'))
        if not ok:
            bad.append(k)
    print(f'\n[EVR_WIDE={wide}] worst e16 / e32 per case: ' + ', '.join(f'{CASES[int(c)][:3]}: {w:.2f}' for c, w in sorted(worst.items()))
          + '\n' + '\n'.join(report))
    assert not bad, (bad, '\n'.join(report))
    # the two forms sum in a different order: identical bits everywhere would mean the switch selected nothing
    assert changed > 0, 'EVR_MFMA16=0 and the default gave identical bits: the 16x16x32 kernel was not reached'
