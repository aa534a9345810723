"""The exact-fp32 twin's Winograd kernel (csrc/wino.hip) against a float64 oracle.

The twin (_HipModel.exact_twin(), EVR_FP32=1) runs F(2x2, 3x3) in three forms: the ConvLSTM gates (cell update in the epilogue) and the
residual convolutions, the k5 stride-2 encoders in space-to-depth form, and the transposed decoders as four sub-pixel phases (the last with
the 1x1 prediction and the crop fused).  Every compared tensor T is held to

    e_gpu = max|T_gpu - T_64|  <=  max(FACTOR * e_32, REL * max|T_64|)        e_32 = max|T_32 - T_64|

where T_64 is oracle.model.UNetRecurrentOracle in float64 (pinned to the reference class run in float64 by
tests/test_oracle_model.py) and T_32 the same oracle in float32 -- the reference's own arithmetic.  The gate is relative to what fp32
itself leaves on the same inputs, so it holds at unit scale and at 65536x alike, and it sees a loss of a few times the fp32 error that
an absolute gate against the fp32 oracle does not.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# e_gpu <= max(FACTOR * e_32, REL * s): FACTOR is the multiple of the reference's own fp32-vs-float64 spread the IN-layout goldens
# already allow on images (tests/test_gpu_model.py _e2vid); REL keeps the gate meaningful where e_32 happens to be tiny
FACTOR = 8.0
REL = 2.0 ** -20
# EVR_WINO=0 only (the direct implicit GEMM, not the twin's default): each output is ONE serial chain of fp32 MFMA accumulations over all
# 9 x cin terms (4608 at the deepest ConvLSTM) where Winograd sums 16 chains of cin; measured 8.6 x e_32 on c2 at 180x240 (6.6 on the
# twin's Winograd default at worst, 8x8), so the direct form gets twice the factor
FACTOR_DIRECT = 16.0
OKEYS = ['num_bins', 'base_num_channels', 'num_encoders', 'num_residual_blocks', 'kernel_size', 'norm', 'use_upsample_conv',
         'recurrent_block_type', 'final_activation']


def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1, torch.get_num_threads()))


def _sd(seed, rescale=None):
    from evreal_amd import weights
    sd = weights.synth_state_dict(weights.unet_recurrent_schema(**weights.E2VID_KWARGS), seed=seed)
    if rescale is not None:
        sd = weights.rescale_encoder_conv(sd, enc=rescale, K=65536.0)
    return sd


def _voxels(seed, frames, n_seq, H, W, scale=1.0):
    """[frames, n_seq, 5, H, W] fp32: a different sparse sequence per slot."""
    from evreal_amd import synth
    v = np.stack([synth.sparse_voxels(seed + 97 * s, frames, 5, H, W, density=0.1) for s in range(n_seq)], 1)
    return np.ascontiguousarray(v * np.float32(scale), dtype=np.float32)


def _twin(sd, debug=False):
    """The exact-fp32 executor (what exact_twin() builds), optionally with every intermediate kept readable."""
    from evreal_amd import model, weights
    m = model.E2VIDRecurrent(dict(weights.E2VID_KWARGS))
    m.arith_override = 'fp32'
    m.debug_taps = debug
    m.load_state_dict(sd)
    assert m.arith == 'fp32'
    return m


def _oracle(sd, dtype):
    from evreal_amd import weights
    from oracle import model as omod
    kw = weights.E2VID_KWARGS
    return omod.UNetRecurrentOracle({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, **{k: kw[k] for k in OKEYS},
                                    dtype=dtype)


def _tap_sums(taps, states, E=3, R=2):
    """What the library's buffers hold after frame 0 (model.cpp plan_unet): the skip sum of every transposed decoder is fused into the
    epilogue of the layer before it -- the last residual block's buffer holds res{R-1} + h{E-1}, dec{i} (i < E-1) holds dec{i} + h{E-2-i};
    the last decoder's debug copy is its own output (the skip with the head goes into the fused prediction)."""
    out = {f'enc{i}.conv': taps[f'enc{i}.conv'] for i in range(E)}
    for r in range(R):
        out[f'res{r}'] = taps[f'res{r}'] + (states[E - 1][0] if r == R - 1 else 0)
    for i in range(E):
        out[f'dec{i}'] = taps[f'dec{i}'] + (states[E - 2 - i][0] if i < E - 1 else 0)
    return out


def _oracle_run(o, vox, H, W, taps=False):
    from oracle import prepost as op
    crop = op.CropParams(W, H, 3)
    o.reset_states()
    out = {}
    with torch.no_grad():
        for f in range(vox.shape[0]):
            t = {} if (taps and f == 0) else None
            out[f'img{f}'] = crop.crop(o(torch.from_numpy(crop.pad(vox[f])), t).numpy()).astype(np.float64)
            if t is not None:
                out.update({'tap.' + k: v.numpy().astype(np.float64) for k, v in _tap_sums(t, o.states).items()})
    for i, (h, c) in enumerate(o.states):
        out[f'h{i}'] = h.numpy().astype(np.float64); out[f'c{i}'] = c.numpy().astype(np.float64)
    return out


def _gpu_run(m, vox, shapes=None, taps=False):
    """Images of every frame, frame-0 taps (debug models, one sequence), final ConvLSTM states; shapes: the oracle's arrays."""
    m.reset_states()
    out = {}
    for f in range(vox.shape[0]):
        out[f'img{f}'] = m(torch.from_numpy(vox[f]).cuda())['image'].cpu().numpy()
        if taps and f == 0:
            for k in [k for k in shapes if k.startswith('tap.')]:
                out[k] = m.read_tensor(k[4:]).cpu().numpy().reshape(shapes[k].shape)
    for i in range(3):
        for s in 'hc':
            out[f'{s}{i}'] = m.read_tensor(f'{s}{i}').cpu().numpy().reshape(shapes[f'{s}{i}'].shape)
    return out


def _bound(name, got, t32, t64, report, factor=FACTOR):
    """-> (ok, e_gpu, e_32, limit) for one tensor; appends a line to `report`."""
    e_gpu = float(np.abs(got.astype(np.float64) - t64).max())
    e_32 = float(np.abs(t32 - t64).max())
    s = float(np.abs(t64).max())
    lim = max(factor * e_32, REL * s)
    ratio = e_gpu / e_32 if e_32 > 0 else float('inf')
    ok = np.isfinite(got).all() and e_gpu <= lim
    report.append(f'  {name:12s} e_gpu {e_gpu:.3e}  e_32 {e_32:.3e}  ratio {ratio:6.2f}  max|T| {s:.3e}  limit {lim:.3e}'
                  + ('' if ok else '   <-- FAIL'))
    return ok, e_gpu, e_32, lim


def _check(case, got, ref32, ref64, keys=None, factor=FACTOR):
    report, bad, worst = [], [], 0.0
    for k in (keys or sorted(ref64)):
        ok, e_gpu, e_32, _ = _bound(k, got[k], ref32[k], ref64[k], report, factor)
        if e_32 > 0:
            worst = max(worst, e_gpu / e_32)
        if not ok:
            bad.append(k)
    print(f'\n[{case}] worst e_gpu / e_32 = {worst:.2f}\n' + '\n'.join(report))
    assert not bad, (case, bad, '\n'.join(report))
    return worst


# (H, W, n_seq, frames, taps): the grids at /2, /4, /8 after padding to multiples of 8 -- 8x8: 4x4, 2x2, 1x1 (one tile, 3 of its 4
# outputs outside at /8); 8x24: single-row grids; 24x40: 12x20, 6x10, 3x5 (odd); 50x70: padded both ways (crop offsets of the fused
# prediction); 180x240: 23x30 at /8 (odd rows), 3 sequences = 540 items of the /2 gate layer (several strides of the 256 persistent
# blocks); 260x346: 33x44 at /8 -- the headline size, one sequence with every tap.  Sequence counts 1, 3, 5: Mt % 64 != 0 everywhere
# and 64-tile blocks that hold the tiles of several images.
SHAPES = [(8, 8, 5, 3, False), (8, 24, 3, 3, False), (24, 40, 1, 3, True), (24, 40, 5, 3, False), (50, 70, 3, 3, False),
          (50, 70, 1, 2, True), (180, 240, 3, 2, False), (260, 346, 1, 2, True)]


@pytest.mark.parametrize('H,W,n_seq,frames,taps', SHAPES, ids=[f'{h}x{w}_n{n}' + ('_taps' if t else '') for h, w, n, _, t in SHAPES])
def test_winograd_twin_vs_float64_oracle(H, W, n_seq, frames, taps):
    """Images of every frame, the final h/c of every level and (one sequence, debug taps) the frame-0 layer outputs -- enc{i}.conv (the
    space-to-depth form), res{i} (the plain form; the last one holds the fused skip sum), dec{i} (the sub-pixel form; dec0/dec1 hold
    their fused skip sums) -- against the float64 oracle at the bound above."""
    _threads()
    sd = _sd(31 + H + W)
    vox = _voxels(1000 + H * W + n_seq, frames, n_seq, H, W)
    r64 = _oracle_run(_oracle(sd, torch.float64), vox, H, W, taps)
    r32 = _oracle_run(_oracle(sd, torch.float32), vox, H, W, taps)
    got = _gpu_run(_twin(sd, debug=taps), vox, r64, taps)
    _check(f'{H}x{W} n_seq={n_seq}' + (' taps' if taps else ''), got, r32, r64)


def test_sequence_of_a_batch_matches_the_sequence_alone():
    """Sequence s of a 5-sequence batch (24x40: 60 tiles per image at /2, so its tiles share 64-tile blocks with its neighbours) against
    the same sequence run alone: both within the bound of the float64 oracle, and within it of each other."""
    _threads()
    H, W, n, s, frames = 24, 40, 5, 3, 3
    sd = _sd(77)
    vox = _voxels(4242, frames, n, H, W)
    m = _twin(sd)
    batch = _gpu_run(m, vox, _oracle_run(_oracle(sd, torch.float64), vox, H, W))
    one = vox[:, s:s + 1].copy()
    r64 = _oracle_run(_oracle(sd, torch.float64), one, H, W)
    r32 = _oracle_run(_oracle(sd, torch.float32), one, H, W)
    alone = _gpu_run(m, one, r64)
    sel = {k: v[s:s + 1] for k, v in batch.items()}
    _check('batch[3] vs float64', sel, r32, r64)
    _check('alone vs float64', alone, r32, r64)
    bad = []
    for k in sorted(r64):
        d = float(np.abs(sel[k].astype(np.float64) - alone[k]).max())
        lim = max(FACTOR * float(np.abs(r32[k] - r64[k]).max()), REL * float(np.abs(r64[k]).max()))
        if not d <= lim:
            bad.append((k, d, lim))
    assert not bad, bad


MAGNITUDES = [('unit', None, 1.0), ('enc0x65536', 0, 1.0), ('enc1x65536', 1, 1.0), ('enc2x65536', 2, 1.0), ('input300', None, 300.0),
              ('input1e5', None, 1e5)]


@pytest.mark.parametrize('name,enc,scale', MAGNITUDES, ids=[m[0] for m in MAGNITUDES])
def test_twin_at_saturation_magnitudes(name, enc, scale):
    """The twin's real use: activations far outside the split formats' range.  weights.rescale_encoder_conv(enc=e, K=65536) keeps the
    network function and makes encoder e's strided output 65536 times larger (the s2d Winograd form writes large values, the gate layer
    transforms them against x-half weights divided by K); input scales 300 and 1e5 as in test_large_activations_are_reported_not_silent.
    The twin built by exact_twin() of a default model holds the float64 bound and reports no saturated run."""
    from evreal_amd import model, weights
    _threads()
    H, W, n, frames = 24, 40, 2, 4
    sd = _sd(55, rescale=enc)
    vox = _voxels(5150, frames, n, H, W, scale)
    m = model.E2VIDRecurrent(dict(weights.E2VID_KWARGS)); m.load_state_dict(sd)
    twin = m.exact_twin()
    assert twin.arith == 'fp32'
    r64 = _oracle_run(_oracle(sd, torch.float64), vox, H, W)
    r32 = _oracle_run(_oracle(sd, torch.float32), vox, H, W)
    twin.saturation(clear=True)
    got = _gpu_run(twin, vox, r64)
    _check(f'24x40 n_seq=2 {name}', got, r32, r64)
    assert twin.saturation()[0] == 0


# ---------------------------------------------------------------- switches read once per process: one fresh interpreter per variant
_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_wino as t
out = {}
for ci, (H, W, n, frames) in enumerate(t.SWITCH_CASES):
    sd = t._sd(90 + ci)
    vox = t._voxels(9000 + ci, frames, n, H, W)
    shapes = {f'{s}{i}': np.zeros((n, 64 << i, (H + 7) // 8 * 4 >> i, (W + 7) // 8 * 4 >> i)) for s in 'hc' for i in range(3)}
    out.update({f'{ci}.{k}': v for k, v in t._gpu_run(t._twin(sd), vox, shapes).items()})
np.savez(sys.argv[2], **out)
"""
# 24x40 x 3 sequences: odd grids, the one short group of decode()'s 2-D order; 180x240 x 3: several items per persistent block
SWITCH_CASES = [(24, 40, 3, 3), (180, 240, 3, 2)]


def _child(tmp_path, name, env):
    out = str(tmp_path / f'{name}.npz')
    e = {k: v for k, v in os.environ.items() if not k.startswith('EVR_WINO')}
    e.update(env)
    r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, out], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (name, r.stdout[-2000:] + r.stderr[-3000:])
    z = np.load(out)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def switch_refs():
    _threads()
    r32, r64 = {}, {}
    for ci, (H, W, n, frames) in enumerate(SWITCH_CASES):
        sd = _sd(90 + ci)
        vox = _voxels(9000 + ci, frames, n, H, W)
        r64.update({f'{ci}.{k}': v for k, v in _oracle_run(_oracle(sd, torch.float64), vox, H, W).items()})
        r32.update({f'{ci}.{k}': v for k, v in _oracle_run(_oracle(sd, torch.float32), vox, H, W).items()})
    return r32, r64


def test_winograd_switches_hold_the_float64_bound(tmp_path, switch_refs):
    """EVR_WINO=0 (the direct implicit GEMM), EVR_WINO_FASTACT=0 (libm gate activations), EVR_WINO_TCONV=0 EVR_WINO_S2D=0 (decoders and
    encoders direct) and the default: each within the bound (EVR_WINO=0: FACTOR_DIRECT); the Winograd-to-direct and fast-to-libm error
    ratios are printed."""
    r32, r64 = switch_refs
    err = {}
    for name, env in [('default', {}), ('wino0', {'EVR_WINO': '0'}), ('fastact0', {'EVR_WINO_FASTACT': '0'}),
                      ('tconv0_s2d0', {'EVR_WINO_TCONV': '0', 'EVR_WINO_S2D': '0'})]:
        got = _child(tmp_path, name, env)
        _check(name, got, r32, r64, factor=FACTOR_DIRECT if name == 'wino0' else FACTOR)
        err[name] = {k: float(np.abs(got[k].astype(np.float64) - r64[k]).max()) for k in r64}
    for a, b in [('default', 'wino0'), ('default', 'fastact0'), ('default', 'tconv0_s2d0')]:
        rat = {k: err[a][k] / err[b][k] for k in r64 if err[b][k] > 0}
        print(f'{a} / {b} error ratio: median {np.median(list(rat.values())):.2f}, max {max(rat.values()):.2f} ({max(rat, key=rat.get)})')


def test_block_count_and_item_order_are_bit_identical(tmp_path):
    """Every output of a Winograd launch is computed by one item with a fixed K order, whatever the persistent block count or the item
    order: EVR_WINO_BLOCKS=1 and =7 (fewer blocks than XCDs: one item range per block) and EVR_WINO_ORDER=0 (the 1-D order for every
    ncb) must reproduce the default run bit for bit."""
    base = _child(tmp_path, 'default', {})
    assert all(np.isfinite(v).all() for v in base.values())
    for name, env in [('blocks1', {'EVR_WINO_BLOCKS': '1'}), ('blocks7', {'EVR_WINO_BLOCKS': '7'}), ('order0', {'EVR_WINO_ORDER': '0'})]:
        got = _child(tmp_path, name, env)
        diff = [k for k in base if not np.array_equal(got[k].view(np.uint32), base[k].view(np.uint32))]
        assert not diff, (name, diff)
