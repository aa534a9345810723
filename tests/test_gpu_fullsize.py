"""GPU parity at the sizes BASELINE.json's configs run at: every comparison is the HIP
path through the C ABI against the torch-CPU oracle on the same events, 1e-4 absolute per pixel (north_star).

  * 100-frame recurrence, 346x260 (pads to 352x264), 8 different sequences advanced together -- the band kernels'
    natural dispatch (the one bench.py times), event-tensor normalization fused, ConvLSTM states checked at the end;
  * E2VID at 640x480 (north_star's second sensor), E2VID+ and HyperE2VID layouts at 346x260;
  * FireNet with the shipped checkpoint at 240x180 (pads to 240x192) over k_events windows of a synthetic sequence;
  * ColorNet at 970x624 (half resolution 485x312 pads to 488x312; full resolution to 976x624) and its behaviour on
    odd sensor sides (BS-ERGB's 970x625): the reference raises there (model/model.py:81-99, see the test).
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_npz
from golden_inputs import gen_events

pytestmark = pytest.mark.gpu
# (default arithmetic = three f16 products, fp32-grade: 1e-5 per pixel; EVR_ARITH=mx6|mx and the exact-fp32 mode: north_star's 1e-4)
ARITH = 'fp32' if (os.environ.get('EVR_FP32') or os.environ.get('EVR_ARITH') == 'fp32') else (os.environ.get('EVR_ARITH') or 'h3')
IMG_ATOL = float(os.environ.get('EVR_TEST_IMG_ATOL', '1e-5' if ARITH == 'h3' else '1e-4'))
OKEYS = ['num_bins', 'base_num_channels', 'num_encoders', 'num_residual_blocks', 'kernel_size', 'norm',
         'use_upsample_conv', 'recurrent_block_type', 'final_activation']


def _pair(kw, seed, fixed=None):
    """(HIP model, oracle) with the same deterministic synthetic weights."""
    from evreal_amd import model, weights
    from oracle import model as omod
    sd = weights.synth_state_dict(weights.unet_recurrent_schema(**kw), seed=seed, fixed=fixed)
    m = model.E2VIDRecurrent(kw); m.load_state_dict(sd)
    okw = {k: kw[k] for k in OKEYS}
    okw['use_dynamic_decoder'] = kw.get('use_dynamic_decoder', False)
    o = omod.UNetRecurrentOracle({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, **okw)
    return m, o


def _windows(seeds, n, W, H):
    """Events of len(seeds) windows, concatenated, + window offsets."""
    ev = [gen_events(s, n, W, H) for s in seeds]
    cat = [np.concatenate([e[i] for e in ev]) for i in range(4)]
    offs = np.arange(len(seeds) + 1, dtype=np.int64) * n
    return ev, cat, offs


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(m, o, H, W, num_encoders, frames, n_seq, n_events, seed0, normalize=True, check_states=False, oracle_seqs=None, o64=None):
    """oracle_seqs: the sequences replayed through the CPU oracle (default: all; the GPU always advances all n_seq together).
    o64: the same oracle in float64, replayed on the first of them; then the return value is (worst, report) where report lists, per
    compared tensor, (name, e_gpu, e_32, max|T_64|) with e_gpu = max|T_gpu - T_64| and e_32 = max|T_32 - T_64| (tests/test_gpu_wino.py)."""
    from evreal_amd.voxel import Voxelizer
    from oracle import prepost as op, voxel as ov
    crop = op.CropParams(W, H, num_encoders)
    vz = Voxelizer()
    st = torch.zeros((n_seq, 3), dtype=torch.float64, device='cuda')
    m.reset_states(); o.reset_states()
    sel = list(range(n_seq)) if oracle_seqs is None else list(oracle_seqs)
    worst = 0.0
    report = []
    if o64 is not None:
        o64.reset_states()

    def cmp64(name, got, t32, t64):
        report.append((name, float(np.abs(got.astype(np.float64) - t64).max()), float(np.abs(t32.astype(np.float64) - t64).max()),
                       float(np.abs(t64).max())))
    for f in range(frames):
        ev, cat, offs = _windows([seed0 + 1000 * f + s for s in range(n_seq)], n_events, W, H)
        g = vz.voxelize(_d(cat[0]), _d(cat[1]), _d(cat[2]), _d(cat[3]), _d(offs), 5, (H, W), stats=st)
        img = m(g, stats=st if normalize else None)['image'].cpu().numpy()
        v = np.stack([ov.events_to_voxel(*ev[s], 5, (H, W)) for s in sel])
        if normalize:
            v = np.stack([op.normalize_event_tensor(v[s:s + 1])[0] for s in range(len(sel))])
        with torch.no_grad():
            want = crop.crop(o(torch.from_numpy(crop.pad(v))).numpy())
        err = float(np.abs(img[sel] - want).max())
        worst = max(worst, err)
        assert err < IMG_ATOL, (f, err)
        if o64 is not None:
            with torch.no_grad():
                want64 = crop.crop(o64(torch.from_numpy(crop.pad(v[:1]))).numpy())
            cmp64(f'img{f}', img[sel[0]:sel[0] + 1], want[:1], want64)
    if check_states:
        for i in range(num_encoders):
            shp = (n_seq,) + tuple(o.states[i][0].shape[1:])
            h = m.read_tensor(f'h{i}').cpu().numpy().reshape(shp)[sel]
            c = m.read_tensor(f'c{i}').cpu().numpy().reshape(shp)[sel]
            np.testing.assert_allclose(h, o.states[i][0].numpy(), rtol=2e-4, atol=5e-5, err_msg=f'h{i}')
            np.testing.assert_allclose(c, o.states[i][1].numpy(), rtol=2e-4, atol=5e-5, err_msg=f'c{i}')
            if o64 is not None:
                cmp64(f'h{i}', h[:1], o.states[i][0].numpy()[:1], o64.states[i][0].numpy())
                cmp64(f'c{i}', c[:1], o.states[i][1].numpy()[:1], o64.states[i][1].numpy())
    return worst if o64 is None else (worst, report)


def test_drift_100_frames_346x260_8_sequences():
    """SURVEY section 7's condition for split precision: >= 100 recurrent steps, full size, on the kernels the bench runs."""
    from evreal_amd import weights
    torch.set_num_threads(min(32, torch.get_num_threads()))
    m, o = _pair(dict(weights.E2VID_KWARGS), seed=21)
    # (the mode variants of tests/test_gpu_modes.py replay sequences 0 and 7 through the oracle: EVR_TEST_DRIFT_ORACLE_SEQS=0,7)
    # (default: sequences 0, 2, 5, 7 -- the GPU advances all 8; EVR_TEST_DRIFT_ORACLE_SEQS=0,1,2,3,4,5,6,7 replays every one)
    sel = [int(x) for x in os.environ.get('EVR_TEST_DRIFT_ORACLE_SEQS', '0,2,5,7').split(',') if x] or None
    worst = _run(m, o, 260, 346, 3, frames=100, n_seq=8, n_events=15000, seed0=40000, check_states=True, oracle_seqs=sel)
    print(f'100-frame drift, 8 sequences: worst per-pixel error {worst:.2e}')


def test_exact_fp32_twin_winograd_346x260():
    """The library's exact-fp32 twin (what a saturated group of sequences is re-run on) computes its ConvLSTM gate and residual
    convolutions as Winograd F(2x2, 3x3) since round 6 (csrc/wino.hip): 346x260 puts ODD grids under it (132x176, 66x88, 33x44 -- the
    last tile row of 33 rows has one valid output row), 3 sequences make ragged tile blocks.  20 recurrent frames against the oracle at
    north_star's 1e-4; the states at the end.  (tests/test_gpu_modes.py runs the golden suite on this form and on EVR_WINO=0.)"""
    from evreal_amd import weights
    torch.set_num_threads(min(32, torch.get_num_threads()))
    m, o = _pair(dict(weights.E2VID_KWARGS), seed=23)
    twin = m.exact_twin()
    assert twin.arith == 'fp32'
    from oracle import model as omod
    o64 = omod.UNetRecurrentOracle(dict(o.sd), **{k: dict(weights.E2VID_KWARGS)[k] for k in OKEYS}, dtype=torch.float64)
    global IMG_ATOL
    keep, IMG_ATOL = IMG_ATOL, 1e-4
    try:
        worst, report = _run(twin, o, 260, 346, 3, frames=20, n_seq=3, n_events=15000, seed0=70000, check_states=True, o64=o64)
    finally:
        IMG_ATOL = keep
    print(f'exact-fp32 twin (Winograd {os.environ.get("EVR_WINO", "on")}), 20 frames x 3 sequences: worst per-pixel error {worst:.2e}')
    assert worst < 2e-5, worst      # measured 1e-6-class; a wrong tile or weight position is 1e-1
    # sequence 0 against the float64 oracle: e_gpu <= max(8 e_32, 2^-20 max|T_64|), the bound of tests/test_gpu_wino.py
    bad = []
    for name, e_gpu, e_32, s in report:
        print(f'  float64 oracle, sequence 0, {name:6s}: e_gpu {e_gpu:.3e}  e_32 {e_32:.3e}  ratio {e_gpu / max(e_32, 1e-300):.2f}')
        if not e_gpu <= max(8.0 * e_32, 2.0 ** -20 * s):
            bad.append((name, e_gpu, e_32, s))
    assert len(report) == 20 + 6 and not bad, bad


def test_one_sequence_split_k_100_frames_346x260():
    """The reference's own operating point -- ONE sequence, batch 1 (eval.py:72) -- runs the deep layers (12 tiles of 128 pixels at
    33 x 44) through the split-K forms of the band kernels (conv.hip launch_band / launch_band_prog: up to four blocks per tile, partial
    sums through the model's workspace, conv_ksplit_epilogue_kernel): 100 recurrent frames at 346x260 against the oracle, states at
    the end.  EVR_TEST_SPLITK_FRAMES shortens it for the EVR_KSPLIT=0 pass below."""
    from evreal_amd import weights
    torch.set_num_threads(min(32, torch.get_num_threads()))
    frames = int(os.environ.get('EVR_TEST_SPLITK_FRAMES', '100'))
    m, o = _pair(dict(weights.E2VID_KWARGS), seed=21)
    worst = _run(m, o, 260, 346, 3, frames=frames, n_seq=1, n_events=15000, seed0=120000, check_states=True)
    print(f'{frames}-frame drift, 1 sequence (split K {os.environ.get("EVR_KSPLIT", "default")}): worst per-pixel error {worst:.2e}')


def test_one_sequence_without_split_k():
    """the same one-sequence run with the split switched off (EVR_KSPLIT=0 is read once per process: a fresh interpreter),
    so that both forms are held to the same oracle at the same gate."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EVR_KSPLIT='0', EVR_TEST_SPLITK_FRAMES='12')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-m', 'gpu', '-p', 'no:cacheprovider',
                        'tests/test_gpu_fullsize.py::test_one_sequence_split_k_100_frames_346x260'],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_split_k_run_count_is_clamped_to_what_the_epilogue_sums():
    """EVR_KSPLIT / EVR_KSPLIT_SMALL are user switches with no documented upper bound, and the wide split-K epilogue sums at
    most 8 partial sets: with 16 the main kernel used to write sixteen and the epilogue silently summed eight.  conv.hip ksplit_cap now
    clamps both to 8: the one-sequence run (every deep layer splits) must still match the oracle."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EVR_KSPLIT='16', EVR_KSPLIT_SMALL='16', EVR_TEST_SPLITK_FRAMES='12')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', '-m', 'gpu', '-p', 'no:cacheprovider',
                        'tests/test_gpu_fullsize.py::test_one_sequence_split_k_100_frames_346x260'],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_recurrence_at_the_64_sequence_dispatch():
    """The recurrence at the dispatch bench.py times: 64 sequences advanced together (the 256 x 128 / 256 x 256-tile ConvLSTM kernels, the
    twin-form decoders with the fused prediction epilogue), sequence 37 replayed through the CPU oracle at every frame; final ConvLSTM
    states checked.  400 frames by default (the suite's time budget); EVR_TEST_RECURRENCE_FRAMES=1000 is the run recorded in
    profiles/r04_recurrence_1000.txt: worst per-pixel error 2.38e-07 over 1000 frames.  (Round 3 ran this from tools/drift_run.py only.)"""
    from evreal_amd import weights
    torch.set_num_threads(min(32, torch.get_num_threads()))
    frames = int(os.environ.get('EVR_TEST_RECURRENCE_FRAMES', '400'))
    m, o = _pair(dict(weights.E2VID_KWARGS), seed=21)
    worst = _run(m, o, 260, 346, 3, frames=frames, n_seq=64, n_events=15000, seed0=90000, check_states=True, oracle_seqs=[37])
    print(f'{frames}-frame recurrence, 64 sequences: worst per-pixel error {worst:.2e}')


def test_e2vid_640x480_vs_oracle():
    from evreal_amd import weights
    m, o = _pair(dict(weights.E2VID_KWARGS), seed=22)
    _run(m, o, 480, 640, 3, frames=2, n_seq=2, n_events=50000, seed0=50000)


def test_e2vid_plus_layout_346x260():
    from evreal_amd import weights
    m, o = _pair(dict(weights.E2VID_PLUS_KWARGS), seed=23)
    _run(m, o, 260, 346, 3, frames=2, n_seq=2, n_events=15000, seed0=60000, normalize=False)


def test_hyper_layout_346x260():
    z = load_npz('e2vid_hyper_seq.npz')
    kw = json.loads(bytes(z['kwargs']).decode())
    fixed = {k[6:]: z[k] for k in z.files if k.startswith('fixed.')}      # the reference's Fourier-Bessel table
    m, o = _pair(kw, seed=24, fixed=fixed)
    _run(m, o, 260, 346, 3, frames=3, n_seq=2, n_events=15000, seed0=70000, normalize=False)


def test_firenet_real_weights_240x180_k_events(tmp_path):
    """BASELINE config 3: FireNet (shipped checkpoint) on a 240x180 sequence, k_events windowing through the
    sequence reader (events resident in HBM, many windows per launch), normalization on (config/method/FireNet.json)."""
    from evreal_amd import model, synth
    from evreal_amd.dataset import MemMapDataset
    from oracle import model as omod, prepost as op, voxel as ov
    w = load_npz('firenet_weights.npz')
    sd = {k: w[k] for k in w.files}
    m = model.FireNet_legacy(unet_kwargs=dict(num_bins=5, recurrent_block_type='convgru', base_num_channels=16,
                                              num_residual_blocks=2, kernel_size=3, norm='none'))
    m.load_state_dict(sd)
    o = omod.FireNetLegacyOracle({k: torch.from_numpy(v) for k, v in sd.items()})
    H, W, K = 180, 240, 7500
    synth.write_sequence(str(tmp_path / 's'), 3, 12 * K + 100, 1.0e6, W, H, 50.0)
    ds = MemMapDataset(str(tmp_path / 's'), num_bins=5, voxel_method={'method': 'k_events', 'k': K, 'sliding_window_w': 0})
    assert tuple(ds.sensor_resolution) == (H, W) and len(ds) == 12
    grid, stats = ds.voxel_batch(list(range(12)))
    fh = ds.filehandle
    crop = op.CropParams(W, H, 4)
    m.reset_states()
    for i in range(12):
        img = m(grid[i:i + 1], stats=stats[i:i + 1])['image'].cpu().numpy()
        xs, ys, tf, ps = synth.window_events_f32(np.asarray(fh['t']), np.asarray(fh['xy']), np.asarray(fh['p']), i * K, (i + 1) * K)
        v = ov.events_to_voxel(xs, ys, tf, ps, 5, (H, W))
        assert np.array_equal(grid[i].cpu().numpy().view(np.uint32), v.view(np.uint32)), i      # tensorizer: bit exact
        with torch.no_grad():
            want = crop.crop(o(torch.from_numpy(crop.pad(op.normalize_event_tensor(v[None])))).numpy())
        assert float(np.abs(img - want).max()) < IMG_ATOL, i


_ROWS_SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from conftest import load_npz
from evreal_amd import model
w = load_npz('firenet_weights.npz')
H, W, n = int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
m = model.FireNet_legacy(unet_kwargs=dict(num_bins=5, recurrent_block_type='convgru', base_num_channels=16,
                                          num_residual_blocks=2, kernel_size=3, norm='none'))
m.load_state_dict({k: w[k] for k in w.files})
g = torch.Generator().manual_seed(5)
outs = []
m.reset_states()
for i in range(3):
    v = (torch.randn((n, 5, H, W), generator=g) * (torch.rand((n, 5, H, W), generator=g) < 0.2)).cuda()
    outs.append(m(v)['image'].cpu().numpy())
np.save(sys.argv[2], np.stack(outs))
"""


@pytest.mark.parametrize('H,W,n', [(180, 240, 24), (260, 346, 12), (100, 131, 40)])
def test_firenet_row_kernel_is_bit_identical_to_the_tile_kernel(tmp_path, H, W, n):
    """Round 6: launches big enough to fill the chip take conv3x3_c16_rows_kernel (128-column strips walked row by row, every input
    row fetched once) instead of conv3x3_c16_kernel (128 linear pixels, three shifted bands).  Per pixel both run the same MFMA
    sequence, so three recurrent FireNet steps (shipped checkpoint; batches of 24 x 240x180, 12 x 346x260 -- three strips, the last
    ragged -- and 40 x 131x100 -- padded to 112 rows, a ragged second strip) must agree BIT FOR BIT: the default selection, the row
    kernel forced with the other step heights, and EVR_C16_ROWS=0."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    got = {}
    for name, env in [('tile', {'EVR_C16_ROWS': '0'}), ('default', {}), ('rows', {'EVR_C16_ROWS': '2'}),
                      ('rows_alt', {'EVR_C16_ROWS': '2', 'EVR_C16_ROWS_1': '2', 'EVR_C16_ROWS_2': '1'})]:
        out = str(tmp_path / f'{name}.npy')
        r = subprocess.run([sys.executable, '-c', _ROWS_SCRIPT, root, out, str(H), str(W), str(n)], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        got[name] = np.load(out)
    assert np.isfinite(got['tile']).all() and float(np.abs(got['tile']).max()) > 0
    for name in ('default', 'rows', 'rows_alt'):
        assert np.array_equal(got[name].view(np.uint32), got['tile'].view(np.uint32)), name


def test_colornet_970x624_streams_vs_oracle():
    """BS-ERGB-sized colour pass (even crop of 970x625): the four half-resolution streams (485x312 -> 488x312) and the
    full-resolution stream (970x624 -> 976x624) against the oracle run stream by stream, as model/model.py:85-99 does."""
    from evreal_amd import model, weights
    from oracle import color as oc, prepost as op
    kw = dict(weights.E2VID_PLUS_KWARGS)
    m, o = _pair(kw, seed=25)
    net = model.ColorNet(m)
    H, W = 624, 970
    ev = gen_events(81000, 50000, W, H)
    from oracle import voxel as ov
    v = ov.events_to_voxel(*ev, 5, (H, W))[None]
    out = net(_d(v))
    planes = out['planes'][0].cpu().numpy(); gray = out['gray'][0, 0].cpu().numpy()
    split = oc.bayer_split(v)[0]                                     # [4,B,312,485]
    ch, cf = op.CropParams(W // 2, H // 2, 3), op.CropParams(W, H, 3)
    assert (ch.pad(split[:1]).shape[-2:], cf.pad(v).shape[-2:]) == ((312, 488), (624, 976))
    with torch.no_grad():
        for c in range(4):
            o.reset_states()
            want = ch.crop(o(torch.from_numpy(ch.pad(split[c:c + 1]))).numpy())[0, 0]
            assert float(np.abs(planes[c] - want).max()) < IMG_ATOL, c
        o.reset_states()
        want = cf.crop(o(torch.from_numpy(cf.pad(v))).numpy())[0, 0]
    assert float(np.abs(gray - want).max()) < IMG_ATOL
    assert out['image'].shape == (1, H, W, 3) and out['image'].dtype == torch.uint8


def test_colornet_odd_sides_raise_like_the_reference():
    """The reference's ColorNet cannot run an odd sensor side: the R/G rows `0::2` keep ceil(H/2) rows while the crop
    is built for int(H/2) (model/model.py:81-90), and the first skip connection raises "The size of tensor a must
    match the size of tensor b" (probed with the reference class at 97x128, 96x129 and 125x194).  BASELINE config 5's
    970x625 therefore needs an even crop there too; here the boundary raises with that explanation, never truncates."""
    from evreal_amd import lib as L, model, weights
    kw = dict(weights.E2VID_PLUS_KWARGS)
    sd = weights.synth_state_dict(weights.unet_recurrent_schema(**kw), seed=2)
    base = model.E2VIDRecurrent(kw); base.load_state_dict(sd)
    net = model.ColorNet(base)
    for H, W in [(97, 128), (96, 129)]:
        with pytest.raises(L.EvrError, match='even'):
            net(torch.zeros((1, 5, H, W), device='cuda'))


def test_spade_e2vid_346x260_vs_oracle():
    """SPADE-E2VID at 346x260 (pads to 352x264): two different sequences advanced together, three frames, the cropper's
    explicit padding included in the first frame's min/max rewrite."""
    from evreal_amd import model, weights
    from evreal_amd.voxel import Voxelizer
    from oracle import model as omod, prepost as op, voxel as ov
    sd = weights.synth_state_dict(weights.spade_e2vid_schema(), seed=26)
    m = model.SpadeE2vid(); m.load_state_dict(sd)
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if np.asarray(v).dtype.kind == 'f'}
    oracles = [omod.SpadeE2vidOracle(tsd), omod.SpadeE2vidOracle(tsd)]
    H, W = 260, 346
    crop = op.CropParams(W, H, 3)
    vz = Voxelizer()
    m.reset_states()
    for f in range(3):
        ev, cat, offs = _windows([90000 + 1000 * f + s for s in range(2)], 15000, W, H)
        g = vz.voxelize(_d(cat[0]), _d(cat[1]), _d(cat[2]), _d(cat[3]), _d(offs), 5, (H, W))
        img = m(g)['image'].cpu().numpy()
        for s in range(2):
            v = ov.events_to_voxel(*ev[s], 5, (H, W))[None]
            with torch.no_grad():
                want = crop.crop(oracles[s](torch.from_numpy(crop.pad(v))).numpy())
            assert float(np.abs(img[s:s + 1] - want).max()) < IMG_ATOL, (f, s)


def test_etnet_346x260_vs_oracle():
    """ET-Net at 346x260 (pads to 352x264: 33 x 44 = 1452 tokens per scale, 23 key tiles with a ragged tail), two
    different sequences advanced together, two frames."""
    from evreal_amd import model, weights
    from evreal_amd.voxel import Voxelizer
    from oracle import model as omod, prepost as op, voxel as ov
    sd = weights.synth_state_dict(weights.etnet_schema(norm=None), seed=27)
    m = model.EITR({'num_bins': 5, 'norm': None}); m.load_state_dict(sd)
    tsd = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if np.asarray(v).dtype.kind == 'f'}
    oracles = [omod.ETNetOracle(tsd), omod.ETNetOracle(tsd)]
    H, W = 260, 346
    crop = op.CropParams(W, H, 3)
    vz = Voxelizer()
    m.reset_states()
    for f in range(2):
        ev, cat, offs = _windows([95000 + 1000 * f + s for s in range(2)], 15000, W, H)
        g = vz.voxelize(_d(cat[0]), _d(cat[1]), _d(cat[2]), _d(cat[3]), _d(offs), 5, (H, W))
        img = m(g)['image'].cpu().numpy()
        for s in range(2):
            v = ov.events_to_voxel(*ev[s], 5, (H, W))[None]
            with torch.no_grad():
                want = crop.crop(oracles[s](torch.from_numpy(crop.pad(v))).numpy())
            assert float(np.abs(img[s:s + 1] - want).max()) < IMG_ATOL, (f, s)
