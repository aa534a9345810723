"""The value- and remainder-dependent branches of csrc/prepost.hip and the tile edges of csrc/metrics.hip, against numpy.

a. evr_percentile_normalize: the frames of tests/pct_paths.py (tests/test_pct_paths_cpu.py holds them to the branches they are meant
   to take: fast, list overflow, bracket missed low / high, the launcher's four-pass conditions) through the default one-pass kernel
   with its fallback, the paired four-pass kernel (EVR_PCT_FAST=0) and the unpaired one (EVR_PCT_FAST=0 EVR_PCT_PAIR=0).  The
   switches are read once per process: one interpreter per variant.  A selection is exact or it is wrong: 'robust' and 'standard' are
   held to numpy's bits, a frame inside a batch to the bits of the frame alone, and the three kernels to each other's bits.
b. evr_event_tensor_normalize as a stand-alone call on several windows at once: the blockIdx.y stride into the statistics, the scalar
   tail (B*H*W % 4 != 0), the misaligned base, an empty and a one-event window between ordinary ones.
c. evr_metrics where the last tile is narrower than the 5-pixel halo, is exactly one tile, or is smaller than a tile, down to the
   12 x 12 minimum, and its refusal of anything smaller.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pct_paths as pp
from golden_inputs import gen_events

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-6          # expf against numpy's exp ('exprobust'); fp32 sums against fp64 ones (event tensor): tests/test_gpu_prepost.py

# ------------------------------------------------------------------------------------------------- a. percentile normalisation
NORMS = ('robust', 'standard', 'exprobust')
VARIANTS = [('default', {}), ('fourpass', {'EVR_PCT_FAST': '0'}), ('unpaired', {'EVR_PCT_FAST': '0', 'EVR_PCT_PAIR': '0'})]


def _on_device(a, misaligned=False):
    """`a` on the GPU, contiguous; misaligned: based one float past a 16-B boundary."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.empty(a.size + 4, dtype=torch.float32, device='cuda')
    assert buf.data_ptr() % 16 == 0
    d = buf[1:1 + a.size] if misaligned else buf[:a.size]
    d = d.view(a.shape)
    d.copy_(torch.from_numpy(a))
    assert d.is_contiguous() and (d.data_ptr() % 16 != 0) == bool(misaligned)
    return d


def _batches():
    """Cases of one shape and alignment, launched together: fast and fallback work-groups side by side in one grid."""
    groups = {}
    for c in pp.cases():
        groups.setdefault((c['frame'].shape, c['misaligned']), []).append(c)
    return [g for g in groups.values() if len(g) > 1]


def _run_pct_table():
    """(in the child) every case alone and inside its batch -> {'<name>.<norm>': [H, W], 'batch.<name>.<norm>': [H, W]}"""
    from evreal_amd.prepost import post_process_normalization
    out = {}
    for c in pp.cases():
        for norm in NORMS:
            if norm != 'exprobust' or c['exp']:
                d = _on_device(c['frame'][None], c['misaligned'])
                out[f"{c['name']}.{norm}"] = post_process_normalization(d, norm).cpu().numpy()[0]
    for g in _batches():
        for norm in NORMS:
            d = _on_device(np.stack([c['frame'] for c in g]), g[0]['misaligned'])
            got = post_process_normalization(d, norm).cpu().numpy()
            for i, c in enumerate(g):
                out[f"batch.{c['name']}.{norm}"] = got[i]
    torch.cuda.synchronize()
    return out


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
import test_gpu_prepost_edges as t
np.savez(sys.argv[2], **t._run_pct_table())
"""


def _child(tmp_path, name, env):
    out = str(tmp_path / f'{name}.npz')
    e = {k: v for k, v in os.environ.items() if k not in ('EVR_PCT_FAST', 'EVR_PCT_PAIR')}
    e.update(env)
    r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, out], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:] + r.stderr[-3000:])
    z = np.load(out)
    return {k: z[k] for k in z.files}


def _same_bits(a, b):
    """NaN where the other has NaN, and the same bits everywhere else"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def test_percentile_paths_vs_numpy(tmp_path):
    from oracle import prepost as op
    # one of the batches holds every kind of work-group of the one-pass kernel
    assert any({'fast', 'overflow', 'miss_low', 'miss_high'} <= {c['branch'][q] for c in g for q in (1.0, 99.0)} for g in _batches())
    runs = {}
    for name, env in VARIANTS:          # one after the other; the first child that does not exit 0 ends the test
        runs[name] = _child(tmp_path, name, env)
    want = {}
    with np.errstate(invalid='ignore', divide='ignore'):
        for c in pp.cases():
            for norm in NORMS:
                if norm != 'exprobust' or c['exp']:
                    want[f"{c['name']}.{norm}"] = op.post_process_normalization(c['frame'].copy(), norm)
    bad = []
    for vname, got in runs.items():
        assert set(want) <= set(got)
        for k, w in want.items():
            g = got[k]
            assert w.dtype == np.float32 and g.dtype == np.float32
            if k.endswith('.exprobust'):
                assert np.isfinite(w).all(), k
                ok = bool(np.isfinite(g).all()) and np.allclose(g, w, rtol=TOL, atol=TOL)
            else:
                ok = np.array_equal(g, w, equal_nan=True)          # bit exact (as test_post_process_normalization_goldens)
            if not ok:
                with np.errstate(invalid='ignore'):
                    bad.append((vname, k, 'vs numpy', int((~np.isclose(g, w, rtol=TOL, atol=TOL, equal_nan=True)).sum())))
        for k in got:                   # a frame of a batch == the same frame alone (n = 1), to the bit
            if k.startswith('batch.'):
                alone = k[len('batch.'):]
                ref = got[alone] if alone in got else None
                if ref is None:         # ('exprobust' of a case whose percentiles coincide: no reference, but still one answer)
                    continue
                if not _same_bits(got[k], ref):
                    bad.append((vname, k, 'batch vs alone'))
    base = runs[VARIANTS[0][0]]
    for vname, _ in VARIANTS[1:]:       # the three kernels select the same order statistics: same bits, same NaN
        assert set(runs[vname]) == set(base)
        for k in base:
            if not _same_bits(runs[vname][k], base[k]):
                bad.append((vname, k, 'vs default kernel'))
    assert not bad, bad
    # the table's degenerate frames do what numpy does: 0 / 0 everywhere
    assert np.isnan(base['const.robust']).all() and np.isnan(base['const.standard']).all()


# ------------------------------------------------------------------------------------------------- b. event-tensor normalisation
def _window_batch(seed, n, B, H, W):
    """[n, B, H, W] sparse voxel grids: window 1 all zeros, one window with a single non-zero (window 3; the last one of a shorter
    batch), and the first cells of every other window non-zero (a write past a window's end lands on them)."""
    from evreal_amd import synth
    v = synth.sparse_voxels(seed, n, B, H, W, density=0.1)
    rng = np.random.default_rng(seed + 1)
    single = 3 if n > 3 else n - 1
    for w in range(n):
        if w == 1:
            v[w] = 0
        elif w == single:
            v[w] = 0
            v[w].reshape(-1)[0] = np.float32(0.75)
        else:
            v[w].reshape(-1)[:4] = (1.0 + rng.random(4)).astype(np.float32) * np.array([1, -1, 1, -1], np.float32)
    return np.ascontiguousarray(v, dtype=np.float32), single


def _check_windows(got, vin, single, what):
    from oracle import prepost as op
    assert got.shape == vin.shape and got.dtype == np.float32
    for w in range(vin.shape[0]):
        want = op.normalize_event_tensor(vin[w])
        np.testing.assert_allclose(got[w], want, rtol=TOL, atol=TOL, err_msg=f'{what}: window {w}')
        assert np.array_equal(got[w] == 0, want == 0), f'{what}: zero mask of window {w}'
    assert np.array_equal(got[1].view(np.uint32), vin[1].view(np.uint32)), f'{what}: the empty window is not left alone'
    assert not got[single].any(), f'{what}: the one-value window (std clamp) is not all zero'


def _hand_stats(v):
    v64 = v.reshape(v.shape[0], -1).astype(np.float64)
    return np.stack([v64.sum(1), (v64 ** 2).sum(1), (v64 != 0).sum(1).astype(np.float64)], 1)


# n, B, H, W.  The apply kernel's grid is min(128, ceil(vol / 4 / 256)) blocks of 256 threads, four values per thread and trip:
#   vol = 315     scalar tail (vol % 4 = 3), two blocks, the last thread group holds 3 values
#   vol = 1920    vector path
#   vol = 7755    vol % 4 = 3, eight blocks, the tail in the last one
#   vol = 131215  the smallest kind of volume that takes a second grid-stride trip (> 128 * 256 * 4 values), vol % 4 = 3: the tail
#                 is reached in the second trip
WINDOW_SHAPES = [(5, 5, 7, 9), (5, 5, 16, 24), (3, 5, 33, 47), (3, 5, 163, 161)]
WINDOW_IDS = ['vol%d' % (s[1] * s[2] * s[3]) for s in WINDOW_SHAPES]


@pytest.mark.parametrize('shape', WINDOW_SHAPES, ids=WINDOW_IDS)
def test_event_tensor_windows_vs_oracle(shape):
    from evreal_amd.prepost import normalize_event_tensor
    n, B, H, W = shape
    vin, single = _window_batch(700 + H, n, B, H, W)
    results = {}
    # partials path (the kernel reduces), then statistics handed over as [n, 3] float64 {sum, sum of squares, non-zeros}
    results['partials'] = normalize_event_tensor(_on_device(vin)).cpu().numpy()
    st = torch.from_numpy(_hand_stats(vin)).cuda()
    results['stats'] = normalize_event_tensor(_on_device(vin), stats=st).cpu().numpy()
    if (B * H * W) % 4 == 0:
        results['partials, misaligned'] = normalize_event_tensor(_on_device(vin, misaligned=True)).cpu().numpy()
        results['stats, misaligned'] = normalize_event_tensor(_on_device(vin, misaligned=True), stats=st).cpu().numpy()
    for what, got in results.items():
        _check_windows(got, vin, single, what)
    # every window of the batch == the same window normalised alone, to the bit
    for w in range(n):
        alone = normalize_event_tensor(_on_device(vin[w:w + 1])).cpu().numpy()[0]
        assert np.array_equal(alone.view(np.uint32), results['partials'][w].view(np.uint32)), f'partials: window {w} alone'
        alone = normalize_event_tensor(_on_device(vin[w:w + 1]), stats=st[w:w + 1].clone()).cpu().numpy()[0]
        assert np.array_equal(alone.view(np.uint32), results['stats'][w].view(np.uint32)), f'stats: window {w} alone'
    # the elementwise arithmetic does not depend on the path: vector and scalar loops give the same bits
    for what in results:
        if 'misaligned' in what:
            assert np.array_equal(results[what].view(np.uint32), results[what.split(',')[0]].view(np.uint32)), what


@pytest.mark.parametrize('shape', WINDOW_SHAPES, ids=WINDOW_IDS)
def test_event_tensor_windows_with_voxelizer_stats(shape):
    """The grid built from events by the tensorizer, normalised with the statistics the tensorizer hands over: an empty window
    (index 1) and a one-event window between ordinary ones."""
    from evreal_amd.prepost import normalize_event_tensor
    from evreal_amd.voxel import Voxelizer
    n, B, H, W = shape
    single = 3 if n > 3 else n - 1
    sizes = [0 if w == 1 else 1 if w == single else 40 + 7 * w for w in range(n)]
    ev, offs = [], [0]
    for w, k in enumerate(sizes):
        ev.append(gen_events(900 + 10 * H + w, k, W, H))
        offs.append(offs[-1] + k)
    x, y, t, p = (np.concatenate(a) for a in zip(*ev))
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st = torch.zeros((n, 3), dtype=torch.float64, device='cuda')
    grid = Voxelizer().voxelize(d(x), d(y), d(t), d(p), d(np.asarray(offs, dtype=np.int64)), B, (H, W), stats=st)
    vin = grid.cpu().numpy()
    nnz = (vin.reshape(n, -1) != 0).sum(1)
    assert nnz[1] == 0 and nnz[single] == 1 and all(nnz[w] > 8 for w in range(n) if w not in (1, single)), nnz
    assert np.array_equal(st.cpu().numpy()[:, 2], nnz.astype(np.float64))
    got = normalize_event_tensor(grid, stats=st).cpu().numpy()
    _check_windows(got, vin, single, 'voxelizer stats')
    for w in range(n):
        alone = normalize_event_tensor(_on_device(vin[w:w + 1]), stats=st[w:w + 1].clone()).cpu().numpy()[0]
        assert np.array_equal(alone.view(np.uint32), got[w].view(np.uint32)), f'window {w} alone'


# ------------------------------------------------------------------------------------------------- c. MSE / SSIM at the tile edges
# tiles are 16 x 64 outputs with a 5-pixel reflected halo
METRIC_SHAPES = [(12, 12),     # the minimum, a 2 x 2 SSIM map: the reflection is longer than what the tile holds of the frame
                 (16, 64),     # exactly one tile
                 (17, 65),     # one pixel into a second tile on both axes
                 (21, 69),     # the last tile exactly as wide as the halo
                 (20, 68),     # one less than the halo
                 (40, 130)]


def _check_metrics(H, W):
    from evreal_amd.prepost import Metrics
    from oracle import metrics as om
    rng = np.random.default_rng(1000 * H + W)
    n = 3
    yy, xx = np.mgrid[0:H, 0:W]
    ref = np.stack([0.5 + 0.4 * np.sin(xx / (7.0 + i) + i) * np.cos(yy / (9.0 + i)) for i in range(n)]).astype(np.float32)
    img = (ref + 0.15 * rng.standard_normal(ref.shape)).astype(np.float32)   # exceeds [0,1] -> exercises the clip
    img[0] = ref[0]
    assert np.abs(img - 0.5).max() > 0.5
    out = Metrics()(torch.from_numpy(img).cuda(), torch.from_numpy(ref).cuda()).cpu().numpy()
    for i in range(n):
        a, b = om.clip01(img[i]), om.clip01(ref[i])
        print(f'{H}x{W} pair {i}: mse {out[i, 0]:.12e} (oracle {om.mse(a, b):.12e})  ssim {out[i, 1]:.9f} (oracle {om.ssim(a, b):.9f})')
        assert abs(out[i, 0] - om.mse(a, b)) <= 1e-12 + 1e-9 * om.mse(a, b), (i, out[i, 0], om.mse(a, b))
        assert abs(out[i, 1] - om.ssim(a, b)) <= 2e-6, (i, out[i, 1], om.ssim(a, b))
    assert out[0, 0] == 0.0 and abs(out[0, 1] - 1.0) < 1e-6
    assert out[1, 0] > 1e-3 and out[1, 1] < 0.9          # (the noisy pairs are not degenerate)


@pytest.mark.parametrize('shape', METRIC_SHAPES, ids=['%dx%d' % s for s in METRIC_SHAPES])
def test_mse_ssim_tile_edges_vs_oracle(shape):
    _check_metrics(*shape)


def _refused(H, W, which=3):
    """evr_metrics on H x W frames -> (return code, message); asserts that a refusal touched neither output nor workspace"""
    from evreal_amd import lib as _lib
    L = _lib.load()
    img = torch.rand((1, 12, 12), device='cuda')
    out = torch.full((1, 2), -7.0, dtype=torch.float64, device='cuda')
    ws = torch.full((4096,), 0x5A, dtype=torch.uint8, device='cuda')
    rc = L.evr_metrics(_lib.ptr(img), _lib.ptr(img), 1, H, W, which, 1, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    msg = L.evr_last_error() if rc else b''
    torch.cuda.synchronize()
    if rc:
        assert (out.cpu().numpy() == -7.0).all() and (ws.cpu().numpy() == 0x5A).all(), 'a refused call wrote something'
    return rc, msg, out.cpu().numpy()


def test_metrics_refuses_11x11():
    """12 x 12 is the smallest frame SSIM is served for: at 11 x 11 the 11-tap window and the 5-pixel crop leave one pixel of the map.
    EVR_ERR_INVALID, and neither the output nor the workspace is touched; likewise where only one side is too short."""
    for H, W in [(11, 11), (11, 12), (12, 11), (10, 64), (16, 10)]:
        rc, msg, _ = _refused(H, W)
        assert rc == -1 and b'11x11' in msg, (H, W, rc, msg)     # EVR_ERR_INVALID
    assert _refused(12, 12)[0] == 0
    # MSE alone has no window: the same frame is served
    rc, _, out = _refused(11, 11, which=1)
    assert rc == 0 and out[0, 0] == 0.0
