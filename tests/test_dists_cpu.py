"""The DISTS oracle (tests/dists_ref.py) held to facts that do not depend on it, and the host-side pieces of the GPU metric (schema,
synthetic weights, the folded one-channel conv1_1 with per-channel constants, the L2 pool's geometry, the size limit, the tracker
without a weights file, the tracker's routing of the new table entry).  No GPU."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dists_ref as R
import lpips_vgg_ref as RV
from conftest import ROOT

VGG16_CFG = [64, 64, 'P', 128, 128, 'P', 256, 256, 256, 'P', 512, 512, 512, 'P', 512, 512, 512]      # torchvision, without the last pool
TAPS = (3, 8, 15, 22, 29)


@pytest.fixture(scope='module')
def sd():
    from evreal_amd import weights
    return weights.synth_dists_state_dict(seed=3)


@pytest.fixture(scope='module')
def scored(sd):
    """fp64 totals and stage distances of the GPU tests' inputs at 37 x 53 and 16 x 16, computed once."""
    return {hw: R.frame_pairs(*hw) + R.dists(sd, *R.frame_pairs(*hw)) for hw in ((37, 53), (16, 16))}


class L2Pool(nn.Module):
    """The published L2pooling: a depthwise 3x3 convolution of the squares with the normalised outer product of (0.5, 1, 0.5),
    stride 2, padding 1."""

    def __init__(self, channels):
        super().__init__()
        a = torch.tensor([0.5, 1.0, 0.5], dtype=torch.float64)
        g = a[:, None] * a[None, :]
        self.conv = nn.Conv2d(channels, channels, kernel_size=3, stride=2, padding=1, groups=channels, bias=False).double()
        with torch.no_grad():
            self.conv.weight.copy_((g / g.sum())[None, None].repeat(channels, 1, 1, 1))

    def forward(self, x):
        return torch.sqrt(self.conv(x ** 2) + 1e-12)


def _sequential(sd):
    layers, cin = [], 3
    for v in VGG16_CFG:
        if v == 'P':
            layers.append(L2Pool(cin))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=False)]
            cin = v
    net = nn.Sequential(*layers).double()
    by_index = {int(k.split('.')[1]): k.rsplit('.', 1)[0] for k in sd if k.startswith('stage')}
    assert sorted(by_index) == [i for i, m in enumerate(net) if isinstance(m, nn.Conv2d)]
    with torch.no_grad():
        for i, name in by_index.items():
            net[i].weight.copy_(torch.as_tensor(sd[name + '.weight']).double())
            net[i].bias.copy_(torch.as_tensor(sd[name + '.bias']).double())
    return net


def test_oracle_equals_a_literal_vgg16_sequential_with_l2_pools(sd, scored):
    img, ref, total, stages = scored[(37, 53)]
    net = _sequential(sd)
    assert len(net) == 30

    def sets(a):
        x = R.three_channels(a, torch.float64)
        outs, h = [x], R.normalise(x)
        with torch.no_grad():
            for i, m in enumerate(net):
                h = m(h)
                if i in TAPS:
                    outs.append(h)
        return outs

    f0, f1 = sets(img), sets(ref)
    assert [f.shape[1] for f in f0] == list(R.CHANNELS) and sum(R.CHANNELS) == 1475
    assert [tuple(f.shape[2:]) for f in f0] == [(37, 53), (37, 53), (19, 27), (10, 14), (5, 7), (3, 4)]      # ceil at every pool
    want_t, want_s = R.stage_distances(f0, f1, torch.as_tensor(sd['alpha']).double(), torch.as_tensor(sd['beta']).double())
    np.testing.assert_allclose(stages, want_s.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(total, want_t.numpy(), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(stages.sum(axis=(1, 2)), total, rtol=0, atol=1e-12)      # the distances add up to the score


def test_identical_frames_score_zero(sd):
    _, ref = R.frame_pairs(21, 34)
    total, stages = R.dists(sd, ref[:3], ref[:3])
    assert np.abs(total).max() <= 1e-12 and np.abs(stages).max() <= 1e-12


def test_the_mean_and_std_buffers_of_a_state_dict_are_used(sd):
    img, ref = R.frame_pairs(16, 16)
    with_buffers = dict(sd, mean=np.array(R.MEAN, np.float32).reshape(1, 3, 1, 1), std=np.array(R.STD, np.float32).reshape(1, 3, 1, 1))
    np.testing.assert_allclose(R.dists(with_buffers, img, ref)[0], R.dists(sd, img, ref)[0], rtol=0, atol=1e-6)
    other = dict(with_buffers, mean=np.array([0.2, 0.3, 0.4], np.float32))
    assert np.abs(R.dists(other, img, ref)[0] - R.dists(sd, img, ref)[0])[1:].min() > 1e-4


def _fold_cases(sd):
    from evreal_amd import weights
    vgg = weights.synth_lpips_vgg_state_dict(seed=3)
    mean, std, shift, scale = np.array(R.MEAN), np.array(R.STD), np.array(RV.SHIFT), np.array(RV.SCALE)
    yield ('dists', sd['stage1.0.weight'], sd['stage1.0.bias'], 1.0 / std, -mean / std,
           lambda g: R.normalise(R.three_channels(g, torch.float64)))
    yield 'lpips', vgg['net.slice1.0.weight'], vgg['net.slice1.0.bias'], 2.0 / scale, (-1.0 - shift) / scale, lambda g: RV.prep(g, torch.float64)


def test_folded_one_channel_conv1_1_equals_the_three_channel_convolution(sd):
    """What fold_scaling_layer (csrc/lpips_host.h) and vgg_conv1_1_kernel (csrc/vgg_backbone.h) compute for x_c = a_c g + b_c:
    wg = sum_c w a_c, wb = sum_c w b_c, and per pixel bias + sum_t inside[t] (wg[t] g[t] + wb[t]) -- a padded tap contributes 0, not
    wb.  DISTS: a = 1/std, b = -mean/std; LPIPS: a = 2/scale, b = (-1 - shift)/scale.  numpy fp64, borders and corners included."""
    rng = np.random.default_rng(11)
    for tag, w, b, ca, cb, prep in _fold_cases(sd):
        w, b = np.asarray(w, np.float64), np.asarray(b, np.float64)
        wg, wb = np.einsum('ocyx,c->yxo', w, ca), np.einsum('ocyx,c->yxo', w, cb)
        for g in (rng.random((5, 7)), np.zeros((4, 4)), np.ones((3, 3)), rng.random((1, 1))):
            H, W = g.shape
            got = np.zeros((H, W, 64))
            for y in range(H):
                for x in range(W):
                    acc = b.copy()
                    for ky in range(3):
                        for kx in range(3):
                            yy, xx = y + ky - 1, x + kx - 1
                            if 0 <= yy < H and 0 <= xx < W:
                                acc += wg[ky, kx] * g[yy, xx] + wb[ky, kx]
                    got[y, x] = acc
            want = F.conv2d(prep(g[None].astype(np.float64)), torch.as_tensor(w), torch.as_tensor(b), padding=1)[0].permute(1, 2, 0).numpy()
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, err_msg=tag)
            if H >= 3 and W >= 3:      # interior pixels: the padding term is a constant that moves into the bias
                np.testing.assert_allclose(got[1, 1], b + wb.sum(axis=(0, 1)) + (wg * g[0:3, 0:3, None]).sum(axis=(0, 1)), rtol=0, atol=1e-12)


def test_l2_pool_is_ceil_mode_and_pads_with_zeros():
    rng = np.random.default_rng(3)
    for h, w in ((1, 1), (2, 3), (5, 7), (8, 8), (19, 27)):
        x = torch.from_numpy(rng.random((1, 2, h, w)))
        y = R.l2pool(x)
        assert tuple(y.shape[2:]) == ((h + 1) // 2, (w + 1) // 2)
        sq = np.zeros((2, h + 2, w + 2))
        sq[:, 1:h + 1, 1:w + 1] = x[0].numpy() ** 2
        k = np.array([1.0, 2.0, 1.0])
        k = np.outer(k, k) / 16
        for oy in range(y.shape[2]):
            for ox in range(y.shape[3]):       # the window centred on (2oy, 2ox); the last one of an odd side hangs over the far edge too
                want = np.sqrt((sq[:, 2 * oy:2 * oy + 3, 2 * ox:2 * ox + 3] * k).sum(axis=(1, 2)) + 1e-12)
                np.testing.assert_allclose(y[0, :, oy, ox].numpy(), want, rtol=1e-14, atol=0)
    one = R.l2pool(torch.ones(1, 1, 3, 3, dtype=torch.float64))[0, 0].numpy()      # corner windows see 9/16 of the weight
    np.testing.assert_allclose(one, np.sqrt(np.full((2, 2), 9.0 / 16) + 1e-12), rtol=1e-14)


def test_schema_shapes(sd):
    from evreal_amd import weights
    s = weights.dists_schema()
    convs = [k for k in s if k.endswith('.weight')]
    assert len(convs) == 13 and len(s) == 13 * 2 + 2
    cin = 3
    for (st, idxs), co in zip(R.STAGES, R.CHANNELS[1:]):
        for i in idxs:
            assert s[f'stage{st}.{i}.weight'] == (co, cin, 3, 3) and s[f'stage{st}.{i}.bias'] == (co,)
            cin = co
    assert s['alpha'] == s['beta'] == (1, 1475, 1, 1)
    assert (sd['alpha'] > 0).all() and (sd['beta'] > 0).all()
    w = sd['alpha'].astype(np.float64).sum() + sd['beta'].astype(np.float64).sum()
    share = (sd['alpha'][0, :3].astype(np.float64).sum() + sd['beta'][0, :3].astype(np.float64).sum()) / w
    assert share >= 0.01, share                # the input's feature set stays visible
    assert all(sd[k].shape == tuple(v) and sd[k].dtype == np.float32 for k, v in s.items())
    again = weights.synth_dists_state_dict(seed=3)
    assert all(np.array_equal(sd[k], again[k]) for k in sd)
    vgg = weights.synth_lpips_vgg_state_dict(seed=3)      # the same gain: the trunk's activations stay in the same range
    assert abs(np.abs(sd['stage3.12.weight']).max() / np.abs(vgg['net.slice3.12.weight']).max() - 1) < 0.01


def test_synthetic_weights_keep_every_stage_distance_alive(scored):
    """Non-vacuity of the GPU tests: at 37 x 53 each of the twelve stage distances of pairs 1 and 2 is at least 1e-4 -- a stage the
    kernels got wrong cannot hide below the tolerance; the terms that are zero by construction are exactly zero."""
    _, _, total, stages = scored[(37, 53)]
    assert stages[1:3].min() >= 1e-4, stages[1:3]
    assert np.abs(stages[0]).max() <= 1e-12 and abs(total[0]) <= 1e-12
    assert stages[3, 0, 1] == 0.0 and stages[3, 0, 0] >= 1e-4      # ones against zeros: no texture, a real mean difference
    assert stages[3, 1:].min() >= 1e-4
    _, _, _, small = scored[(16, 16)]
    assert np.array_equal(small[:, 5, 1], np.zeros(4))             # relu5_3 of a 16 x 16 frame is one pixel: no variance
    assert small[1:, 5, 0].min() >= 1e-4 and small[1:, 1:5].min() > 0


def test_too_small_agrees_with_the_c_entry_point():
    from evreal_amd.lpips import DISTS
    src = open(os.path.join(ROOT, 'evreal_amd', 'csrc', 'dists.hip')).read()
    assert int(re.search(r'constexpr int MIN_SIDE = (\d+);', src).group(1)) == DISTS.MIN_SIDE == R.MIN_SIDE == 16
    assert 'EVR_REQUIRE(H >= MIN_SIDE && W >= MIN_SIDE, "evr_dists: image %dx%d too small' in src
    for H, W in ((16, 16), (15, 40), (40, 15), (17, 16), (8, 40), (31, 33)):
        why = DISTS.too_small(H, W)
        assert (why is None) == (H >= 16 and W >= 16), (H, W)
        assert why is None or f'{H}x{W}' in why


@pytest.mark.parametrize('route', ['register_metric', 'pyiqa', 'nobody'])
def test_tracker_without_weights_leaves_the_name_to_its_other_providers(tmp_path, monkeypatch, capsys, route):
    """Without a weights file `dists` goes on to register_metric / pyiqa / `Unknown metric` as before; a metric of that name that is
    not this project's GPU metric is booked and finalized like any other (finalize() must not look for the handle's range counter)."""
    from evreal_amd import build, eval_metrics as em
    build.build(verbose=False)
    monkeypatch.setenv(em.DISTS_WEIGHTS_ENV, str(tmp_path / 'nowhere.pth'))
    monkeypatch.setattr(em.EvalMetricsTracker, '_dists_cache', [False, None])
    monkeypatch.setattr(em, '_pyiqa_factory', SimpleNamespace(list_of_metrics=[]))

    class Stub(em.BaseMetric):
        def calculate(self, img, ref):
            return float(np.abs(img - ref).mean())

    if route == 'register_metric':
        monkeypatch.setitem(em._REGISTRY, 'dists', lambda: Stub('dists'))
    elif route == 'pyiqa':
        fn = lambda imgs, refs: (imgs - refs).abs().mean(dim=(1, 2, 3))
        fake = type('FakePyiqa', (), {'list_of_metrics': ['dists'],
                                      'get_metric': lambda self, name: em._QueuedIqaMetric(name, False, fn)})()
        monkeypatch.setattr(em, '_pyiqa_factory', fake)
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['dists'], has_reference_frames=True)
    out = capsys.readouterr().out
    assert out.count('dists: no weights at') == 1
    assert em.EvalMetricsTracker._dists_cache == [True, None]
    if route == 'nobody':
        assert t.metrics == [] and 'Unknown metric dists' in out
        t.finalize(0)
        return
    assert [m.name for m in t.metrics] == ['dists'] and not getattr(t.metrics[0], 'on_gpu', False)
    rng = np.random.default_rng(1)
    imgs, refs = torch.from_numpy(rng.random((6, 20, 24), dtype=np.float32)), torch.from_numpy(rng.random((6, 20, 24), dtype=np.float32))
    t.update_batch(list(range(6)), imgs, refs, [0.01 * i for i in range(6)], None)
    t.finalize(5)
    want = [float((a - b).abs().mean()) for a, b in zip(imgs, refs)]
    lines = open(tmp_path / 'out' / 'dists.txt').read().splitlines()
    assert [int(l.split()[0]) for l in lines] == list(range(6))
    assert all(abs(float(l.split()[1]) - w) <= 1.01e-5 for l, w in zip(lines, want))
    assert abs(t.get_mean_scores()['dists'] - np.mean(want)) <= 1e-6


# ---- the tracker's routing with the new table entry: tests/test_metric_table_cpu.py's stand-ins, for a name list with `dists` ----
NAMES = ['mse', 'ssim', 'psnr', 'ms_ssim', 'gmsd', 'piqe', 'lpips', 'lpips-vgg', 'dists', 'niqe', 'brisque']
BASE = {'mse': 10, 'ssim': 20, 'psnr': 30, 'ms_ssim': 40, 'gmsd': 50, 'piqe': 60, 'lpips': 70, 'lpips-vgg': 80, 'dists': 110, 'niqe': 90,
        'brisque': 100}
BATCHES = (3, 2, 1)
UNUSED = 1e6        # gmsd's second column (the mean GMS): no file may hold it
IN_BATCH = [j for n in BATCHES for j in range(n)]       # a frame's position in the batch it arrived in


class _StandIn:
    """A wrapper's call shape (flags, no `ref` for a no-reference metric, `out=` or a returned tensor) with base + arange(n) in
    every column."""

    def __init__(self, *bases, returns_first=False):
        self.bases, self.returns_first, self.calls = bases, returns_first, []

    def __call__(self, img, ref=None, clip=True, out=None, **flags):
        assert clip is True
        self.calls.append(flags)
        n = img.shape[0]
        rows = torch.stack([b + torch.arange(n, dtype=torch.float64) for b in self.bases], dim=1)
        rows = rows[:, 0] if len(self.bases) == 1 else rows
        if out is not None:
            out.copy_(rows)
            rows = out
        return rows[:, 0] if self.returns_first else rows       # (GMSD writes two columns and returns the first)

    def saturation(self):
        return 0


def _tracker(tmp_path, monkeypatch, sub):
    from evreal_amd import build, eval_metrics as em
    build.build(verbose=False)
    for env in (em.FR_METRICS_ENV, em.PIQE_ENV, em.GMSD_ENV):
        monkeypatch.delenv(env, raising=False)
    monkeypatch.setattr(em, '_pyiqa_factory', SimpleNamespace(list_of_metrics=[]))
    T = em.EvalMetricsTracker
    stand = {k: _StandIn(*b, returns_first=k == 'gmsd') for k, b in dict(
        gpu=(10, 20), fr=(30, 40), gmsd=(50, UNUSED), piqe=(60,), lpips=(70,), lpips_vgg=(80,), dists=(110,), niqe=(90,),
        brisque=(100,)).items()}
    for k in ('lpips', 'lpips_vgg', 'dists', 'niqe', 'brisque', 'piqe'):
        monkeypatch.setattr(T, f'_{k}_cache', [True, stand[k]])
    t = T(output_dir=str(tmp_path / sub), quan_eval_metric_names=list(NAMES), has_reference_frames=True)
    t._gpu, t._fr, t._gmsd = stand['gpu'], stand['fr'], stand['gmsd']
    return t, stand


def _feed(t, H, W):
    k = 0
    for n in BATCHES:
        idx = list(range(k, k + n))
        t.update_batch(idx, torch.zeros((n, H, W)), torch.zeros((n, H, W)), [0.01 * i for i in idx], None)
        k += n
    t.finalize(k - 1)


def _lines(t, name):
    return open(f'{t.output_dir}/{name}.txt').read().splitlines()


def test_the_dists_column_reaches_its_own_file(tmp_path, monkeypatch, capsys):
    t, stand = _tracker(tmp_path, monkeypatch, 'out')
    assert [m.name for m in t.metrics] == NAMES and t.wants_precomputed() == NAMES
    _feed(t, 200, 200)
    means = t.get_mean_scores()
    for name in NAMES:
        assert _lines(t, name) == ['{} {:.5f}'.format(i, BASE[name] + j) for i, j in enumerate(IN_BATCH)], name
        assert means[name] == pytest.approx(BASE[name] + np.mean(IN_BATCH), abs=1e-12), name
    for k, s in stand.items():
        assert len(s.calls) == len(BATCHES), k          # one launch set per batch
    out = capsys.readouterr().out
    assert 'Exception in metric' not in out and 'Unknown metric' not in out


def test_dists_is_refused_on_small_frames_and_its_neighbours_are_full(tmp_path, monkeypatch, capsys):
    t, stand = _tracker(tmp_path, monkeypatch, 'small')
    _feed(t, 8, 200)
    out = capsys.readouterr().out
    means = t.get_mean_scores()
    for name in NAMES:
        if name in ('ms_ssim', 'lpips-vgg', 'dists'):
            assert _lines(t, name) == [] and means[name] == -1, name
            assert out.count(f'Exception in metric {name}: ') == 1
        else:
            assert _lines(t, name) == ['{} {:.5f}'.format(i, BASE[name] + j) for i, j in enumerate(IN_BATCH)], name
    assert out.count('Exception in metric') == 3
    assert stand['dists'].calls == [] and stand['lpips_vgg'].calls == []      # refused from the shape: never launched
