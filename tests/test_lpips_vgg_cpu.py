"""The LPIPS-VGG oracle (tests/lpips_vgg_ref.py) held to facts that do not depend on it, and the host-side pieces of the GPU
metric (schema, synthetic weights, the folded one-channel conv1_1, the size limit, the tracker without a weights file).  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import lpips_vgg_ref as R

VGG16_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'M', 512, 512, 512, 'M', 512, 512, 512]      # torchvision, without the last pool
TAPS = (3, 8, 15, 22, 29)


@pytest.fixture(scope='module')
def sd():
    from evreal_amd import weights
    return weights.synth_lpips_vgg_state_dict(seed=3)


@pytest.fixture(scope='module')
def scored(sd):
    """fp64 totals and per-layer distances of the GPU tests' inputs at 37 x 53, computed once."""
    img, ref = R.frame_pairs(37, 53)
    return img, ref, R.lpips_vgg(sd, img, ref)


def _sequential(sd, dtype):
    layers, cin = [], 3
    for v in VGG16_CFG:
        if v == 'M':
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=False)]
            cin = v
    net = nn.Sequential(*layers).to(dtype)
    by_index = {int(k.split('.')[2]): k.rsplit('.', 1)[0] for k in sd if k.startswith('net.')}
    assert sorted(by_index) == [i for i, m in enumerate(net) if isinstance(m, nn.Conv2d)]
    with torch.no_grad():
        for i, name in by_index.items():
            net[i].weight.copy_(torch.as_tensor(sd[name + '.weight']).to(dtype))
            net[i].bias.copy_(torch.as_tensor(sd[name + '.bias']).to(dtype))
    return net


def test_oracle_equals_a_literal_vgg16_sequential(sd):
    img, ref = R.frame_pairs(37, 53)
    net = _sequential(sd, torch.float64)
    assert len(net) == 30

    def taps(x):
        outs = []
        with torch.no_grad():
            for i, m in enumerate(net):
                x = m(x)
                if i in TAPS:
                    outs.append(x)
        return outs

    f0, f1 = taps(R.prep(img, torch.float64)), taps(R.prep(ref, torch.float64))
    assert [f.shape[1] for f in f0] == list(R.CHANNELS)
    assert [tuple(f.shape[2:]) for f in f0] == [(37, 53), (18, 26), (9, 13), (4, 6), (2, 3)]
    lins = [torch.as_tensor(sd[f'lin{l}.model.1.weight']).double() for l in range(5)]
    want = R.distances(f0, f1, lins).numpy()
    total, layers = R.lpips_vgg(sd, img, ref)
    np.testing.assert_allclose(layers, want, rtol=1e-12, atol=0)
    np.testing.assert_allclose(total, want.sum(axis=1), rtol=1e-12, atol=0)


def test_identical_frames_score_exactly_zero(sd):
    img, ref = R.frame_pairs(21, 34)
    for dtype in (torch.float64, torch.float32):
        total, layers = R.lpips_vgg(sd, ref, ref, dtype)
        assert np.array_equal(total, np.zeros(len(ref))) and np.array_equal(layers, np.zeros((len(ref), 5)))


def test_schema_shapes(sd):
    from evreal_amd import weights
    s = weights.lpips_vgg_schema()
    convs = [k for k in s if k.endswith('.weight') and k.startswith('net.')]
    assert len(convs) == 13 and len(s) == 13 * 2 + 5
    cin = 3
    for (sl, idxs), co in zip(R.SLICES, R.CHANNELS):
        for i in idxs:
            assert s[f'net.slice{sl}.{i}.weight'] == (co, cin, 3, 3) and s[f'net.slice{sl}.{i}.bias'] == (co,)
            cin = co
    for l, c in enumerate(R.CHANNELS):
        assert s[f'lin{l}.model.1.weight'] == (1, c, 1, 1)
        assert (sd[f'lin{l}.model.1.weight'] >= 0).all()
    assert all(sd[k].shape == tuple(v) and sd[k].dtype == np.float32 for k, v in s.items())
    again = weights.synth_lpips_vgg_state_dict(seed=3)
    assert all(np.array_equal(sd[k], again[k]) for k in sd)


def test_folded_one_channel_conv1_1_equals_the_three_channel_convolution(sd):
    """What csrc/lpips_vgg.hip computes for conv1_1: wg = sum_c w*2/scale_c, wb = sum_c w*(-1 - shift_c)/scale_c, and per pixel
    bias + sum_t inside[t]*(wg[t]*g[t] + wb[t]) -- a padded tap contributes 0, not wb.  numpy fp64, borders and corners included."""
    w = np.asarray(sd['net.slice1.0.weight'], np.float64)      # [64,3,3,3]
    b = np.asarray(sd['net.slice1.0.bias'], np.float64)
    shift, scale = np.array(R.SHIFT), np.array(R.SCALE)
    wg = np.einsum('ocyx,c->yxo', w, 2.0 / scale)
    wb = np.einsum('ocyx,c->yxo', w, (-1.0 - shift) / scale)
    rng = np.random.default_rng(11)
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
        x3 = R.prep(g[None].astype(np.float64), torch.float64)
        want = F.conv2d(x3, torch.as_tensor(w), torch.as_tensor(b), padding=1)[0].permute(1, 2, 0).numpy()
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
        if H >= 3 and W >= 3:      # interior pixels: the padding term is a constant that moves into the bias
            np.testing.assert_allclose(got[1, 1], b + wb.sum(axis=(0, 1)) + (wg * g[0:3, 0:3, None]).sum(axis=(0, 1)), rtol=0, atol=1e-12)


def test_synthetic_weights_keep_every_layer_alive(sd, scored):
    """Non-vacuity of the GPU tests at 37 x 53: every pixel of every tap layer has a non-zero feature norm, and every layer's
    distance is at least 1e-4 on the non-identical pairs -- a layer the kernels got wrong cannot hide below the tolerance."""
    img, ref, (total, layers) = scored
    sd64 = {k: torch.as_tensor(v).double() for k, v in sd.items()}
    with torch.no_grad():
        for a in (img, ref):
            for f in R.features(sd64, R.prep(a, torch.float64)):
                assert float(torch.sqrt((f ** 2).sum(dim=1)).min()) > 0.0
    assert np.array_equal(layers[0], np.zeros(5)) and total[0] == 0.0
    assert layers[1:].min() >= 1e-4, layers
    e32 = np.abs(R.lpips_vgg(sd, img, ref, torch.float32)[1] - layers)
    print('fp32 against fp64, relative, per layer:', (e32[1:] / layers[1:]).max(axis=0))


def test_too_small_agrees_with_the_fourth_pool():
    from evreal_amd.lpips import LPIPSVGG
    assert LPIPSVGG.MIN_SIDE == R.MIN_SIDE == 16
    for H, W in ((16, 16), (15, 40), (40, 15), (17, 16), (8, 40), (31, 33)):
        x = torch.zeros(1, 1, H, W)
        try:
            for _ in range(4):
                x = F.max_pool2d(x, kernel_size=2, stride=2)
            raised = False
        except RuntimeError:
            raised = True
        why = LPIPSVGG.too_small(H, W)
        assert (why is not None) == raised, (H, W)
        assert why is None or f'{H}x{W}' in why


@pytest.mark.parametrize('route', ['register_metric', 'pyiqa'])
def test_tracker_without_weights_leaves_the_name_to_its_other_providers(tmp_path, monkeypatch, route):
    """Without a weights file `lpips-vgg` goes on to register_metric / pyiqa as before: a metric of that name that is not this
    project's GPU metric is booked and finalized like any other (finalize() must not look for the handle's range counter)."""
    from evreal_amd import build, eval_metrics as em
    build.build(verbose=False)
    monkeypatch.setenv(em.LPIPS_VGG_WEIGHTS_ENV, str(tmp_path / 'nowhere.pth'))
    monkeypatch.setattr(em.EvalMetricsTracker, '_lpips_vgg_cache', [False, None])

    class Stub(em.BaseMetric):
        def calculate(self, img, ref):
            return float(np.abs(img - ref).mean())

    if route == 'register_metric':
        monkeypatch.setitem(em._REGISTRY, 'lpips-vgg', lambda: Stub('lpips-vgg'))
    else:
        fn = lambda imgs, refs: (imgs - refs).abs().mean(dim=(1, 2, 3))
        fake = type('FakePyiqa', (), {'list_of_metrics': ['lpips-vgg'],
                                      'get_metric': lambda self, name: em._QueuedIqaMetric(name, False, fn)})()
        monkeypatch.setattr(em, '_pyiqa_factory', fake)
    t = em.EvalMetricsTracker(output_dir=str(tmp_path / 'out'), quan_eval_metric_names=['lpips-vgg'], has_reference_frames=True)
    assert [m.name for m in t.metrics] == ['lpips-vgg'] and not getattr(t.metrics[0], 'on_gpu', False)
    assert em.EvalMetricsTracker._lpips_vgg_cache == [True, None]
    rng = np.random.default_rng(1)
    imgs, refs = torch.from_numpy(rng.random((6, 20, 24), dtype=np.float32)), torch.from_numpy(rng.random((6, 20, 24), dtype=np.float32))
    t.update_batch(list(range(6)), imgs, refs, [0.01 * i for i in range(6)], None)
    t.finalize(5)
    want = [float((a - b).abs().mean()) for a, b in zip(imgs, refs)]
    lines = open(tmp_path / 'out' / 'lpips-vgg.txt').read().splitlines()
    assert [int(l.split()[0]) for l in lines] == list(range(6))
    assert all(abs(float(l.split()[1]) - w) <= 1.01e-5 for l, w in zip(lines, want))
    assert abs(t.get_mean_scores()['lpips-vgg'] - np.mean(want)) <= 1e-6
