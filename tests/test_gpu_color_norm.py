"""GPU: evr_color_percentile_normalize (post_process_norm of merged uint8 BGR frames in colour mode) against the numpy float
path of tests/color_norm_ref.py -- bytes bit-exact, lo / hi exact -- and the colour drop-in with post_process_norm end to end."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import color_norm_ref as cref

pytestmark = pytest.mark.gpu

# 2x2: 12 bytes, a tail-only frame.  3x5: 45 bytes.  37x23: 2553 bytes, no multiple of 16 -- in a batch every frame after the first
# starts misaligned.  48x64 and 260x346: several work-groups per frame.
SHAPES = [(2, 2), (3, 5), (37, 23), (48, 64), (260, 346)]


@functools.lru_cache(maxsize=None)
def _frames(H, W):
    a = np.stack([cref.frame(kind, H, W, 11) for kind in cref.KINDS])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _want(H, W, norm):
    """[(bytes, lo, hi)] of every frame of _frames(H, W): computed once, shared, never written"""
    out = [cref.direct(f, norm) for f in _frames(H, W)]
    for b, _, _ in out:
        b.setflags(write=False)
    return out


def _norm(x, norm, **kw):
    from evreal_amd import prepost
    return prepost.color_post_process_normalization(x, norm, **kw)


@pytest.mark.parametrize('norm', cref.NORMS)
@pytest.mark.parametrize('H,W', SHAPES)
def test_bytes_and_range_are_bit_exact(H, W, norm):
    frames, want = _frames(H, W), _want(H, W, norm)
    x = torch.from_numpy(frames.copy()).cuda()
    out, rng = _norm(x, norm, return_range=True)
    assert out is not x and np.array_equal(x.cpu().numpy(), frames)          # out of place: the input is untouched
    out, rng = out.cpu().numpy(), rng.cpu().numpy()
    for k, kind in enumerate(cref.KINDS):
        b, lo, hi = want[k]
        print(f'{kind} {H}x{W} {norm}: lo {rng[k, 0]!r} (want {lo!r}) hi {rng[k, 1]!r} (want {hi!r}) '
              f'differing bytes {int((out[k] != b).sum())} of {b.size}')
        assert rng[k, 0] == lo and rng[k, 1] == hi, (kind, rng[k], lo, hi)
        assert np.array_equal(out[k], b), (kind, int((out[k] != b).sum()))
    assert not out[cref.KINDS.index('constant')].any()                       # 0/0 = NaN -> byte 0
    if 3 * H * W >= 2553 and norm != 'standard':                             # (one minority byte in 12 or 45 is no 0.2 %)
        k = cref.KINDS.index('two_levels')
        assert rng[k, 0] == rng[k, 1] and set(np.unique(out[k])) == {0, 255}
    if norm == 'standard':
        k = cref.KINDS.index('two_levels')
        assert rng[k, 0] < rng[k, 1]


@pytest.mark.parametrize('norm', cref.NORMS)
def test_single_frame_without_batch_dimension(norm):
    H, W = 37, 23
    k = cref.KINDS.index('uniform')
    x = torch.from_numpy(_frames(H, W)[k].copy()).cuda()
    out, rng = _norm(x, norm, return_range=True)
    b, lo, hi = _want(H, W, norm)[k]
    assert out.shape == x.shape and tuple(rng.shape) == (1, 2)
    assert np.array_equal(out.cpu().numpy(), b) and rng[0, 0].item() == lo and rng[0, 1].item() == hi


@pytest.mark.parametrize('H,W', [(37, 23), (48, 64)])
def test_batch_gives_each_frame_what_it_gets_alone(H, W):
    frames = _frames(H, W)[:5]                                               # five different frames
    x = torch.from_numpy(frames.copy()).cuda()
    for norm in cref.NORMS:
        batch = _norm(x, norm).cpu().numpy()
        for k in range(5):
            alone = _norm(x[k].clone(), norm).cpu().numpy()
            assert np.array_equal(batch[k], alone), (norm, k)


@pytest.mark.parametrize('H,W', [(3, 5), (37, 23), (260, 346)])
def test_in_place_equals_out_of_place(H, W):
    frames = _frames(H, W)
    for norm in cref.NORMS:
        x = torch.from_numpy(frames.copy()).cuda()
        want = _norm(x, norm)
        got = _norm(x, norm, out=x)
        assert got is x and torch.equal(x, want), norm
        # an output whose frames sit at another alignment than the input's
        buf = torch.zeros(x.numel() + 5, dtype=torch.uint8, device='cuda')
        y = buf[5:].view(x.shape)
        _norm(torch.from_numpy(frames.copy()).cuda(), norm, out=y)
        assert torch.equal(y, want) and not buf[:5].any(), norm


def test_empty_batch_and_too_large_frames():
    from evreal_amd import lib as L
    out = _norm(torch.empty((0, 4, 6, 3), dtype=torch.uint8, device='cuda'), 'robust')
    assert tuple(out.shape) == (0, 4, 6, 3)
    l = L.load()
    x = torch.zeros(64, dtype=torch.uint8, device='cuda')
    v = torch.zeros(256, dtype=torch.float32, device='cuda')
    ws = torch.zeros(1024, dtype=torch.int32, device='cuda')
    args = lambda H, W, nbytes: (L.ptr(x), L.ptr(x), 1, H, W, L.ptr(v), 1.0, 99.0, L.ptr(ws), nbytes, L.stream_ptr())
    assert l.evr_color_percentile_normalize(*args(2048, 2731, 4096)) == -1          # 3*H*W >= 2^24: EVR_ERR_INVALID, no launch
    assert b'2^24' in l.evr_last_error()
    assert l.evr_color_percentile_normalize(*args(2, 2, 1031)) == -3                # EVR_ERR_WORKSPACE
    assert l.evr_color_percentile_normalize_workspace_bytes(1) == 1032


def _write_configs(tmp_path, method, method_config):
    for sub in ('eval', 'method', 'dataset'):
        os.makedirs(tmp_path / 'config' / sub, exist_ok=True)
    json.dump({"dataset_kwargs": {"num_bins": 5, "voxel_method": {"method": "between_frames"}, "keep_ratio": 1.0},
               "save_images": True, "histeq": "none", "color": True, "eval_infer_all": False, "ts_tol_ms": 1.0,
               "create_video": False}, open(tmp_path / 'config/eval/color.json', 'w'))
    json.dump(method_config, open(tmp_path / f'config/method/{method}.json', 'w'))
    json.dump({"root_path": str(tmp_path / 'data/C'), "sequences": {"s0": {}}}, open(tmp_path / 'config/dataset/C.json', 'w'))


@pytest.mark.parametrize('method,norm', [('E2VID+', 'robust'), ('SSL-E2VID', 'exprobust')])
def test_color_eval_with_post_process_norm_end_to_end(tmp_path, monkeypatch, method, norm):
    """The layout of test_gpu_color.py::test_color_eval_config_runs_end_to_end with a method config that carries a post_process_norm:
    every PNG decodes to color_norm_ref of the merged frame that reached the normalisation, RGB flipped; timestamps as in a
    'none' run."""
    from PIL import Image
    from evreal_amd import eval as ev, prepost, synth, weights
    kw = dict(weights.E2VID_PLUS_KWARGS)
    sd = weights.synth_state_dict(weights.unet_recurrent_schema(**kw), seed=2)
    tensors = {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    if method == 'SSL-E2VID':           # a plain state dict (eval.py:134-139)
        torch.save(tensors, tmp_path / 'm.pth')
    else:                               # config is a dict-like with ['arch'] = {'type', 'args'}
        torch.save({'state_dict': tensors, 'config': {'arch': {'type': 'E2VIDRecurrent', 'args': {'unet_kwargs': kw}}}},
                   tmp_path / 'm.pth')
    synth.write_sequence(str(tmp_path / 'data/C/s0'), 5, 20000, 2.0e5, 64, 48, 50.0)
    seen = []
    real = prepost.color_post_process_normalization

    def spy(bgr_u8, norm_, **kwargs):
        seen.append((bgr_u8.cpu().numpy().copy(), norm_))
        return real(bgr_u8, norm_, **kwargs)
    monkeypatch.setattr(prepost, 'color_post_process_normalization', spy)
    monkeypatch.chdir(tmp_path)
    out = tmp_path / f'outputs/color/C/s0/{method}'
    ts = {}
    for pn in ('none', norm):
        _write_configs(tmp_path, method, {"model_name": method, "model_path": str(tmp_path / 'm.pth'),
                                          "event_tensor_normalization": True, "post_process_norm": pn})
        del seen[:]
        ev.evaluate([method], ['color'], ['C'], ['mse'])
        ts[pn] = open(out / 'timestamps.txt').read()
        os.remove(out / 'timestamps.txt')
    assert len(ts[norm].strip().splitlines()) == 3 and ts[norm] == ts['none']
    frames = np.concatenate([a for a, _ in seen])
    assert all(n_ == norm for _, n_ in seen) and frames.shape == (3, 48, 64, 3)
    pngs = sorted(p for p in os.listdir(out) if p.startswith('frame_'))
    assert len(pngs) == 3
    for p, f in zip(pngs, frames):
        im = np.asarray(Image.open(out / p))
        want = cref.direct(f, norm)[0][..., ::-1]
        assert f.std() > 0, "a constant merged frame would make this test vacuous"
        assert np.array_equal(im, want), (p, int((im != want).sum()))
