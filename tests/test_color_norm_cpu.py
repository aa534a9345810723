"""Colour post-process normalisation, the parts that need no GPU: the histogram / table form the kernels compute equals the direct
float path byte for byte (tests/color_norm_ref.py), and the public function checks its `norm` argument before it loads the library."""
import numpy as np
import pytest

import color_norm_ref as cref

SHAPES = [(2, 2), (3, 5), (7, 59), (37, 23), (48, 64), (180, 240)]


@pytest.mark.parametrize('norm', cref.NORMS)
def test_table_form_equals_the_direct_float_path(norm):
    n = 0
    for seed, (H, W) in enumerate(SHAPES):
        for kind in cref.KINDS:
            u8 = cref.frame(kind, H, W, seed)
            want, lo, hi = cref.direct(u8, norm)
            got, lo_t, hi_t = cref.table(u8, norm)
            assert lo_t == lo and hi_t == hi, (kind, H, W, lo, lo_t, hi, hi_t)
            assert np.array_equal(got, want), (kind, H, W, int((got != want).sum()))
            n += 1
    assert n == 36


def test_reference_frames_have_the_properties_their_names_promise():
    H, W = 48, 64
    out, lo, hi = cref.direct(cref.frame('constant', H, W, 0), 'robust')
    assert lo == hi and not out.any()                                   # 0/0 = NaN everywhere -> byte 0
    u8 = cref.frame('two_levels', H, W, 0)
    out, lo, hi = cref.direct(u8, 'robust')
    assert lo == hi and set(np.unique(out)) == {0, 255} and np.array_equal(out == 255, u8 == 200)
    out, lo, hi = cref.direct(u8, 'standard')
    assert lo < hi and np.array_equal(out == 255, u8 == 200)
    u8 = cref.frame('band_outliers', H, W, 0)
    assert cref.direct(u8, 'robust')[2] <= np.float32(102) / np.float32(255) < cref.direct(u8, 'standard')[2] == 1
    assert len(np.unique(cref.frame('four_levels', H, W, 0))) == 4
    assert (cref.frame('dark_clipped', H, W, 0) == 0).mean() > 0.5


def test_argument_check_needs_no_gpu(monkeypatch):
    import torch
    from evreal_amd import lib, prepost
    monkeypatch.setattr(lib, 'load', lambda: pytest.fail("the library must not be loaded for an argument error or for 'none'"))
    x = torch.zeros((2, 4, 6, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="Unrecognized normalization argument: bogus"):
        prepost.color_post_process_normalization(x, 'bogus')
    assert prepost.color_post_process_normalization(x, 'none') is x
