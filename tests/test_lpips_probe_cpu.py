"""The power of the per-layer LPIPS probe (tests/lpips_probe.py), checked without a GPU: what tests/test_gpu_lpips_probe.py may claim
to notice.  Every deliberate error of lpips_probe.ERRORS, put into a float64 restatement of the oracle, must move at least one gated
score of the probe's inputs by ten times the gate; the fp32 oracle must sit a hundred times inside the gate; and no gated score may be
so small that the gate's absolute term carries it.  The table of the same errors on the inputs of test_lpips_vs_oracle and of
tests/test_gpu_lpips_modes.py is printed for contrast (pytest -s)."""
import numpy as np
import pytest

import lpips_probe as lp
from test_gpu_lpips_modes import _frames as frames_64x80
from test_gpu_lpips_modes import bound

GATED = range(1, lp.NPAIRS)          # pair 0 is identical: its score is exactly 0 and is asserted as such


def _means(shape, error=None):
    key = ('means', tuple(shape), error)
    if key not in lp._CACHE:
        img, ref = lp.pairs(shape)
        lp._CACHE[key] = lp.channel_means(img, ref, error)
    return lp._CACHE[key]


def test_restatement_is_the_oracle():
    """Without an error the restatement (channel means, then a head) gives the oracle's float64 scores: what the errors are put into is
    the arithmetic the GPU test compares with.  Pair 0 scores exactly 0."""
    for shape in lp.SHAPES:
        for name in lp.VARIANTS:
            want64, _ = lp.reference(shape, name)
            got = lp.scores(_means(shape), lp.variant(name))
            assert got[0] == 0.0 and want64[0] == 0.0
            np.testing.assert_allclose(got, want64, rtol=1e-12, atol=0)


def test_reference_within_its_own_bound_and_scores_not_small():
    """On every gated case the fp32 oracle is within 0.01 of the bound of the float64 one, and want64 >= 1e-3: the 1e-7 absolute term
    of the gate is under 0.05 % of the smallest score."""
    worst, smallest = 0.0, np.inf
    for shape in lp.SHAPES:
        for name in lp.VARIANTS:
            want64, want32 = lp.reference(shape, name)
            for p in GATED:
                r = abs(want32[p] - want64[p]) / bound(want64[p], want32[p], 1)
                worst, smallest = max(worst, r), min(smallest, want64[p])
                assert r <= 0.01, (shape, name, p, want64[p], want32[p])
                assert want64[p] >= 1e-3, (shape, name, p, want64[p])
    print(f'\nfp32 oracle against float64: worst {worst:.2e} of the bound; smallest gated score {smallest:.3e}')


@pytest.mark.parametrize('error', list(lp.ERRORS))
def test_every_injected_error_moves_a_gated_score(error):
    """At least one (shape, variant, pair) moves by >= 10 x bound(want64, want32, 1) in float64."""
    best = (0.0, None)
    for shape in lp.SHAPES:
        wrong = _means(shape, error)
        for name in lp.VARIANTS:
            want64, want32 = lp.reference(shape, name)
            got = lp.scores(wrong, lp.variant(name), error)
            ratio = np.abs(got - want64) / bound(want64, want32, 1)
            for p in GATED:
                if ratio[p] > best[0]:
                    best = (float(ratio[p]), (shape, name, p, float(abs(got[p] - want64[p]) / want64[p])))
    print(f'\n{error}: {best[0]:.0f} x bound at shape {best[1][0]}, {best[1][1]}, pair {best[1][2]} (relative change {best[1][3]:.1e})')
    assert best[0] >= 10.0, (error, best)


def _old_inputs(shape):
    """The frames of test_lpips_vs_oracle (tests/test_gpu_prepost.py) at `shape`."""
    H, W = shape
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    ref = np.stack([0.5 + 0.4 * np.sin(xx / (7.0 + i)) * np.cos(yy / (9.0 + i)) for i in range(3)]).astype(np.float32)
    img = np.clip(ref + 0.1 * rng.standard_normal(ref.shape), 0, 1).astype(np.float32)
    img[0] = ref[0]
    return img, ref


def test_print_contrast_with_todays_inputs():
    """Printed, not asserted: the relative change of the scores that test_lpips_vs_oracle (260x346, 180x240, 96x128) and
    test_arithmetic_modes (64x80) gate at 2e-4, all five lin heads of seed 3, pairs 1 and 2, under the first four errors."""
    sd = lp.base_state_dict()
    cols = [((260, 346), _old_inputs), ((180, 240), _old_inputs), ((96, 128), _old_inputs), ((64, 80), lambda s: frames_64x80())]
    base = {s: lp.scores(lp.channel_means(*f(s)), sd) for s, f in cols}
    lines = ['relative change of the gated totals (pairs 1, 2); the gate is 2e-4',
             f'{"error":34s}' + ''.join(f'{f"{s[0]}x{s[1]}":>20s}' for s, _ in cols)]
    for error in lp.TABLE_ERRORS:
        row = f'{error:34s}'
        for s, f in cols:
            got = lp.scores(lp.channel_means(*f(s), error), sd, error)
            rel = np.abs(got - base[s])[1:] / base[s][1:]
            row += f'{", ".join(f"{r:.0e}" for r in rel):>20s}'
        lines.append(row)
    print('\n' + '\n'.join(lines))
