"""Which kernel a convolution gets, without a GPU: csrc/conv_route.cpp is pure host code, so tests/conv_route_cpu.cpp -- a program with
its own main() that fills launch plans by hand -- is compiled against it alone with build.py's hipcc and its rows are compared with
tests/golden/conv_routes.json: the E2VID / FireNet layers at the smallest tile counts where a rule of the dispatch flips (ragged rounds,
the twin / 256 x 256 / plain / decoder thresholds, split K and its epilogue, the programmed band forms, FireNet's row kernel, LPIPS
conv2) and the switches of the ConvKnobs table, given as a value, not through the environment."""
import json
import os
import subprocess

import pytest

from evreal_amd import build as evr_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'evreal_amd', 'csrc')

pytestmark = pytest.mark.skipif(not os.path.exists(evr_build.HIPCC), reason='no hipcc')


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('conv_route') / 'conv_route_cpu')
    cmd = [evr_build.HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC, '-Wall', '-Werror',
           '-x', 'hip', os.path.join(ROOT, 'tests', 'conv_route_cpu.cpp'), os.path.join(CSRC, 'conv_route.cpp'), '-o', exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith('EVR_')}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    return {d['id']: d for d in map(json.loads, r.stdout.splitlines())}


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(ROOT, 'tests', 'golden', 'conv_routes.json')) as fh:
        return {k: v for k, v in json.load(fh).items() if not k.startswith('_')}


def test_every_row_matches_the_golden_table(rows, golden):
    assert sorted(rows) == sorted(golden)
    wrong = {}
    for rid, want in golden.items():
        got = {k: rows[rid][k] for k in want if k != 'trace'}
        if got != {k: v for k, v in want.items() if k != 'trace'}:
            wrong[rid] = (got, want)
    assert not wrong, wrong


def test_the_ragged_round_rule_keeps_the_twin_form(rows):
    # 128 input channels: 2904 tiles of 256 x 256 are 11.34 rounds of 256 blocks -> twin; 5808 = 22.69 rounds -> the 256 x 256 skewed loop
    assert (rows['enc0.rec.32seq']['wn'], rows['enc0.rec.32seq']['alt']) == (1, 0)
    assert (rows['enc0.rec.64seq']['wn'], rows['enc0.rec.64seq']['alt']) == (2, 1)


def test_split_k_caps(rows):
    assert [rows[k]['ks'] for k in ('band.192', 'band.193', 'band.64', 'band.65', 'band.64.no_ws')] == [2, 1, 8, 4, 1]
    assert [rows[k]['epi_sum'] for k in ('band.64', 'band.65')] == [8, 4]
    # EVR_KSPLIT set: the <= 64-tile cap of 8 is off; 16 is clamped to the 8 runs the epilogue sums; 0: never
    assert [rows[k]['ks'] for k in ('ksplit4.band.64', 'ksplit16.band.32', 'ksplit0.band.64')] == [4, 8, 1]


def test_an_explicit_wide_min_moves_all_four_thresholds(rows):
    assert rows['wide_min1.enc2.rec.1seq']['family'] == 'wide16' and rows['wide_min1.enc2.rec.1seq']['wn'] == 2      # 256 x 256: 600
    assert rows['wide_min1.enc0.rec.1seq']['family'] == 'wide16' and rows['wide_min1.enc0.rec.1seq']['wn'] == 1      # twin: 350
    assert rows['wide_min1.dec2.1seq']['family'] == 'wide'                                                            # dec32: 350
    assert rows['wide_min1.residual.1seq']['family'] == 'wide'                                                        # plain: 1024
    # ... and EVR_WIDE_MIN_PLAIN only the last
    assert rows['wide_min_plain.residual.1seq']['family'] == 'wide' and rows['wide_min_plain.enc0.rec.4seq'] == dict(rows['enc0.rec.4seq'], id='wide_min_plain.enc0.rec.4seq')


def test_the_band_switches(rows):
    assert rows['no_band.enc0.rec.64seq']['family'] == rows['no_band.enc.nb2.600']['family'] == rows['no_band.lpips.conv2.band']['family'] == 'igemm'
    assert rows['band5_0.lpips.conv2.band']['family'] == 'igemm' and rows['band5_0.residual.64seq']['family'] == 'band'
    assert rows['lpips.conv2.band']['family'] == 'bandk' and rows['lpips.conv2']['family'] == 'igemm'
    # EVR_BAND_MIN wins over EVR_BAND5_MIN
    assert rows['band_min.lpips.conv2.band']['family'] == 'igemm'


def test_firenet_row_kernel_threshold_and_switches(rows):
    assert [rows[k]['family'] for k in ('c16.1016', 'c16.1024', 'rows0.c16.1024', 'rows2.c16.8')] == ['c16_tile', 'c16_rows', 'c16_tile', 'c16_rows']
