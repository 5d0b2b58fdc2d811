"""The knob table of the kernel dispatchers (csrc/lp_knobs.h) on the CPU: a stand-alone host program that includes the header alone prints
every field.  The defaults are asserted literally (a wrong sentinel -- 0 where -1 means "auto" -- would silently change dispatch), every kept
knob must land in its own field, and the names of the retired A/B switches must change nothing."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'latent_pose_reenactment_amd', 'csrc')
DEFAULTS = {       # field (its environment name: LP_ + the field in capitals) -> default
    'conv_pp': -1, 'conv_w8': -1, 'conv_ksplit': 8, 'conv_split_wgs': 256, 'conv_nbuf': 0, 'conv_xcd': 1, 'conv_pipe': 1, 'conv_pipe_mr': 0,
    'conv1x1_pipe': 0, 'wgrad_cob': 0, 'wgrad3_pipe': 1, 'wgrad3_x3': 1, 'thin_mfma': 1, 'gconv_rows': 1, 'gconv_rows_wgs': 0, 'stat_split_fixed': 0,
}
RETIRED = ['LP_CONV1X1_B1', 'LP_CONV1X1_TILE', 'LP_CONV_X3_BN64', 'LP_CONV_ADBUF', 'LP_CONV_CC1', 'LP_GCONV_HALF', 'LP_CONV_PIPE_N64', 'LP_CONV_PIPE_X3',
           'LP_CONV1X1_PIPE_MAXK', 'LP_WGRAD1X1_OLD', 'LP_W1_KP', 'LP_WGRAD_COB1', 'LP_WGRAD3_WGS', 'LP_WGRAD3_MIN_TILES', 'LP_GWGRAD_DIAG']
PROGRAM = ('#include "lp_knobs.h"\n#include <stdio.h>\nint main() {\n    const LpKnobs& k = lp_knobs();\n'
           + ''.join(f'    printf("{f} %d\\n", k.{f});\n' for f in DEFAULTS)
           + f'    return sizeof(LpKnobs) == {len(DEFAULTS)} * sizeof(int) ? 0 : 3;      // 3: a field this program does not print\n}}\n')


@pytest.fixture(scope='module')
def knobs(tmp_path_factory):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    d = tmp_path_factory.mktemp('knobs')
    (d / 'knobs.cpp').write_text(PROGRAM)
    r = subprocess.run([cxx, '-std=c++17', '-Wall', '-Werror', '-I', CSRC, str(d / 'knobs.cpp'), '-o', str(d / 'knobs')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(env):
        clean = {k: v for k, v in os.environ.items() if not k.startswith('LP_')}
        r = subprocess.run([str(d / 'knobs')], env=dict(clean, **env), capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stderr)
        return {l.split()[0]: int(l.split()[1]) for l in r.stdout.splitlines()}
    return run


def test_defaults(knobs):
    assert knobs({}) == DEFAULTS


def test_every_kept_knob_lands_in_its_own_field(knobs):
    want = dict({f: 1000 + i for i, f in enumerate(DEFAULTS)}, stat_split_fixed=1)      # (a presence switch: set to anything, "0" included, is on)
    env = dict({'LP_' + f.upper(): str(v) for f, v in want.items()}, LP_STAT_SPLIT_FIXED='0')
    assert knobs(env) == want
    for f in DEFAULTS:                                    # and one at a time: no other field moves
        assert knobs({'LP_' + f.upper(): env['LP_' + f.upper()]}) == dict(DEFAULTS, **{f: want[f]})


def test_retired_names_change_nothing(knobs):
    for v in ('0', '1', '2', '64', '256'):
        assert knobs({n: v for n in RETIRED}) == DEFAULTS
