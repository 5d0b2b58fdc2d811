"""conv_wgrad_kernel<KS, UPS, PREC, COB> and the three reductions behind it (csrc/conv_wgrad.hip), bit for bit against the fp64 sums of exact integer
operands -- tests/wgrad_exact_cases.py, once per knob setting in a fresh interpreter.  The scripts append the launch record of every case to one
file; after all settings have run, every form of the literal table below must have been recorded at least once.  The budget of every case is
asserted on the CPU (no GPU needed)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import wgrad_exact_cases as M  # noqa: E402

SETTINGS = [{}, {'LP_WGRAD_COB': '64'}, {'LP_WGRAD3_PIPE': '0'}, {'LP_WGRAD3_X3': '0'}]
IDS = [','.join(f'{k}={v}' for k, v in e.items()) or 'default' for e in SETTINGS]
SCRIPT, OK = 'wgrad_exact_cases.py', 'WGRAD_EXACT_OK'
KNOBS = ('LP_WGRAD_COB', 'LP_WGRAD3_PIPE', 'LP_WGRAD3_X3')

G = dict(kernel='generic')
FORMS = [
    ('COB 128 3x3', dict(G, ks=3, ups=0, cob=128)),
    ('COB 128 3x3 ups', dict(G, ks=3, ups=1, cob=128)),
    ('COB 64 3x3', dict(G, ks=3, ups=0, cob=64)),
    ('COB 64 3x3 ups', dict(G, ks=3, ups=1, cob=64)),
    ('COB 128 1x1 with a bias gradient', dict(G, ks=1, cob=128, bias=1)),
    ('COB 64 1x1 with a bias gradient', dict(G, ks=1, cob=64, bias=1)),
    ('1x1 kernel without a bias gradient', dict(kernel='1x1', ks=1, bias=0)),
    ('eight image slots', dict(G, lnb=3)),
    ('sixteen image slots', dict(G, lnb=4)),
]
for _red in ('flat32', 'flat256', 'tiled'):
    FORMS += [(f'{_red} one split', dict(G, red=_red, splits=1, bias=1)), (f'{_red} five splits', dict(G, red=_red, splits=5, bias=1)),
              (f'{_red} splits capped by the tiles', dict(G, red=_red, splits=6, tiles=6, bias=1))]
FORMS += [('tiled 1x1', dict(G, red='tiled', ks=1, bias=1))]

_RUNS = {}


def run_setting(i, tmp):
    """one script run per knob setting, cached: -> (returncode, stdout, stderr, records)"""
    if i not in _RUNS:
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env.update(SETTINGS[i])
        log = os.path.join(tmp, f'forms_{i}.jsonl')
        env['LP_FORM_LOG'] = log
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', SCRIPT)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        recs = [json.loads(line) for line in open(log)] if os.path.exists(log) else []
        _RUNS[i] = (r.returncode, r.stdout, r.stderr, recs)
    return _RUNS[i]


@pytest.fixture(scope='module')
def form_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp('wgrad_forms'))


def test_every_case_is_within_the_exactness_budget():
    """CPU: build() asserts sum_pixels |dy| |a| (and the bias gradient's sum |dy| + |accumulator|) <= 2^22 quanta for every case, mode and role"""
    for prec in M.PRECS:
        for index, case in enumerate(M.CASES):
            for wide in M.roles(index, prec):
                assert M.build(case, prec, wide, (0, 2)[index & 1])['quanta'] <= 2 ** 22


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(SETTINGS)), ids=IDS)
def test_conv_wgrad_kernel_is_exact_on_integer_operands(i, form_dir):
    rc, out, err, _ = run_setting(i, form_dir)
    print(out[-20000:])
    assert rc == 0 and OK in out, (out[-6000:], err[-3000:])


@pytest.mark.gpu
def test_every_wgrad_form_was_recorded(form_dir):
    recs = []
    for i in range(len(SETTINGS)):
        rc, out, err, r = run_setting(i, form_dir)
        assert rc == 0 and OK in out, (IDS[i], out[-3000:], err[-3000:])
        recs += [x['rec'] for x in r]
    missing = [name for name, want in FORMS if not any(all(rec.get(k) == v for k, v in want.items()) for rec in recs)]
    assert not missing, f'forms no exact case reached: {missing}'
