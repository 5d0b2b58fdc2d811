"""The KS = 2 forms of conv_dma_kernel (csrc/conv_dma.hip: the scatter to the x2 grid and the gather over (phase, chunk)) through lp_pack_weights modes
2 .. 5, bit for bit against the fp64 contraction of exact integer operands -- tests/conv_phase_exact_cases.py, once per knob setting in a fresh
interpreter (the knob table is read once per process).  The scripts append the launch record of every case to one file; after all settings have run,
every form of the literal table below must have been recorded at least once.  The budget of every case, the identity of the phase algebra with the
dense operation and the restated weight packs are asserted on the CPU (no GPU needed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import conv_phase_exact_cases as M  # noqa: E402
import exact_operands as E  # noqa: E402
import operand_restatement as R  # noqa: E402

SETTINGS = [{}, {'LP_CONV_PP': '1'}, {'LP_CONV_PP': '0'}, {'LP_CONV_NBUF': '3'}, {'LP_CONV_NBUF': '2', 'LP_CONV_SPLIT_WGS': '512'}, {'LP_CONV_KSPLIT': '1'}]
IDS = [','.join(f'{k}={v}' for k, v in e.items()) or 'default' for e in SETTINGS]
SCRIPT, OK = 'conv_phase_exact_cases.py', 'CONV_PHASE_EXACT_OK'
KNOBS = ('LP_CONV_PP', 'LP_CONV_W8', 'LP_CONV_KSPLIT', 'LP_CONV_SPLIT_WGS', 'LP_CONV_NBUF', 'LP_CONV_XCD', 'LP_CONV_PIPE', 'LP_CONV_PIPE_MR', 'LP_CONV1X1_PIPE')

# every KS = 2 form of conv_dma_kernel's dispatch: (name, fields the record of at least one exact case must show; ``mode`` = the pack mode of the case
# that asked: 2 / 5 run the scatter form, 3 / 4 the gather form -- the record itself does not tell them apart)
D = dict(kernel='dma', ks=2)
T2244, T4144 = dict(wm=2, wn=2, mr=4, nr=4), dict(wm=4, wn=1, mr=4, nr=4)
FORMS = [
    ('<2,2,4,4> scatter', dict(D, mode=2, **T2244)),
    ('<4,1,4,4> scatter', dict(D, mode=2, **T4144)),
    ('<2,2,4,4> scatter, pool data gradient', dict(D, mode=5, **T2244)),
    ('<4,1,4,4> scatter, pool data gradient', dict(D, mode=5, **T4144)),
    ('<2,2,4,4> gather', dict(D, mode=3, **T2244)),
    ('<4,1,4,4> gather', dict(D, mode=3, **T4144)),
    ('<2,2,4,4> gather, pool forward', dict(D, mode=4, **T2244)),
    ('<4,1,4,4> gather, pool forward', dict(D, mode=4, **T4144)),
    ('ping-pong scatter <2,2,4,4>', dict(D, mode=2, pp=1, **T2244)),
    ('ping-pong gather <2,2,4,4>', dict(D, mode=3, pp=1, **T2244)),
    ('2-deep weight ring <2,2,4,4>', dict(D, pp=0, nbuf=2, **T2244)),
    ('2-deep weight ring <4,1,4,4>', dict(D, pp=0, nbuf=2, **T4144)),
    ('3-deep weight ring <2,2,4,4>', dict(D, pp=0, nbuf=3, **T2244)),
    ('3-deep weight ring <4,1,4,4>', dict(D, pp=0, nbuf=3, **T4144)),
    ('split-K 2 <2,2,4,4>', dict(D, ksplit=2, finish=1, **T2244)),
    ('split-K 2 <4,1,4,4>', dict(D, ksplit=2, finish=1, **T4144)),
    ('split-K 4 <2,2,4,4> scatter', dict(D, mode=2, ksplit=4, finish=1, **T2244)),
    ('split-K 4 <4,1,4,4> gather', dict(D, mode=3, ksplit=4, finish=1, **T4144)),
    ('split-K 8 <2,2,4,4> gather', dict(D, mode=3, ksplit=8, finish=1, **T2244)),
    ('split-K 8 <2,2,4,4> gather, pool forward', dict(D, mode=4, ksplit=8, finish=1, **T2244)),
    ('split-K 6 <2,2,4,4> (18 chunks)', dict(D, mode=2, ksplit=6, finish=1, **T2244)),
    ('split-K 7 <2,2,4,4> gather (20 stages)', dict(D, mode=3, ksplit=7, finish=1, **T2244)),
    ('unsplit gather <2,2,4,4>', dict(D, mode=3, ksplit=1, finish=0, **T2244)),
    ('statistics offered <2,2,4,4> scatter', dict(D, mode=2, stats=1, **T2244)),
    ('statistics offered <4,1,4,4> scatter', dict(D, mode=2, stats=1, **T4144)),
    ('statistics offered <4,1,4,4> gather', dict(D, mode=4, stats=1, **T4144)),
]

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
    return str(tmp_path_factory.mktemp('conv_phase_forms'))


def test_every_case_is_within_the_exactness_budget():
    """CPU: build() asserts alpha * phase_conv(|A|, |W'|) + |bias| + |res| <= 2^22 quanta for every case, mode and role, that the tap sums are integers of
    the weight quantum, that the reference is an fp32 value and -- single-plane modes 2 and 4 -- that the phase algebra IS the dense operation"""
    for prec in M.PRECS:
        for index, case in enumerate(M.CASES):
            for wide in M.roles(index, prec):
                b = M.build(case, prec, wide, M.pro_of(index, case))
                assert b['quanta'] <= 2 ** 22


def test_restated_weight_packs_of_every_case_decode_to_the_pre_summed_taps():
    """CPU: the words tests/operand_restatement.py says lp_pack_weights writes for every case (the GPU run compares the kernel's words with them) decode to
    the terms the reference contracts, with zero pad rows and columns"""
    for prec in M.PRECS:
        for index, case in enumerate(M.CASES):
            wide = M.roles(index, prec)[-1]
            b = M.build(case, prec, wide, M.pro_of(index, case))
            n, h, w, cin, cout = case['shape']
            cols_p = case['cols_p'] or (cin + 63) // 64 * 64
            hi, lo = R.weight_pack(b['w'].numpy(), case['mode'], (cout + 127) // 128 * 128, cols_p, prec)
            dec = R.decode(hi, lo, prec)
            assert not dec[:, cout:, :].any() and not dec[:, :, cin:].any()
            assert np.array_equal(dec[:, :cout, :cin], sum(b['t_terms']).numpy()), case['id']
            assert np.array_equal(R.decode(hi, None, 0 if prec == 1 else prec)[:, :cout, :cin], b['t_terms'][0].numpy()), case['id']


def test_the_case_list_names_every_setting_it_needs():
    ids = [c['id'] for c in M.CASES]
    assert {c['pp1'] for c in M.CASES} >= {'even', 'odd', 'gather'}
    assert {c['mode'] for c in M.CASES} == {2, 3, 4, 5} and len(ids) == len(set(ids))
    assert any(c['want_y'] == 0 for c in M.CASES if c['mode'] == 2) and any(c['want_y'] == 0 for c in M.CASES if c['mode'] == 4)
    assert torch.equal(torch.tensor([c['ksplit'] for c in M.CASES]).unique(), torch.tensor([1, 2, 4, 6, 7, 8]))


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(SETTINGS)), ids=IDS)
def test_phase_forms_are_exact_on_integer_operands(i, form_dir):
    rc, out, err, _ = run_setting(i, form_dir)
    print(out[-20000:])
    assert rc == 0 and OK in out, (out[-6000:], err[-3000:])


@pytest.mark.gpu
def test_every_phase_form_was_recorded(form_dir):
    recs = []
    for i in range(len(SETTINGS)):
        rc, out, err, r = run_setting(i, form_dir)
        assert rc == 0 and OK in out, (IDS[i], out[-3000:], err[-3000:])
        recs += [dict(x['rec'], mode=x['mode']) for x in r]
    missing = [name for name, want in FORMS if not any(all(rec.get(k) == v for k, v in want.items()) for rec in recs)]
    assert not missing, f'forms no exact case reached: {missing}'
