"""CPU study behind the gates of tests/test_resnext_hip.py: the ResNeXt HIP path's orchestration (embedders/resnext_hip.py) run through the
plain-torch emulation of its kernels in fp64, with the operands of EVERY contraction rounded the way the kernel that call selects rounds
them -- i.e. the error an assignment of operand modes itself implies on this network and input, independent of any kernel.  The rounding
and the table of assignments live in tests/rounding_study.py and tests/emu_modes.py (this is a thin caller, so that the gates and the
study cannot drift).
usage: embedder_rounding_study.py [--layers 2,2,1,1] CASE [CASE ...] | all        (cases: tests/rounding_study.py CASES)
Prints, per case, eval and train mode: logits / all gradients / worst BatchNorm buffer vs exact fp64 (rel-L2) and the six worst
parameter gradients.  The [2,2,1,1] figures are the MODE_PREDICTIONS table of tests/test_resnext_hip.py (the GPU kernels land within 25 %
of them).  --layers 2,1,1,1 (the net of test_resnext_forward_backward_vs_fp64; logits / all gradients): bf16x3 eval 6.3e-6 / 4.7e-5,
train 3.5e-5 / 1.3e-2;  f16 eval 5.0e-4 / 2.0e-3, train 3.1e-3 / 1.4e-1;  f16-Y16=0 eval 4.9e-4 / 2.4e-3, train 2.9e-3 / 1.3e-1."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import rounding_study as RS          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--layers', default='2,2,1,1')
ap.add_argument('cases', nargs='+')
args = ap.parse_args()
layers = tuple(int(v) for v in args.layers.split(','))
for case in (list(RS.CASES) if args.cases == ['all'] else args.cases):
    for train in (False, True):
        e = RS.predict(case, train, layers=layers)
        print(f'{case} {"train" if train else "eval"}: logits {e["logits"]:.2e}, all-gradients {e["grads"]:.2e}, buffers {e["buffers"]:.2e}', flush=True)
        print('  worst', [(k, f'{v:.1e}') for v, k in e['worst']], flush=True)
