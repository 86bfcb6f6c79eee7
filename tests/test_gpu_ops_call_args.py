"""The GEMM / split / conv3x3 wrappers of naws_hip/ops.py pass the C ABI exactly what they passed
before they were rewritten over shared helpers: tests/golden/ops_call_args_before.json holds, per
operand form (2-D, batched, row-sliced operands, row-strided out / aux, batch-strided bias, column
and row ranges, pool2, a caller's out), the argument tuples recorded with the parent commit's
module, pointers as (tensor, byte offset) - and the exception of one malformed operand per rule.
naws_hip.lib.call is replaced by the recorder for the duration: nothing is launched."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
try:
    import make_ops_call_args as rec
finally:
    sys.path.pop(0)

BEFORE = json.load(open(os.path.join(HERE, 'golden', 'ops_call_args_before.json')))


@pytest.fixture(scope='module')
def recorded(dev):
    from naws_hip import ops
    return rec.record(ops, dev)


@pytest.mark.gpu
def test_the_fixture_covers_every_case_and_every_rule(recorded):
    assert sorted(recorded) == sorted(BEFORE) == sorted(n for n, _ in rec.CASES)
    kinds = {e['raises'] for e in BEFORE.values() if 'raises' in e}
    assert {'TypeError', 'NawsError'} <= kinds
    assert sum('raises' not in e for e in BEFORE.values()) >= 80


@pytest.mark.gpu
@pytest.mark.parametrize('name', [n for n, _ in rec.CASES])
def test_wrapper_passes_what_the_parent_passed(recorded, name):
    assert recorded[name] == BEFORE[name]
