"""The op-by-op plan launches what it launched before the operator table: two training iterations
of the tiny model (one 3 x 48 x 64 image, 12 rois, 20 classes, dropout on, RNG_SEED 3) per build,
every `naws_hip.lib.call` recorded - entry name, ints and the u64 seed exactly, floats by repr,
pointers as null / not null - and compared element for element with the trace of the parent commit
(tests/golden/opbyop_call_trace_before.json, written there by make_golden_opbyop_call_trace.py).
An equal trace is the same kernels in the same order at the same shapes and scalars; that the
pointers carry the right tensors is what the numeric suites of the plan check."""
import json
import math
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
try:
    import make_golden_opbyop_call_trace as rec
finally:
    sys.path.pop(0)
BEFORE = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'opbyop_call_trace_before.json')))


def test_the_recorded_builds_are_the_ones_traced():
    assert sorted(BEFORE) == sorted(rec.BUILDS) and len(BEFORE) == 7
    assert all(len(calls) > 300 for calls in BEFORE.values())


@pytest.mark.parametrize('name', sorted(rec.BUILDS))
def test_two_iterations_launch_what_they_launched_before(dev, name):
    """The second iteration runs the cached per-op objects, the cached SGD objects and the half of
    CenterLoss that takes in the first iteration's centre contributions.  The losses of both
    iterations are finite and positive, so a trace of garbage cannot pass."""
    calls, losses = rec.trace(dev, name)
    want = BEFORE[name]
    print('%s: %d calls (before: %d); losses %s' % (name, len(calls), len(want), losses))
    assert [c[0] for c in calls] == [c[0] for c in want]
    for k, (got, exp) in enumerate(zip(calls, want)):
        assert got == exp, (k, got, exp)
    assert len(losses) == 2 and all(l for l in losses)
    for it in losses:
        for blob, v in it.items():
            assert math.isfinite(v) and v > 0, (blob, v)
