"""The update schedule launches and synchronises what it did before it had one owner
(naws_hip/update.py): per scenario of tests/golden/make_golden_update_trace.py - every route of the
deferred SGD update, three or four iterations of the tiny model each - every C-ABI call with the
ordinal of its stream, every event recorded and waited for and every call of the gradient exchange
are compared element for element with the trace of the parent commit
(tests/golden/update_trace_before.json, written there by the same generator), and the SHA-256 of
every state tensor after the last flush() with the parent's (both of its runs gave the same digests
in every scenario).  An equal trace is the same kernels in the same order on the same streams
behind the same events; the digests say that the pointers carried the same tensors."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
try:
    import make_golden_update_trace as rec
finally:
    sys.path.pop(0)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
try:
    from update_trace_rec import unpack
finally:
    sys.path.pop(0)
BEFORE = unpack(json.load(open(os.path.join(ROOT, 'tests', 'golden', 'update_trace_before.json'))))


def test_the_recorded_scenarios_are_the_ones_traced():
    assert sorted(BEFORE) == sorted(rec.SCENARIOS) and len(BEFORE) == 14
    for name, want in BEFORE.items():
        kinds = {row[0] for row in want['trace']}
        assert {'record_event', 'wait_event', 'reducer.reduce_async', 'reducer.wait'} <= kinds, name
        assert len(want['trace']) > 100 and {'params', 'momentum'} <= set(want['digests']), name
    for name in ('h_pipelined_eager', 'i_pipelined_after'):
        assert any(row[0] == 'reducer.wait_first' for row in BEFORE[name]['trace'])
    kinds = {row[0] for row in BEFORE['k_sharded_then_default']['trace']}
    assert {'reducer.reduce_to_owner_async', 'reducer.gather_blocks_async'} <= kinds


@pytest.mark.parametrize('name', sorted(rec.SCENARIOS))
def test_the_schedule_is_what_it_was_before(dev, name):
    rows, digests = rec.run(dev, name)
    want = BEFORE[name]
    print('%s: %d rows (before: %d)' % (name, len(rows), len(want['trace'])))
    assert [r[0] for r in rows] == [r[0] for r in want['trace']]
    for k, (got, exp) in enumerate(zip(rows, want['trace'])):
        assert got == exp, (k, got, exp)
    assert digests == want['digests']
