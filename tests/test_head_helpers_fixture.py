"""tests/golden/head_helpers_before.json against the case list of tests/test_gpu_head_helpers_bits.py
(no GPU needed): the fixture holds exactly those cases, and no digest repeats across cases of
different shapes - a recorder that ignored its input would give one digest for all of them."""
import json
import re

import test_gpu_head_helpers_bits as bits


def _fixture():
    with open(bits.FIXTURE) as f:
        return json.load(f)


def test_fixture_lists_exactly_the_gpu_cases():
    fx = _fixture()
    assert sorted(fx) == sorted(bits.CASES)
    assert len(set(bits.CASES)) == len(bits.CASES)
    for case, rec in fx.items():
        assert rec, case
        for key, digest in rec.items():
            assert re.fullmatch(r'[0-9a-f]{64}', digest), (case, key)


def _shape(case):
    """What fixes the shape of a case's outputs: everything but the split count of the fc8 cases
    (FC8_KSPLIT changes the partial sums, not the shape; slices of one step give equal bits) and
    the segmentation of the tail cases (40 proposals either way; the per-row class softmax does
    not see the image boundaries)."""
    p = case.split('-')
    if p[0].startswith('fc8'):
        return tuple(p[:3])
    return (p[0], p[2]) if p[0] == 'tail' else tuple(p)


def test_no_digest_repeats_across_shapes():
    seen = {}
    for case, rec in sorted(_fixture().items()):
        for key, digest in rec.items():
            first = seen.setdefault(digest, case)
            assert _shape(first) == _shape(case), (digest, first, case, key)
