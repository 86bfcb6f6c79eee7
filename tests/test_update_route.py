"""naws_hip.update.choose_route names, from plain values, the kernels a whole-arena SGD update runs
and the re-split that goes with them.  Every combination of its boolean inputs is compared with
the expressions `WsddnEngine._apply_update` evaluated before the route had one owner, restated
here literally (the kernel if/elif and the re-split if/elif over planes / planes_bf / fused);
what that code refused with RuntimeError must still raise."""
import itertools

import pytest

from naws_hip import update as U


def _before(w6_done, fused_planes, regions, iter1, dirty, scaled, fc, k6_256, wgrad_update):
    """engine.py's _apply_update of the parent commit: `fc` = self._fc is not None, `regions` =
    self._sgd_regions is not None, `scaled` = self.arith.reports_maxima, `dirty` =
    self._planes_dirty, `iter1` = self.iter_size == 1, `k6_256` = self.k6 % 256 == 0."""
    if w6_done and (not fc or not regions or not wgrad_update):
        raise RuntimeError('fc6_w was updated in its wgrad epilogue but the plane state is gone')
    writes = w6_done or (fused_planes and regions and iter1 and not dirty)
    planes, planes_bf = writes and scaled, writes and not scaled
    fused = planes or (scaled and fc and iter1 and k6_256)
    # the kernel ...
    if planes:
        kernel = 'f16x2_rest' if w6_done else 'f16x2_whole'
    elif planes_bf:
        kernel = 'planes_rest' if w6_done else 'planes_whole'
    else:
        kernel = 'elementwise_rowmax' if fused else 'elementwise'
    # ... and the re-split behind it
    if planes:
        resplit = 'finish7' if w6_done else 'resplit6_finish7'
    elif fused:
        resplit = 'split_from_maxima'
    elif planes_bf:
        resplit = 'convert_w7t'
    elif fc:
        resplit = 'split_all'
    else:
        resplit = None
    return kernel, resplit


# what each named route launches, in the words of _before()
LAUNCHES = {
    'planes_f16x2': ('f16x2_whole', 'resplit6_finish7'),
    'planes_f16x2_rest': ('f16x2_rest', 'finish7'),
    'planes16': ('planes_whole', 'convert_w7t'),
    'planes16_rest': ('planes_rest', 'convert_w7t'),
    'rowmax': ('elementwise_rowmax', 'split_from_maxima'),
    'split_all': ('elementwise', 'split_all'),
    'plain': ('elementwise', None),
}
COMBINATIONS = list(itertools.product((False, True), repeat=9))


def test_the_routes_are_named_once():
    assert sorted(LAUNCHES) == sorted(U.ROUTES) and len(set(LAUNCHES.values())) == 7


def test_every_combination_takes_the_route_it_took_before():
    seen, refused = set(), 0
    for w6_done, fused_planes, regions, iter1, dirty, scaled, fc, k6_256, wgrad in COMBINATIONS:
        f = U.Facts(fused_planes=fused_planes, regions=regions, iter1=iter1, dirty=dirty,
                    maxima=scaled, planes16=fc, k6_256=k6_256, wgrad_update=wgrad)
        try:
            want = _before(w6_done, fused_planes, regions, iter1, dirty, scaled, fc, k6_256, wgrad)
        except RuntimeError:
            refused += 1
            with pytest.raises(RuntimeError, match='wgrad epilogue'):
                U.choose_route(f, w6_done)
            continue
        got = U.choose_route(f, w6_done)
        assert LAUNCHES[got] == want, (f, w6_done, got, want)
        seen.add(got)
    assert seen == set(U.ROUTES)
    assert refused == 256 - 32          # fc6_w done: all but (fc, regions, wgrad_update) all true


def test_shared_preconditions():
    f = U.Facts(True, True, True, False, True, True, True, True)
    assert U.rows_whole(f) and U.planes_valid(f)
    assert not U.rows_whole(f._replace(iter1=False)) and not U.rows_whole(f._replace(k6_256=False))
    assert not U.planes_valid(f._replace(dirty=True)) and not U.planes_valid(f._replace(regions=False))


def test_the_trace_fixture_unpacks_and_packs_back_to_itself():
    """tests/test_gpu_update_trace.py compares against unpack(fixture): the packed form is lossless
    (event ordinals in recording order, one fresh ordinal per record_event)."""
    import json
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    try:
        from update_trace_rec import pack, unpack
    finally:
        sys.path.pop(0)
    packed = json.load(open(os.path.join(here, 'golden', 'update_trace_before.json')))
    full = unpack(packed)
    assert pack(full) == packed and sum(len(s['trace']) for s in full.values()) == 3691
    for sc in full.values():
        rec = [r[2] for r in sc['trace'] if r[0] == 'record_event']
        assert rec == ['e%d' % k for k in range(len(rec))]
        assert all(r[2] in rec for r in sc['trace'] if r[0] == 'wait_event')
