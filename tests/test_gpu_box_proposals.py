"""Box-proposal matching on the GPU (csrc/proposal_eval_ops.hip) against the tests' own literal
loop (tests/box_proposals_ref.py), value by value per ground-truth box with the sentinels, and
the device route of the evaluation against the host route and the recorded reference run.
Everything is array_equal / bit equality: no tolerance anywhere.

Shapes, each the smallest that reaches its branch: (P, G) = (1, 1); no proposals; no gt; 65 and
130 gt (the lanes loop over gt, more gt than proposals); 63 / 64 / 65 / 129 proposals (the lane
stride's edges); 200 x 130 (many rounds, cached proposals consumed); limits 0 (none), 1, 64, 100
and P, P + 1 of every shape, with all 8 area ranges, in ONE launch; 90 images x 48 settings (more
work items than the capped grid has waves: the grid-stride loop)."""
import logging

import numpy as np
import pytest
import torch

import box_proposals_ref as bp
import guard

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (0, 3), (3, 0), (3, 65), (200, 130), (63, 3), (64, 3), (65, 3), (129, 3)]
LIMITS = sorted({0, 1, 64, 100} | {p for p, _g in SHAPES} | {p + 1 for p, _g in SHAPES})
KINDS = {'float': dict(), 'quarter_pixel': dict(quantum=0.25), 'ties': dict(quantum=1.0, ties=True)}


def device_per_gt(roidb, areas, limits, dev, out=None):
    """-> float32 [len(areas) * len(limits), G] on the host (limit 0 = none)."""
    from detectron.datasets import json_dataset_evaluator as jde
    from naws_hip import ops
    t = [torch.from_numpy(a).to(dev) for a in jde.flatten_roidb(roidb)]
    lo = [bp.RANGES[a][0] for a in areas]
    hi = [bp.RANGES[a][1] for a in areas]
    got = ops.proposal_match(t[0], t[1], t[2], t[3], t[4], lo, hi, limits, out=out)
    return got.cpu().numpy()


def reference_per_gt(roidb, areas, limits):
    cache = {}
    return np.stack([bp.per_gt(roidb, a, l if l else None, cache=cache) for a in areas for l in limits])


@pytest.fixture(scope='module')
def cases():
    """kind -> (roidb, reference values [8 * len(LIMITS), G]): computed once."""
    out = {}
    for i, (kind, kw) in enumerate(sorted(KINDS.items())):
        roidb = bp.synthetic_roidb(50 + i, SHAPES, **kw)
        out[kind] = (roidb, reference_per_gt(roidb, bp.AREAS, LIMITS))
    return out


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_matching_equals_the_literal_loop(dev, cases, kind):
    roidb, want = cases[kind]
    assert want.shape == (8 * len(LIMITS), sum(g for _p, g in SHAPES))
    # the cases are there: every sentinel, matched values, zeros of gt left over
    assert (want == -1).any() and (want == -2).any() and (want == 0).any() and (want > 0.5).any()
    g = guard.carve(want.shape, torch.float32, dev)
    got = device_per_gt(roidb, bp.AREAS, LIMITS, dev, out=g.t)
    g.check('gt_iou')
    assert not guard.holds_sentinel(g.t[:, :1]) and got.dtype == np.float32
    bad = np.argwhere(got.astype(np.float64) != want)
    assert bad.size == 0, ('first difference at (setting, gt)', bad[0].tolist(), got[tuple(bad[0])],
                           want[tuple(bad[0])])
    again = device_per_gt(roidb, bp.AREAS, LIMITS, dev)
    assert got.tobytes() == again.tobytes()


def test_ties_are_broken_towards_the_lower_gt_then_the_lower_proposal(dev):
    """Two different gt tie at exactly 0.5 on one proposal: the lower gt takes it, the other is
    left with what remains (0); identical proposals: the value is the same, and the used one is
    the lower (a second identical gt then gets the second copy, not nothing)."""
    E = bp.make_entry
    roidb = [E([[0, 0, 9, 9], [0, 5, 9, 14]], [1, 1], [0, 0], [100, 100], [[0, 5, 9, 9], [0, 0, 5, 4]]),
             E([[0, 5, 9, 14], [0, 0, 9, 9]], [1, 1], [0, 0], [100, 100], [[0, 5, 9, 9], [0, 0, 5, 4]]),
             E([[20, 20, 59, 59], [20, 20, 59, 59], [20, 20, 59, 59]], [2, 2, 2], [0] * 3, [1600] * 3,
               [[22, 22, 59, 59], [22, 22, 59, 59]])]
    got = device_per_gt(roidb, ['all'], [0, 1], dev)
    x = np.float32(38 * 38) / np.float32(1600)
    assert got[0].tolist() == [0.5, 0.0, 0.5, np.float32(30) / np.float32(100), x, x, 0.0]
    assert got[1].tolist() == [0.5, 0.0, 0.5, 0.0, x, 0.0, 0.0]
    want = reference_per_gt(roidb, ['all'], [0, 1])
    assert np.array_equal(got.astype(np.float64), want)


def test_grid_stride_loop(dev):
    from naws_hip import ops
    rng = np.random.default_rng(7)
    shapes = [(int(p), int(g)) for p, g in zip(rng.integers(0, 9, 90), rng.integers(0, 5, 90))]
    roidb = bp.synthetic_roidb(8, shapes, quantum=0.5, ties=True)
    limits = [0, 1, 2, 3, 5, 8]
    assert len(roidb) * 8 * len(limits) > 4 * ops.proposal_match_max_grid()
    got = device_per_gt(roidb, bp.AREAS, limits, dev)
    assert np.array_equal(got.astype(np.float64), reference_per_gt(roidb, bp.AREAS, limits))


def test_bad_segments_touch_nothing(dev):
    """Offsets that pass the wrapper (monotone, ending at the row count) cannot leave the arrays;
    the kernel's own check is reached through the C entry with a workspace sized for shorter
    segments: the segments that exceed it keep the caller's values, the others are matched."""
    from detectron.datasets import json_dataset_evaluator as jde
    from naws_hip import lib
    roidb = bp.synthetic_roidb(3, [(5, 2), (40, 3), (6, 9), (4, 1)])
    t = [torch.from_numpy(a).to(dev) for a in jde.flatten_roidb(roidb)]
    lo, hi, lim = np.zeros(1, np.float32), np.full(1, 1e10, np.float32), np.zeros(1, np.int32)
    need = int(lib.load().naws_proposal_match_workspace_bytes(8, 4))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    out = guard.carve((1, 15), torch.float32, dev)
    out.t.fill_(7.0)
    lib.call('naws_proposal_match_fwd', t[0].data_ptr(), t[1].data_ptr(), 55, t[2].data_ptr(),
             t[3].data_ptr(), t[4].data_ptr(), 15, 4, lo.ctypes.data, hi.ctypes.data, 1, lim.ctypes.data, 1,
             8, 4, ws.data_ptr(), need, out.t.data_ptr(), torch.cuda.current_stream().cuda_stream)
    got = out.t.cpu().numpy()[0]
    out.check('gt_iou')
    want = reference_per_gt(roidb, ['all'], [0])[0]
    assert (got[2:14] == 7.0).all()                      # 40 proposals > 8; 9 gt > 4
    assert np.array_equal(got[:2].astype(np.float64), want[:2])
    assert np.array_equal(got[14:].astype(np.float64), want[14:])


def test_device_route_equals_the_recorded_reference(dev):
    from detectron.datasets import json_dataset_evaluator as jde
    fx = bp.fixture()
    roidb = bp.fixture_roidb(fx)
    stats = jde.evaluate_box_proposals_sweep(None, roidb, areas=bp.AREAS, limits=bp.FIXTURE_LIMITS,
                                             route='device')
    assert list(stats) == [(a, l) for l in bp.FIXTURE_LIMITS for a in bp.AREAS]
    for (area, limit), s in stats.items():
        if s['num_pos']:
            bp.assert_same_stats(s, bp.fixture_stats(fx, area, limit))


@pytest.fixture(scope='module')
def forty():
    rng = np.random.default_rng(40)
    shapes = [(int(p), int(g)) for p, g in zip(rng.integers(0, 150, 40), rng.integers(0, 12, 40))]
    shapes[3], shapes[7], shapes[11] = (0, 4), (30, 0), (1100, 5)       # (one image above limit 1000)
    return bp.synthetic_roidb(41, shapes, quantum=0.25, ties=True)


class _Dataset(object):
    name = 'toy_2007_test'


def test_task_evaluation_device_equals_host(dev, forty, cfgmod, caplog):
    from detectron.datasets import json_dataset_evaluator as jde, task_evaluation
    host = task_evaluation.evaluate_box_proposals(_Dataset(), forty, route='host')
    with caplog.at_level(logging.INFO):
        device = task_evaluation.evaluate_box_proposals(_Dataset(), forty)       # the default route
    assert 'Box proposal recall: device route (HIP kernel)' in caplog.text
    assert device == host and list(device['toy_2007_test']['box_proposal']) == list(
        host['toy_2007_test']['box_proposal'])
    for k, v in device['toy_2007_test']['box_proposal'].items():
        assert np.float64(v).tobytes() == np.float64(host['toy_2007_test']['box_proposal'][k]).tobytes()
    assert 0 < device['toy_2007_test']['box_proposal']['AR@100'] < 1
    limits, areas = (None, 1, 100, 1000), bp.AREAS
    a = jde.evaluate_box_proposals_sweep(None, forty, areas=areas, limits=limits, route='host')
    b = jde.evaluate_box_proposals_sweep(None, forty, areas=areas, limits=limits, route='device')
    assert list(a) == list(b)
    for key in a:
        if a[key]['num_pos']:
            bp.assert_same_stats(a[key], b[key])
        else:
            assert b[key]['num_pos'] == 0 and len(b[key]['gt_overlaps']) == 0
