"""RoIIoU pinned on integer-valued boxes by the one piece of reference code
that compiles untouched: detectron/utils/cython_bbox.pyx, compiled by `make -C oracle ref` and run
on these very boxes by tests/golden/make_golden_bbox_overlaps.py.  Its results are recorded in
tests/golden/reference_bbox_overlaps.npz as the SHA-256 of each matrix (bit-for-bit equality)
and its values at seeded positions (where a mismatch lies).

detectron/ops/roi_iou_op.cu:27-62 truncates the coordinates to int, takes w, h = int(max(d + 1., 0.)),
inters = w * h, uni = areas - inters and divides in float; cython_bbox.pyx:bbox_overlaps does the
same +1 arithmetic on the float32 coordinates themselves.  On integer-valued boxes whose areas stay
below 2^24 (every box of a 600 x 1000 or 1200 x 2000 image: the bench proposals, MCG's uint16 boxes)
every intermediate is an exact integer in both, so the two must agree BIT FOR BIT off the diagonal
(the diagonal is forced to 1 by the operator and is 1 by arithmetic in bbox_overlaps).  On
fractional coordinates (rois after x im_scale) they differ exactly where the truncation changes the
boxes: RoIIoU(frac) == bbox_overlaps(trunc(frac)).

The HIP kernel is held bit-exact to the oracle in tests/test_gpu_ops.py::test_roi_iou_bitexact and,
below (GPU), to the compiled reference module's results directly."""
import hashlib
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'reference_bbox_overlaps.npz')


def _ref():
    return np.load(GOLD)


def _sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _assert_is_reference(got, key):
    """`got` (flattened) is bit for bit the recorded reference matrix `key`."""
    got = got.reshape(-1)
    ref = _ref()
    idx, val = ref[key + '_idx'], ref[key + '_val']
    assert got.dtype == val.dtype == np.float32
    bad = got[idx].view(np.int32) != val.view(np.int32)
    assert not bad.any(), '%d of %d sampled entries differ, first at flat index %d' % (
        bad.sum(), len(idx), idx[bad][0])
    assert _sha256(got) == str(ref[key + '_sha256']), 'differs from the reference off the sample'


def _rois(boxes):
    r = np.zeros((boxes.shape[0], 5), np.float32)
    r[:, 1:] = boxes
    return r


def _int_boxes(rng, n, h, w):
    x1 = rng.integers(0, w - 2, n)
    y1 = rng.integers(0, h - 2, n)
    x2 = np.minimum(x1 + rng.integers(0, w, n), w - 1)
    y2 = np.minimum(y1 + rng.integers(0, h, n), h - 1)
    return np.stack([x1, y1, x2, y2], 1).astype(np.float32)


def _bench_boxes(n, h, w, seed):
    from detectron.datasets import synthetic
    e = synthetic.make_roidb(1, n, 20, h, w, seed=seed)[0]
    b = np.asarray(e['boxes'], np.float32)
    assert np.array_equal(b, np.floor(b))           # the bench proposals are integer-valued
    return b


CASES = [('random 2500 in 600x1000', lambda: _int_boxes(np.random.default_rng(5), 2500, 600, 1000)),
         ('random 2100 in 1200x2000', lambda: _int_boxes(np.random.default_rng(6), 2100, 1200, 2000)),
         ('bench proposals 2000', lambda: _bench_boxes(2000, 600, 1000, 11)),
         ('bench proposals 4000 (configs[4])', lambda: _bench_boxes(4000, 375, 500, 11)),
         ('degenerate: 1-px boxes, duplicates, touching edges',
          lambda: np.array([[0, 0, 0, 0], [0, 0, 0, 0], [5, 5, 5, 9], [5, 9, 8, 9], [0, 0, 999, 599],
                            [999, 599, 999, 599], [10, 10, 19, 19], [20, 10, 29, 19],
                            [19, 19, 30, 30]], np.float32))]


def fractional_boxes():
    """(fractional boxes, the same boxes truncated) of the fractional-coordinates test."""
    b = _int_boxes(np.random.default_rng(9), 700, 600, 1000)
    scale = np.float32(600.0 / 375.0)               # what _project_im_rois multiplies by
    bf = (b * scale).astype(np.float32)
    return bf, np.trunc(bf).astype(np.float32)


@pytest.mark.parametrize('name,make', CASES, ids=[c[0] for c in CASES])
def test_oracle_roi_iou_equals_compiled_reference_bbox_overlaps_on_integer_boxes(name, make):
    from oracle import oracle
    b = make()
    j = oracle.roi_iou(_rois(b))
    # J[j, i] of boxes (i, j): both symmetric; compare whole matrices bit for bit
    _assert_is_reference(j, 'int%d' % [c[0] for c in CASES].index(name))
    assert (np.diag(j) == 1.0).all()
    # not a vacuous comparison: a fair share of pairs overlap
    assert (j[~np.eye(len(b), dtype=bool)] > 0).mean() > 0.02 or len(b) < 16


def test_oracle_roi_iou_on_fractional_boxes_is_the_reference_on_truncated_boxes():
    """Fractional coordinates: RoIIoU truncates first (roi_iou_op.cu:32-39), bbox_overlaps does
    not - so RoIIoU(b) == bbox_overlaps(trunc(b)) bit for bit, and it differs from
    bbox_overlaps(b) exactly on pairs whose truncated boxes give another quotient."""
    from oracle import oracle
    bf, _tr = fractional_boxes()
    assert (bf != np.floor(bf)).any()
    j = oracle.roi_iou(_rois(bf))
    off = ~np.eye(len(bf), dtype=bool)
    _assert_is_reference(j[off], 'frac_trunc')
    # (so it differs from bbox_overlaps(b) exactly where bbox_overlaps(trunc(b)) does; the sample
    # holds such pairs)
    ref = _ref()
    idx, ov_t, ov_f = ref['frac_float_idx'], ref['frac_trunc_val'], ref['frac_float_val']
    differs = j[off][idx] != ov_f
    assert np.array_equal(differs, ov_t != ov_f)
    assert differs.any() and int(ref['frac_n_differ']) > 0     # truncation does matter on these boxes
    # known answer of SURVEY.md appendix B: 148.5 -> 148
    k = oracle.roi_iou(_rois(np.array([[148.5, 10.2, 200.9, 60.7], [148, 10, 200, 60]], np.float32)))
    assert k[0, 1] == 1.0 and k[1, 0] == 1.0


@pytest.mark.gpu
@pytest.mark.parametrize('name,make', CASES[:4], ids=[c[0] for c in CASES[:4]])
def test_hip_roi_iou_equals_compiled_reference_bbox_overlaps_on_integer_boxes(name, make, dev):
    """The product kernel (naws_roi_iou_fwd through detectron.ops.RoIIoU) against the compiled
    reference module's results, no restatement in between."""
    import torch
    from naws_hip import ops
    b = make()
    j = ops.roi_iou(torch.from_numpy(_rois(b)).to(dev)).cpu().numpy()
    _assert_is_reference(j, 'int%d' % [c[0] for c in CASES].index(name))
