"""Independent reference of the box-proposal matching (a helper module of the tests, used where the
reference tree is absent): the literal loop of json_dataset_evaluator.py:286-323 - a dense
overlap matrix, argmax / max, marking with -1 - written from the reference's text, keeping the
value PER ground-truth box with the kernel's sentinels:

    matched: its overlap;  valid and never matched: 0;  outside the area range: -1;
    valid but the image has no proposals: -2.

Also three deliberately wrong matchings (the test of the test), the fixture's loader and the
seeded synthetic roidbs of the GPU tests."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'reference_box_proposals.npz')

AREAS = ('all', 'small', 'medium', 'large', '96-128', '128-256', '256-512', '512-inf')
RANGES = {'all': (0**2, 1e5**2), 'small': (0**2, 32**2), 'medium': (32**2, 96**2),
          'large': (96**2, 1e5**2), '96-128': (96**2, 128**2), '128-256': (128**2, 256**2),
          '256-512': (256**2, 512**2), '512-inf': (512**2, 1e5**2)}
FIXTURE_LIMITS = (None, 1, 3, 100)
THRESHOLDS = np.arange(0.5, 0.95 + 1e-5, 0.05)


def overlaps_matrix(boxes, gt):
    """cython_bbox.pyx:27-63 element by element in numpy scalars (not the product's vectorised
    restatement): float32 differences, `+ 1` and products in double, float32 stores."""
    f32, f64 = np.float32, np.float64
    out = np.zeros((len(boxes), len(gt)), f32)
    for k in range(len(gt)):
        q = [f32(v) for v in gt[k]]
        qa = f32((f64(q[2] - q[0]) + 1.0) * (f64(q[3] - q[1]) + 1.0))
        for n in range(len(boxes)):
            b = [f32(v) for v in boxes[n]]
            iw = f32(f64(min(b[2], q[2]) - max(b[0], q[0])) + 1.0)
            if iw > 0:
                ih = f32(f64(min(b[3], q[3]) - max(b[1], q[1])) + 1.0)
                if ih > 0:
                    ua = f32((f64(b[2] - b[0]) + 1.0) * (f64(b[3] - b[1]) + 1.0) + f64(qa) - f64(iw * ih))
                    out[n, k] = (iw * ih) / ua
    return out


def split_entry(entry):
    gt_inds = np.where((entry['gt_classes'] > 0) & (entry['is_crowd'] == 0))[0]
    props = entry['boxes'][np.where(entry['gt_classes'] == 0)[0]].astype(np.float32)
    return props, entry['boxes'][gt_inds].astype(np.float32), entry['seg_areas'][gt_inds]


def match_image(props, gt, valid, limit, overlaps=None, mode='reference'):
    """Per-gt values of one image; `valid` a bool mask over gt.  mode: 'reference', or one of the
    wrong matchings 'tie_high_gt', 'no_marking', 'limit_after'."""
    out = np.where(valid, 0.0, -1.0)
    vi = np.where(valid)[0]
    if len(props) == 0:
        out[vi] = -2.0
        return out
    full = overlaps if overlaps is not None else overlaps_matrix(props, gt)
    cut = len(props) if limit is None else min(limit, len(props))
    rows = len(props) if mode == 'limit_after' else cut
    ov = full[:rows][:, vi].astype(np.float32).copy()
    if mode == 'no_marking':
        if len(vi):
            out[vi] = ov.max(axis=0)
        return out
    for _j in range(min(ov.shape[0], ov.shape[1])):
        argmax_overlaps = ov.argmax(axis=0)
        max_overlaps = ov.max(axis=0)
        if mode == 'tie_high_gt':
            gt_ind = len(max_overlaps) - 1 - max_overlaps[::-1].argmax()
        else:
            gt_ind = max_overlaps.argmax()
        box_ind = argmax_overlaps[gt_ind]
        val = ov[box_ind, gt_ind]
        assert val >= 0
        if not (mode == 'limit_after' and box_ind >= cut):
            out[vi[gt_ind]] = val
        ov[box_ind, :] = -1
        ov[:, gt_ind] = -1
    return out


def per_gt(roidb, area, limit, mode='reference', cache=None):
    """The per-gt values of every image, concatenated in roidb order."""
    lo, hi = RANGES[area]
    vals = []
    for i, entry in enumerate(roidb):
        props, gt, areas = split_entry(entry)
        full = None
        if cache is not None:
            if i not in cache:
                cache[i] = overlaps_matrix(props, gt)
            full = cache[i]
        vals.append(match_image(props, gt, (areas >= lo) & (areas <= hi), limit, full, mode))
    return np.concatenate(vals) if vals else np.zeros(0)


def summarize(values):
    """The reference's tail from per-gt values."""
    num_pos = int((values != -1).sum())
    gt_overlaps = np.sort(values[values >= 0].astype(np.float64))
    recalls = np.zeros_like(THRESHOLDS)
    with np.errstate(invalid='ignore', divide='ignore'):
        for i, t in enumerate(THRESHOLDS):
            recalls[i] = (gt_overlaps >= t).sum() / float(num_pos)
    return {'ar': recalls.mean(), 'recalls': recalls, 'thresholds': THRESHOLDS,
            'gt_overlaps': gt_overlaps, 'num_pos': num_pos}


def evaluate(roidb, area='all', limit=None, mode='reference', cache=None):
    return summarize(per_gt(roidb, area, limit, mode, cache))


def assert_same_stats(a, b):
    assert a['num_pos'] == b['num_pos']
    assert a['gt_overlaps'].dtype == b['gt_overlaps'].dtype == np.float64
    assert np.array_equal(a['gt_overlaps'], b['gt_overlaps'])
    assert np.array_equal(a['thresholds'], b['thresholds'])
    assert np.asarray(a['recalls']).tobytes() == np.asarray(b['recalls']).tobytes()
    assert np.float64(a['ar']).tobytes() == np.float64(b['ar']).tobytes()


def make_entry(gt_boxes, gt_classes, is_crowd, seg_areas, props):
    gt_boxes = np.asarray(gt_boxes, np.float32).reshape(-1, 4)
    props = np.asarray(props, np.float32).reshape(-1, 4)
    n = len(props)
    return {'boxes': np.concatenate([gt_boxes, props]),
            'gt_classes': np.concatenate([np.asarray(gt_classes, np.int32).reshape(-1), np.zeros(n, np.int32)]),
            'is_crowd': np.concatenate([np.asarray(is_crowd, bool).reshape(-1), np.zeros(n, bool)]),
            'seg_areas': np.concatenate([np.asarray(seg_areas, np.float32).reshape(-1), np.zeros(n, np.float32)])}


def fixture():
    return np.load(FIXTURE)


def fixture_roidb(fx):
    return [{k: fx['im%d_%s' % (i, k)] for k in ('boxes', 'gt_classes', 'is_crowd', 'seg_areas')}
            for i in range(int(fx['n_images']))]


def fixture_stats(fx, area, limit):
    key = '%s_%s_' % (area, 'none' if limit is None else limit)
    return {'ar': fx[key + 'ar'][()], 'recalls': fx[key + 'recalls'], 'thresholds': fx['thresholds'],
            'gt_overlaps': fx[key + 'gt_overlaps'], 'num_pos': int(fx[key + 'num_pos'])}


def random_boxes(rng, n, quantum=None, size=(8., 700.), extent=900.):
    xy = rng.uniform(0, extent, (n, 2))
    wh = rng.uniform(size[0], size[1], (n, 2))
    b = np.concatenate([xy, xy + wh], 1)
    if quantum:
        b = np.round(b / quantum) * quantum
    return b.astype(np.float32)


def synthetic_entry(rng, p, g, quantum=None, ties=False):
    """g ground-truth boxes (a crowd one and a background-class... none: all count) and p
    proposals, half of them jittered copies of gt; seg_areas spread over every area range and
    some exactly on a bound; ties: duplicated proposals and duplicated gt."""
    gt = random_boxes(rng, g, quantum)
    props = random_boxes(rng, p, quantum)
    if g and p:
        near = rng.random(p) < 0.5
        pick = rng.integers(0, g, p)
        jit = gt[pick] + rng.normal(0, 12, (p, 4)).astype(np.float32)
        if quantum:
            jit = np.round(jit / quantum) * quantum
        props = np.where(near[:, None], jit, props).astype(np.float32)
    if ties:
        if p >= 4:
            props[p // 2] = props[0]
            props[p - 1] = props[1]
        if g >= 3:
            gt[g - 1] = gt[0]
            if p >= 2:
                props[1] = gt[0]
    w, h = gt[:, 2] - gt[:, 0] + 1, gt[:, 3] - gt[:, 1] + 1
    seg = (w * h * rng.uniform(0.3, 1.0, g)).astype(np.float32)
    bounds = np.array([32**2, 96**2, 128**2, 256**2, 512**2], np.float32)
    on = rng.random(g) < 0.2
    seg = np.where(on, bounds[rng.integers(0, len(bounds), g)], seg).astype(np.float32)
    return make_entry(gt, rng.integers(1, 21, g), np.zeros(g, bool), seg, props)


def synthetic_roidb(seed, shapes, quantum=None, ties=False):
    rng = np.random.default_rng(seed)
    return [synthetic_entry(rng, p, g, quantum, ties) for p, g in shapes]
