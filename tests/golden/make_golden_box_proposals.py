#!/usr/bin/env python3
"""Record the reference's own evaluate_box_proposals (detectron/datasets/json_dataset_evaluator.py
:255-336) on a small synthetic roidb, for all 8 area ranges x limits {None, 1, 3, 100}.

Runs ONLY where the reference tree is present and oracle/_ref has been built (`make -C oracle
ref`).  The reference file is imported by path and run as it is; what it imports from the rest of
that tree is stubbed: pycocotools, the config object and detectron.utils.io (all unused by the
function called), and detectron.utils.boxes by a module whose bbox_overlaps is the reference's
compiled cython_bbox.

Writes tests/golden/reference_box_proposals.npz (data only):
  n_images, thresholds
  im<i>_boxes / _gt_classes / _is_crowd / _seg_areas          the roidb entries
  <area>_<limit>_ar / _recalls / _gt_overlaps / _num_pos      limit 'none', 1, 3, 100

The roidb (ROIDB below): an image with gt and no proposals; one without gt; crowd gt; more valid
gt than proposals; identical proposals and identical gt; two DIFFERENT gt that tie at an overlap
of exactly 0.5 on one proposal (10x10 boxes, a 10x5 proposal inside both) with a second proposal
that only the first reaches; a proposal beyond limits 1 and 3 that beats the early ones; gt areas
exactly 32^2, 96^2 and 128^2; non-integer coordinates; 120 proposals (more than limit 100).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_box_proposals.py
"""
import glob
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get('REF', '/root/reference')
sys.path[:0] = [os.path.dirname(HERE)]


def roidb():
    import box_proposals_ref as bp
    E = bp.make_entry
    rng = np.random.default_rng(23)
    db = []
    # 0: gt, no proposals; areas exactly 32^2 (small AND medium)
    db.append(E([[10, 10, 41, 41], [50, 60, 200, 220]], [3, 7], [0, 0], [32 * 32, 151 * 161], []))
    # 1: no gt
    db.append(E([], [], [], [], [[5, 5, 60, 60], [1, 2, 30, 40], [100, 100, 180, 150]]))
    # 2: a crowd region the best proposal sits on, and a plain box
    db.append(E([[20, 20, 120, 120], [150, 30, 220, 100]], [5, 5], [1, 0], [101 * 101, 71 * 71],
                [[20, 20, 120, 120], [152, 33, 221, 98], [150, 30, 190, 100]]))
    # 3: five valid gt, four proposals; proposal 3 is the only good one for gt 0 (limits 1 and 3
    # cut it off); gt 4 is reached by nothing
    db.append(E([[10, 10, 110, 90], [130, 20, 230, 120], [20, 140, 100, 230], [250, 250, 330, 300],
                 [400, 400, 460, 470]], [1, 2, 3, 4, 5], [0] * 5,
                [101 * 81, 101 * 101, 81 * 91, 81 * 51, 61 * 71],
                [[128, 25, 225, 118], [25, 150, 90, 228], [255, 240, 340, 310], [11, 12, 108, 88]]))
    # 4: identical proposals and identical gt
    db.append(E([[20, 20, 59, 59], [20, 20, 59, 59], [100, 100, 180, 170]], [2, 2, 9], [0] * 3,
                [40 * 40, 40 * 40, 81 * 71],
                [[22, 22, 59, 59], [22, 22, 59, 59], [95, 105, 175, 172], [20, 20, 59, 59]]))
    # 5: two different 10x10 gt, a 10x5 proposal inside both (0.5 exactly with each), and a
    # proposal that overlaps only the first
    db.append(E([[0, 0, 9, 9], [0, 5, 9, 14]], [4, 4], [0, 0], [100, 100],
                [[0, 5, 9, 9], [0, 0, 5, 4]]))
    # 6: areas exactly 96^2 (medium, large, 96-128) and 128^2 (large, 96-128, 128-256)
    db.append(E([[0, 0, 95, 95], [100, 0, 227, 127], [300, 300, 899, 899]], [6, 6, 8], [0] * 3,
                [96 * 96, 128 * 128, 600 * 600],
                [[2, 3, 97, 94], [101, 4, 220, 125], [310, 290, 880, 905], [0, 0, 227, 127]]))
    # 7: non-integer coordinates, 120 proposals
    db.append(bp.synthetic_entry(rng, 120, 6))
    # 8: quarter-pixel coordinates with ties, more gt than limit 3
    db.append(bp.synthetic_entry(rng, 9, 7, quantum=0.25, ties=True))
    return db


def load_reference():
    so = glob.glob(os.path.join(ROOT, 'oracle', '_ref', 'cython_bbox*.so'))
    if not so:
        sys.exit('oracle/_ref/cython_bbox not built: make -C oracle ref')
    spec = importlib.util.spec_from_file_location('cython_bbox', so[0])
    cython_bbox = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cython_bbox)
    for name in ('pycocotools', 'pycocotools.cocoeval', 'detectron', 'detectron.core',
                 'detectron.core.config', 'detectron.utils', 'detectron.utils.io',
                 'detectron.utils.boxes'):
        sys.modules[name] = types.ModuleType(name)
    sys.modules['pycocotools.cocoeval'].COCOeval = None
    sys.modules['detectron.core.config'].cfg = None
    sys.modules['detectron.utils.io'].save_object = None
    sys.modules['detectron.utils.boxes'].bbox_overlaps = cython_bbox.bbox_overlaps
    sys.modules['detectron.utils'].boxes = sys.modules['detectron.utils.boxes']
    path = os.path.join(REFERENCE, 'detectron', 'datasets', 'json_dataset_evaluator.py')
    spec = importlib.util.spec_from_file_location('detectron.datasets.json_dataset_evaluator', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    sys.dont_write_bytecode = True
    if not os.path.isdir(REFERENCE):
        sys.exit('the reference tree is not on this machine')
    import box_proposals_ref as bp
    ref = load_reference()
    db = roidb()
    out = {'n_images': np.array(len(db)), 'thresholds': bp.THRESHOLDS}
    for i, e in enumerate(db):
        for k, v in e.items():
            out['im%d_%s' % (i, k)] = v
    for area in bp.AREAS:
        for limit in bp.FIXTURE_LIMITS:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')              # 0 / 0 of a range without gt
                r = ref.evaluate_box_proposals(None, db, area=area, limit=limit)
            key = '%s_%s_' % (area, 'none' if limit is None else limit)
            assert np.array_equal(r['thresholds'], bp.THRESHOLDS)
            out[key + 'ar'] = np.float64(r['ar'])
            out[key + 'recalls'] = r['recalls']
            out[key + 'gt_overlaps'] = r['gt_overlaps']
            out[key + 'num_pos'] = np.int64(r['num_pos'])
            print('%-8s limit %-4s num_pos %2d recorded %2d ar %.6f'
                  % (area, limit, r['num_pos'], len(r['gt_overlaps']), r['ar']))
    np.savez_compressed(os.path.join(HERE, 'reference_box_proposals.npz'), **out)
    print('wrote reference_box_proposals.npz (%d arrays)' % len(out))


if __name__ == '__main__':
    main()
