#!/usr/bin/env python3
"""Time the test-time grid search (detectron/core/grid_search_wsl.py) on seeded synthetic
candidates of VOC07-test size - 4952 images, 20 classes, 2000 boxes per image, 1 to 6 annotated
objects per image:

  device route  the full default grid (11 x 10 x 5 = 550 settings), per stage: the one-time host
                preparation (visiting orders, the rounded numbers), upload + the three sort
                orders, the NMS pass (naws_nms_multi_fwd), the cut tables (naws_grid_cut_fwd),
                the per-setting selection and the evaluation (naws_voc_match_fwd /
                naws_voc_ap_fwd) - wall seconds and device-event milliseconds each;
  host route    the literal loop over the named sub-grid (--host-settings) on the first
                --host-images images; its seconds per setting are scaled by images / host-images
                to the full set (the loop is linear in the images), NOT run for 550 settings.

    python tools/bench_grid_search.py [--images 4952] [--boxes 2000] [--live 0.05] [--skip-host]

--live is the share of (box, class) scores above the smallest score threshold of the grid (1e-10):
only those are candidates.  Prints one JSON line; the two routes are compared on the host subset
(n_dets, mAP and mCorLoc of every named setting must be equal)."""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def synthetic(n_images, n_classes, n_boxes, live, seed, width=500, height=375):
    """-> (recs, names, classes, candidates).  Half of the boxes are jittered copies of an
    annotated object (so NMS has clusters to thin out), the rest proposals anywhere; a live score
    is 10^U(-10, 0), raised for the object's class on its copies, a dead one 10^U(-30, -10)."""
    rng = np.random.default_rng(seed)
    names = ['%06d' % (i + 1) for i in range(n_images)]
    classes = ['__background__'] + ['class%02d' % k for k in range(n_classes)]
    recs, cands = {}, []
    k = n_classes + 1
    for name in names:
        m = int(rng.integers(1, 7))
        xy = rng.integers(1, width - 120, (m, 2))
        wh = rng.integers(20, 200, (m, 2))
        cls = rng.integers(1, k, m)
        dif = rng.random(m) < 0.15
        recs[name] = [{'name': classes[int(c)], 'pose': 'Unspecified', 'truncated': 0, 'difficult': int(d),
                       'bbox': [int(p[0]), int(p[1]), int(p[0] + s[0]), int(p[1] + s[1])]}
                      for c, d, p, s in zip(cls, dif, xy, wh)]
        gt = np.concatenate([xy, xy + wh], 1).astype(np.float64) - 1
        near = rng.random(n_boxes) < 0.5
        pick = rng.integers(0, m, n_boxes)
        jit = gt[pick] + np.round(rng.normal(0, 10, (n_boxes, 4)))
        p = rng.integers(0, width - 40, (n_boxes, 2))
        far = np.concatenate([p, p + rng.integers(20, 250, (n_boxes, 2))], 1).astype(np.float64)
        boxes = np.where(near[:, None], jit, far)
        boxes[:, 2:] = np.maximum(boxes[:, 2:], boxes[:, :2] + 1)
        expo = np.where(rng.random((n_boxes, k)) < live, rng.uniform(-10, 0, (n_boxes, k)),
                        rng.uniform(-30, -10.5, (n_boxes, k)))
        hit = np.flatnonzero(near)
        expo[hit, cls[pick[hit]]] = rng.uniform(-3, 0, len(hit))
        scores = (10.0 ** expo).astype(np.float32)
        scores[:, 0] = -1
        cands.append((scores, boxes.astype(np.float32)))
    return recs, names, classes, cands


def parse_settings(text):
    out = []
    for part in text.split(';'):
        a, b, c = part.split(',')
        out.append((float(a), float(b), int(c)))
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--images', type=int, default=4952)
    p.add_argument('--classes', type=int, default=20)
    p.add_argument('--boxes', type=int, default=2000)
    p.add_argument('--live', type=float, default=0.05)
    p.add_argument('--seed', type=int, default=2007)
    p.add_argument('--host-images', type=int, default=200)
    p.add_argument('--host-settings', type=parse_settings, default=parse_settings('0.5,1e-9,100;0.3,1e-5,10000'),
                   help='NMS,SCORE_THRESH,DETECTIONS_PER_IM;... the sub-grid of the host route')
    p.add_argument('--skip-host', action='store_true')
    p.add_argument('--skip-device', action='store_true')
    args = p.parse_args(argv)
    import logging
    logging.basicConfig(level=logging.INFO, format='%(levelname)s %(filename)s:%(lineno)4d: %(message)s')
    import torch
    from detectron.core.config import cfg
    from detectron.core import grid_search_wsl as gs
    cfg.TEST.BBOX_REG = False
    t0 = time.perf_counter()
    recs, names, classes, cands = synthetic(args.images, args.classes, args.boxes, args.live, args.seed)
    out = OrderedDict(images=args.images, classes=args.classes, boxes=args.boxes, live=args.live,
                      build_s=time.perf_counter() - t0)
    device = torch.cuda.is_available() and not args.skip_device
    full = (list(gs.DEFAULT_NMSES), list(gs.DEFAULT_THRESHS), list(gs.DEFAULT_LIMITS))
    if device:
        h = max(1, min(8, args.images))                           # loads the kernels, warms the allocator
        gs.grid_search_arrays(recs, names[:h], classes, cands[:h], *full, route='device')
        timings = OrderedDict()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = gs.grid_search_arrays(recs, names, classes, cands, *full, route='device', timings=timings)
        out['device_total_s'] = time.perf_counter() - t0
        out['device'] = timings
        n_set = len(rows)
        out['device_s_per_setting'] = out['device_total_s'] / n_set
        sweep = sum(timings[k + '_wall_s'] for k in ('select', 'eval'))
        out['device_s_per_setting_without_one_time_work'] = sweep / n_set
        best = rows[gs.best_setting(rows)]
        out['best'] = [best['nms'], best['score_thresh'], best['detections_per_im'], best['mAP']]
        out['n_dets_min_max'] = [min(r['n_dets'] for r in rows), max(r['n_dets'] for r in rows)]
    if not args.skip_host:
        h = max(1, min(args.host_images, args.images))
        sub = {n: recs[n] for n in names[:h]}
        per, agree = [], True
        for s in args.host_settings:
            lists = [[v] for v in s]
            t0 = time.perf_counter()
            hr = gs.grid_search_arrays(sub, names[:h], classes, cands[:h], *lists, route='host')[0]
            per.append(time.perf_counter() - t0)
            if device:
                dr = gs.grid_search_arrays(sub, names[:h], classes, cands[:h], *lists, route='device')[0]
                agree = agree and all(hr[k] == dr[k] for k in ('n_dets', 'mAP', 'mCorLoc'))
        out['host_images'] = h
        out['host_settings'] = [list(s) for s in args.host_settings]
        out['host_s_per_setting_on_subset'] = per
        scale = args.images / float(h)
        out['host_s_per_setting_extrapolated'] = float(np.mean(per)) * scale
        if device:
            out['routes_agree_on_subset'] = bool(agree)
            assert agree, 'the two routes disagree on the host subset'
            out['host_over_device_per_setting'] = (out['host_s_per_setting_extrapolated'] /
                                                   out['device_s_per_setting'])
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
