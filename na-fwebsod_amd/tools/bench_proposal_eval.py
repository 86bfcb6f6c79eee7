#!/usr/bin/env python3
"""Time the box-proposal recall (detectron/datasets/json_dataset_evaluator.py) on a seeded
synthetic roidb of VOC07-test size - 4952 images, 2000 proposals each, 1 to 6 ground-truth boxes
per image and every 50th image with dozens - on the host route (the numpy loop, one pass per
setting) and on the device route (csrc/proposal_eval_ops.hip: every image under every setting in
one launch), for the reference's 8 settings (4 areas x limits 100, 1000) and for a sweep of 8
areas x 6 limits, and check that the two routes agree.

    python tools/bench_proposal_eval.py [--images 4952] [--proposals 2000] [--repeat 3]
        [--skip-host] [--skip-host-sweep]

Prints one JSON line: per stage the host seconds and the device route's seconds split into
flatten (roidb -> arrays, on the CPU), upload, kernel (launch to completion) and host tail (counts,
sort, download); the device route's first call, which loads the kernel, is reported apart from the
best of the repeats.  A report, not a gate."""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

STAGES = OrderedDict([
    ('reference8', (('all', 'small', 'medium', 'large'), (100, 1000))),
    ('sweep48', (('all', 'small', 'medium', 'large', '96-128', '128-256', '256-512', '512-inf'),
                 (10, 100, 300, 1000, 2000, None))),
])


def synthetic_roidb(n_images, n_props, seed):
    rng = np.random.default_rng(seed)
    roidb = []
    for i in range(n_images):
        g = int(rng.integers(24, 60)) if i % 50 == 49 else int(rng.integers(1, 7))
        xy = rng.integers(0, 380, (g, 2))
        wh = rng.integers(12, 700, (g, 2))
        gt = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        near = rng.random(n_props) < 0.3
        pick = rng.integers(0, g, n_props)
        jit = np.round(gt[pick] + rng.normal(0, 15, (n_props, 4)))
        p = rng.integers(0, 400, (n_props, 2))
        far = np.concatenate([p, p + rng.integers(20, 650, (n_props, 2))], 1)
        props = np.where(near[:, None], jit, far).astype(np.float32)
        seg = ((wh[:, 0] + 1) * (wh[:, 1] + 1) * rng.uniform(0.4, 1.0, g)).astype(np.float32)
        crowd = rng.random(g) < 0.03
        roidb.append({
            'boxes': np.concatenate([gt, props]),
            'gt_classes': np.concatenate([rng.integers(1, 21, g).astype(np.int32), np.zeros(n_props, np.int32)]),
            'is_crowd': np.concatenate([crowd, np.zeros(n_props, bool)]),
            'seg_areas': np.concatenate([seg, np.zeros(n_props, np.float32)])})
    return roidb


def same(a, b):
    return (a['num_pos'] == b['num_pos'] and np.array_equal(a['gt_overlaps'], b['gt_overlaps'])
            and a['recalls'].tobytes() == b['recalls'].tobytes()
            and np.float64(a['ar']).tobytes() == np.float64(b['ar']).tobytes())


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--images', type=int, default=4952)
    p.add_argument('--proposals', type=int, default=2000)
    p.add_argument('--repeat', type=int, default=3)
    p.add_argument('--seed', type=int, default=2007)
    p.add_argument('--skip-host', action='store_true')
    p.add_argument('--skip-host-sweep', action='store_true', help='time the host route on the 8 settings only')
    args = p.parse_args(argv)
    import torch
    from detectron.datasets import json_dataset_evaluator as jde
    roidb = synthetic_roidb(args.images, args.proposals, args.seed)
    out = OrderedDict(images=args.images, proposals_per_image=args.proposals,
                      gt=int(sum((e['gt_classes'] > 0).sum() for e in roidb)))
    for stage, (areas, limits) in STAGES.items():
        r = OrderedDict(settings=len(areas) * len(limits))
        host = None
        if not args.skip_host and not (args.skip_host_sweep and stage != 'reference8'):
            t0 = time.perf_counter()
            host = jde.evaluate_box_proposals_sweep(None, roidb, areas=areas, limits=limits, route='host')
            r['host_s'] = time.perf_counter() - t0
        if torch.cuda.is_available():
            runs = []
            for _ in range(1 + max(1, args.repeat)):
                tm = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dev = jde.evaluate_box_proposals_sweep(None, roidb, areas=areas, limits=limits,
                                                       route='device', timings=tm)
                tm['total_s'] = time.perf_counter() - t0
                runs.append(tm)
            r['device_first_s'] = runs[0]['total_s']
            best = min(runs[1:], key=lambda t: t['total_s'])
            r['device_s'] = best['total_s']
            for k in ('flatten_s', 'upload_s', 'kernel_s', 'tail_s'):
                r['device_' + k] = best[k]
            r['AR@100'] = float(dev[('all', 100)]['ar'])
            if host is not None:
                assert list(host) == list(dev)
                assert all(same(host[k], dev[k]) for k in host), 'the routes differ'
                r['routes_agree'] = True
                r['speedup'] = r['host_s'] / r['device_s']
        out[stage] = r
    print(json.dumps(out))
    return out


if __name__ == '__main__':
    main()
