#!/usr/bin/env python3
"""RoIAlign next to RoIPoolF at the bench shape: 1 x 74 x 124 x 512 features (NCHW at the op layer,
as the executor calls them) and the 2000 proposals the synthetic roidb gives a 600 x 1000 image.

  ops    O.RoIAlign / O.RoIAlignGradient at sampling_ratio 0 and 2 and O.RoIPoolF /
         O.RoIPoolFGradient, the legs interleaved round by round in one process, device-event
         times; then the two RoIAlign entries alone on NHWC (no transposes) with the proposals'
         mean weighted-pixel count, the atomic bytes it implies and the rate that comes out
  steps  one na_wsddn training iteration on the op-by-op plan: RoIPoolF, RoIAlign at
         sampling_ratio 2 and 0, body frozen and trainable, interleaved the same way

    timeout -k 10 600 python tools/bench_roi_align.py [--rounds 5] [--reps 5] [--steps 3]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from detectron.core import config as c  # noqa: E402
from detectron.core.executor import NetExecutor  # noqa: E402
from detectron.datasets import synthetic  # noqa: E402
import detectron.modeling.model_builder_wsl as mbld  # noqa: E402
import detectron.ops as O  # noqa: E402
from naws_hip import ops  # noqa: E402

YAML = os.path.join(ROOT, 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
H, W, C, SCALE, PH, PW = 74, 124, 512, 0.125, 7, 7


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def report(name, ts, extra=''):
    ts = sorted(ts)
    print('%-44s median %8.3f ms (min %.3f, max %.3f, n = %d)%s'
          % (name, ts[len(ts) // 2], ts[0], ts[-1], len(ts), extra), flush=True)
    return ts[len(ts) // 2]


def weighted_pixels(rois, sampling):
    """Mean over the rois of (rows that carry a weight) x (columns that carry one): the pixels
    RoIAlignGradient adds to per channel, counted on the host by the geometry of include/naws.h
    (float32, as the kernel)."""
    f32 = np.float32
    tot = 0
    for roi in rois.astype(f32):
        n_axis = []
        for lo_c, hi_c, bins, L in ((roi[2], roi[4], PH, H), (roi[1], roi[3], PW, W)):
            s, e = lo_c * f32(SCALE), hi_c * f32(SCALE)
            r = max(e - s, f32(1.0))
            b = f32(r / f32(bins))
            g = sampling if sampling > 0 else int(np.ceil(f32(r / f32(bins))))
            p = np.arange(bins, dtype=f32)[:, None]
            i = np.arange(g, dtype=f32)[None, :]
            y = (s + p * b) + ((i + f32(0.5)) * b) / f32(g)
            ok = (y >= -1) & (y <= L)
            y = np.clip(y[ok], 0, None)
            lo = np.minimum(y.astype(np.int64), L - 1)
            hi = np.minimum(lo + 1, L - 1)
            l = np.where(lo >= L - 1, 0, y - lo)
            n_axis.append(len(set(lo[l < 1].tolist()) | set(hi[l > 0].tolist())))
        tot += n_axis[0] * n_axis[1]
    return tot / float(len(rois))


def bench_ops(dev, rois_np, rounds, reps):
    g = torch.Generator().manual_seed(1)
    x = torch.randn((1, C, H, W), generator=g).to(dev)
    xh = ops.nchw_to_nhwc(x)
    rois = torch.from_numpy(rois_np).to(dev)
    dy = torch.randn((len(rois_np), C, PH, PW), generator=g).to(dev)
    _, am = O.RoIPoolF(x, rois, PH, PW, SCALE)
    legs = [('RoIPoolF fwd', lambda: O.RoIPoolF(x, rois, PH, PW, SCALE)),
            ('RoIPoolF bwd', lambda: O.RoIPoolFGradient(x, rois, am, dy))]
    for s in (0, 2):
        legs += [('RoIAlign s%d fwd' % s, lambda s=s: O.RoIAlign(x, rois, PH, PW, SCALE, s)),
                 ('RoIAlign s%d bwd' % s,
                  lambda s=s: O.RoIAlignGradient(x, rois, dy, PH, PW, SCALE, s)),
                 ('RoIAlign s%d fwd, entry alone (NHWC)' % s,
                  lambda s=s: ops.roi_align(xh, rois, PH, PW, SCALE, s, layout='NHWC')),
                 ('RoIAlign s%d bwd, entry alone (NHWC)' % s,
                  lambda s=s: ops.roi_align_grad(dy, rois, (1, H, W, C), SCALE, s, layout='NHWC'))]
    times = {name: [] for name, _ in legs}
    for rnd in range(rounds + 1):                       # round 0 warms every leg up
        for name, fn in legs:
            for _ in range(reps):
                t = event_ms(fn)
                if rnd:
                    times[name].append(t)
    med = {name: report(name, ts) for name, ts in times.items()}
    for s in (0, 2):
        px = weighted_pixels(rois_np, s)
        gb = len(rois_np) * px * C * 4 / 1e9
        ms = med['RoIAlign s%d bwd, entry alone (NHWC)' % s]
        zero = lambda: torch.zeros((1, H, W, C), device=dev)
        zero()                                           # (the first call pays for the allocation)
        fill = min(event_ms(zero) for _ in range(5))
        print('sampling %d: mean weighted pixels per roi %.1f -> %.2f GB of float atomic adds; '
              'entry %.3f ms (its zero-fill is about %.3f ms) = %.2f TB/s of added bytes'
              % (s, px, gb, ms, fill, gb / max(ms, 1e-9)), flush=True)


def bench_steps(dev, rois_mb, rounds, steps):
    blobs = synthetic.init_blobs(20, seed=3)
    t = {k: torch.from_numpy(v).to(dev) for k, v in rois_mb.items()}
    cases = []
    for frozen in (True, False):
        for method, s in (('RoIPoolF', 0), ('RoIAlign', 2), ('RoIAlign', 0)):
            cases.append(('%s body, %s%s' % ('frozen' if frozen else 'trainable', method,
                                             ' s%d' % s if method == 'RoIAlign' else ''),
                          frozen, method, s))
    times = {k[0]: [] for k in cases}
    for rnd in range(rounds + 1):
        for name, frozen, method, s in cases:
            c.reset_cfg()
            c.merge_cfg_from_file(YAML)
            c.merge_cfg_from_list(['NUM_GPUS', 1, 'TRAIN.FREEZE_CONV_BODY', frozen,
                                   'FAST_RCNN.ROI_XFORM_METHOD', method,
                                   'FAST_RCNN.ROI_XFORM_SAMPLING_RATIO', s])
            model = mbld.create('generalized_wsl', train=True)
            ex = NetExecutor(model, dev, force_interpreted=True)     # every leg op by op
            ex.load_blobs(dict(blobs))
            model.UpdateWorkspaceLr(0, 1e-5)
            for step in range(steps):
                ex.feed(t)
                ms = event_ms(ex.run)
                if rnd and step:
                    times[name].append(ms)
            del model, ex
            torch.cuda.empty_cache()
    c.reset_cfg()
    for name, ts in times.items():
        report(name + ' (ms/iter)', ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--skip-steps', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    mb = synthetic.make_minibatch(synthetic.make_roidb(1, 2000, 20, 600, 1000, seed=11), 20)
    bench_ops(dev, mb['rois'], args.rounds, args.reps)
    if not args.skip_steps:
        bench_steps(dev, mb, max(args.rounds - 2, 1), args.steps)


if __name__ == '__main__':
    main()
