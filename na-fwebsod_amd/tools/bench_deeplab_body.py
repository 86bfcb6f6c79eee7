#!/usr/bin/env python3
"""What the DeepLab VGG-16 body (MODEL.CONV_BODY VGG16.add_VGG16_conv5_body_deeplab) costs next to
the origin body at the bench shape (600 x 1000 images, 2000 proposals each): the conv body alone and
one whole na_wsddn training step, the two bodies interleaved in one process and timed with device
events (the method of tools/ab_convbody.py), and the 3x3 pool kernel alone at two of its layer
shapes with the fraction of the HBM peak its compulsory traffic (input read once + output written
once) reaches.

    python tools/bench_deeplab_body.py [--rounds 7] [--iters 10] [--images 2]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from detectron.datasets import synthetic  # noqa: E402
from naws_hip import ops  # noqa: E402
from naws_hip.engine import WsddnEngine  # noqa: E402

HBM_PEAK = 8.0e12            # bytes / s, MI355X


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def report(name, ts):
    ts = sorted(ts)
    print('%-44s median %.3f ms (min %.3f max %.3f)' % (name, ts[len(ts) // 2], ts[0], ts[-1]))
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--images', type=int, default=2)
    ap.add_argument('--rois', type=int, default=2000)
    ap.add_argument('--mfma-dtype', default='fp16x2')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    c = 20
    blobs = synthetic.init_blobs(c, seed=11)
    mb = synthetic.make_minibatch(synthetic.make_roidb(a.images, a.rois, c, 600, 1000, seed=11), c)
    t = {k: torch.from_numpy(v).to(dev) for k, v in mb.items()}
    engines = {}
    for body in ('origin', 'deeplab'):
        eng = WsddnEngine(c + 1, dev, gpu_num=a.images, seed=11, mfma_dtype=a.mfma_dtype, body=body)
        eng.set_conv_blobs(blobs)
        eng.set_head_blobs(blobs)
        eng.set_lr(1e-5)
        engines[body] = eng
        print('%s: conv5_3 %s' % (body, tuple(eng.conv_body(t['data']).shape)))
    runs = {
        'conv body': lambda e: e.conv_body(t['data']),
        'training step': lambda e: e.train_step(t['data'], t['rois'], t['obn_scores'], t['labels_oh']),
    }
    for what, fn in runs.items():
        times = {b: [] for b in engines}
        for r in range(a.rounds + 1):
            for body, eng in engines.items():             # interleaved: drift hits both alike
                ms = timed(lambda: fn(eng), a.iters)
                if r > 0:
                    times[body].append(ms)
        for eng in engines.values():
            eng.flush()
        med = {b: report('%s, %s body (%d images)' % (what, b, a.images), ts)
               for b, ts in times.items()}
        print('%s: deeplab / origin = %.3f' % (what, med['deeplab'] / med['origin']))
    # the pool alone
    for (h, w, ch), stride in (((600, 1000, 64), 2), ((75, 125, 512), 1)):
        x = torch.randn((1, h, w, ch), device=dev)
        y = ops.maxpool3x3_nhwc(x, stride)
        ts = [timed(lambda: ops.maxpool3x3_nhwc(x, stride, out=y), 50) for _ in range(a.rounds)]
        med = report('maxpool3x3 %d x %d x %d stride %d' % (h, w, ch, stride), ts)
        nbytes = 4 * (x.numel() + y.numel())
        print('   %.1f MB compulsory traffic: %.2f TB/s = %.1f %% of the %.1f TB/s HBM peak'
              % (nbytes / 1e6, nbytes / med / 1e9, 100 * nbytes / (med * 1e-3) / HBM_PEAK,
                 HBM_PEAK / 1e12))
        if stride == 2:
            x2 = x[:, :, :, :]
            y2 = ops.maxpool2x2_nhwc(x2, 2)
            ts = [timed(lambda: ops.maxpool2x2_nhwc(x2, 2, out=y2), 50) for _ in range(a.rounds)]
            report('   (maxpool2x2 of the same map, stride 2)', ts)


if __name__ == '__main__':
    main()
