#!/usr/bin/env python3
"""ms per training iteration of na_wsddn on the op-by-op plan at the bench shape (one 600 x 1000
image, 2000 proposals) with the conv body frozen (TRAIN.FREEZE_CONV_BODY True, the shipped yamls)
and trainable (False: conv3_1..conv5_3 and RoIPoolF get a backward), the two cases interleaved
round by round in one process, device-event times per iteration; then device-event times of the
new C-ABI entries on their own at the shapes of that iteration."""
import argparse
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from detectron.core import config as c  # noqa: E402
from detectron.core.executor import NetExecutor  # noqa: E402
from detectron.datasets import synthetic  # noqa: E402
import detectron.modeling.model_builder_wsl as mbld  # noqa: E402
from naws_hip import ops  # noqa: E402

YAML = os.path.join(ROOT, 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')


def build(dev, frozen, blobs):
    c.reset_cfg()
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', 1, 'TRAIN.FREEZE_CONV_BODY', frozen])
    model = mbld.create('generalized_wsl', train=True)
    ex = NetExecutor(model, dev, force_interpreted=True)
    assert ex.plan == 'interpreted'
    ex.load_blobs(dict(blobs))
    model.UpdateWorkspaceLr(0, 1e-5)
    return model, ex


def timed(fn, reps):
    fn()                                                   # warm-up (first launch, allocator)
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def per_op(dev, reps):
    """The new entries alone, NHWC, at the layer shapes of a 600 x 1000 image (dilation 2 body)."""
    g = torch.Generator().manual_seed(1)

    def rnd(*shape):
        return torch.randn(shape, generator=g).to(dev)

    rows = []
    layers = [('conv3_x wgrad', 150, 250, 256, 256, 1), ('conv4_1 wgrad', 75, 125, 256, 512, 1),
              ('conv4_x wgrad', 75, 125, 512, 512, 1), ('conv5_x wgrad', 74, 124, 512, 512, 2)]
    for name, h, w, ci, co, d in layers:
        x, dy = rnd(1, h, w, ci), rnd(1, h, w, co)
        n = ops.L.load().naws_conv3x3_nhwc_wgrad_workspace_floats(1, h, w, ci, co, d)
        ws = torch.empty((n,), device=dev)
        rows.append((name + ' (%dx%d, %d->%d, d%d)' % (h, w, ci, co, d),
                     timed(lambda: ops.conv3x3_nhwc_wgrad(x, dy, d, workspace=ws), reps)))
        wt = rnd(co, ci, 3, 3)
        wp = ops.conv3x3_dgrad_pack_weight(wt)
        rows.append((name.replace('wgrad', 'dgrad pack'),
                     timed(lambda: ops.conv3x3_dgrad_pack_weight(wt), reps)))
        rows.append((name.replace('wgrad', 'dgrad conv'),
                     timed(lambda: ops.conv3x3_nhwc(dy, wp, None, d, relu=False), reps)))
    for name, h, w, ch, s in (('pool3 bwd', 150, 250, 256, 2), ('pool4 bwd', 75, 125, 512, 1)):
        x = rnd(1, h, w, ch)
        y = ops.maxpool2x2_nhwc(x, s)
        dy = torch.randn(y.shape, generator=g).to(dev)
        rows.append((name + ' (%dx%d, C %d, stride %d)' % (h, w, ch, s),
                     timed(lambda: ops.maxpool2x2_nhwc_grad(x, y, dy, s), reps)))
    mb = synthetic.make_minibatch(synthetic.make_roidb(1, 2000, 20, 600, 1000, seed=11), 20)
    rois = torch.from_numpy(mb['rois']).to(dev)
    feat = rnd(1, 512, 74, 124)
    y, am = ops.roi_pool_f(feat, rois, 7, 7, 0.125, layout='NCHW', with_argmax=True)
    dy = torch.randn(y.shape, generator=g).to(dev)
    rows.append(('RoIPoolF bwd (2000 rois, 512 x 74 x 124, NCHW)',
                 timed(lambda: ops.roi_pool_f_grad(dy, am, rois, tuple(feat.shape)), reps)))
    for name, (med, lo, hi) in rows:
        print('%-52s median %8.3f ms (min %.3f, max %.3f)' % (name, med, lo, hi), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--op-reps', type=int, default=10)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    blobs = synthetic.init_blobs(20, seed=3)
    mb = synthetic.make_minibatch(synthetic.make_roidb(1, 2000, 20, 600, 1000, seed=11), 20)
    t = {k: torch.from_numpy(v).to(dev) for k, v in mb.items()}
    cases = [('frozen body', True), ('trainable body', False)]
    times = {name: [] for name, _f in cases}
    for rnd in range(args.rounds + 1):                   # round 0 warms every shape up
        for name, frozen in cases:
            model, ex = build(dev, frozen, blobs)          # (cfg is read while the graph runs)
            for _step in range(args.steps):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ex.feed(t)
                s.record()
                ex.run()
                e.record()
                torch.cuda.synchronize()
                if rnd and _step:
                    times[name].append(s.elapsed_time(e))
            del model, ex
            torch.cuda.empty_cache()
    c.reset_cfg()
    for name, ts in times.items():
        ts = sorted(ts)
        print('%-24s median %.2f ms/iter (min %.2f, max %.2f, n = %d)' % (
            name, ts[len(ts) // 2], ts[0], ts[-1], len(ts)), flush=True)
    per_op(dev, args.op_reps)


if __name__ == '__main__':
    main()
