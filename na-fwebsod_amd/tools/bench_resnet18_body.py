#!/usr/bin/env python3
"""What the ResNet18-WS body (MODEL.CONV_BODY ResNet18.add_ResNet18_conv5_body) costs next to the
VGG-16 origin body on the op-by-op plan at the bench shape (one 600 x 1000 image, 2000 proposals):
the conv body alone and one whole plain-WSDDN training iteration (WEBLY.WEBLY_ON False, frozen body,
a 4096-wide 2-fc head on both), the two models interleaved in one process and timed with device
events (the method of tools/bench_deeplab_body.py).  Both bodies run op by op here - the VGG-16
body's fused plan is not what is compared -, so every layer pays its NCHW <-> NHWC transposes and
its weight packing on both sides.

    python tools/bench_resnet18_body.py [--rounds 7] [--iters 5] [--res5-dilation 2]
"""
import argparse
import os
import sys

import torch

PKG = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, PKG)
from detectron.core import config as c  # noqa: E402
from detectron.datasets import synthetic  # noqa: E402

YAML = os.path.join(PKG, 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
NFG = 20
BODIES = {
    'VGG-16 origin': ['MODEL.CONV_BODY', 'VGG16.add_VGG16_conv5_body_origin',
                      'FAST_RCNN.ROI_BOX_HEAD', 'wsl_heads.add_VGG16_roi_2fc_head'],
    'ResNet18 conv5': ['MODEL.CONV_BODY', 'ResNet18.add_ResNet18_conv5_body',
                       'RESNETS.TRANS_FUNC', 'residual_transformation',
                       'FAST_RCNN.ROI_BOX_HEAD', 'wsl_heads.add_ResNet_roi_2fc_head',
                       'FAST_RCNN.MLP_HEAD_DIM', 4096],
}


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
    print('%-52s median %.3f ms (min %.3f max %.3f)' % (name, ts[len(ts) // 2], ts[0], ts[-1]))
    return ts[len(ts) // 2]


def build(dev, extra, feed):
    """(model, executor, number of body ops) under the cfg of one body; one step has run, so every
    per-op object exists before the cfg moves on to the next body."""
    from detectron.core.executor import NetExecutor
    import detectron.modeling.model_builder_wsl as mbld
    c.reset_cfg()
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', 1, 'WEBLY.WEBLY_ON', False, 'TRAIN.FREEZE_CONV_BODY', True,
                           'MODEL.NUM_CLASSES', NFG + 1] + extra)
    c.assert_and_infer_cfg(make_immutable=False)
    model = mbld.create('generalized_wsl', train=True)
    ex = NetExecutor(model, dev, force_interpreted=True)
    ex.init_params(seed=11)
    first = [n for n in model.params if n.endswith('_w')][0]
    ex.ws[first].mul_(1.0 / 64.0)            # +-128 pixels in, O(1) activations through the stack
    n_body = [i for i, op in enumerate(model.net.ops) if op.type.startswith('RoI')][0]
    model.UpdateWorkspaceLr(0, 1e-5)
    ex.feed(feed)
    ex.run()
    torch.cuda.synchronize()
    return model, ex, n_body


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--rois', type=int, default=2000)
    ap.add_argument('--res5-dilation', type=int, default=2)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    mb = synthetic.make_minibatch(synthetic.make_roidb(1, a.rois, NFG, 600, 1000, seed=11), NFG)
    feed = {k: torch.from_numpy(v).to(dev) for k, v in mb.items()}
    nets = {}
    for name, extra in BODIES.items():
        if name.startswith('ResNet'):
            extra = extra + ['RESNETS.RES5_DILATION', a.res5_dilation]
        model, ex, n_body = build(dev, extra, feed)
        out = model.net.ops[n_body - 1].outputs[0]
        print('%s: %d body ops, %s %s, loss_cls %.4f' % (
            name, n_body, out, tuple(ex.ws[out].shape), float(ex.ws['loss_cls'].reshape(-1)[0])))
        nets[name] = (model, ex, n_body)

    def body(net):
        model, ex, n_body = net
        for idx, op in enumerate(model.net.ops[:n_body]):
            ex._forward(idx, op, ex.ws)

    runs = {'conv body': body, 'training iteration': lambda net: net[1].run()}
    for what, fn in runs.items():
        times = {n: [] for n in nets}
        for r in range(a.rounds + 1):
            for name, net in nets.items():                # interleaved: drift hits both alike
                ms = timed(lambda: fn(net), a.iters)
                if r > 0:
                    times[name].append(ms)
        med = {n: report('%s, %s (op by op)' % (what, n), ts) for n, ts in times.items()}
        print('%s: ResNet18 / VGG-16 = %.3f' % (what, med['ResNet18 conv5'] / med['VGG-16 origin']))


if __name__ == '__main__':
    main()
