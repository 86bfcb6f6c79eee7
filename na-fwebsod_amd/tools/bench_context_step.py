#!/usr/bin/env python3
"""ms per training iteration of the op-by-op plan on the plain WSDDN model (WEBLY.WEBLY_ON False)
at the bench shape (one 600 x 1000 image, 2000 proposals), with and without WSL.CONTEXT and with
and without the FC input gradients nobody reads (dX = dY W behind StopGradient, which
AddGradientOperators no longer emits: `keep dead dX` puts them back).  The four cases are
interleaved round by round in one process; device-event times per iteration."""
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

YAML = os.path.join(ROOT, 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')


def build(dev, context, keep_dead_dx, blobs):
    c.reset_cfg()
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', 1, 'WEBLY.WEBLY_ON', False, 'WSL.CONTEXT', context,
                           'FAST_RCNN.ROI_BOX_HEAD', 'wsl_heads.add_VGG16_roi_2fc_head'])
    model = mbld.create('generalized_wsl', train=True)
    if keep_dead_dx:
        for o in model.grad_ops:
            if o.type == 'FCGradient' and o.args['_gin'][0] is None:
                o.args['_gin'][0] = o.inputs[0] + '_grad'
    ex = NetExecutor(model, dev)
    assert ex.plan == 'interpreted'
    b = dict(blobs)
    if context:
        b['fc8d_frame_w'], b['fc8d_frame_b'] = b['fc8d_w'], b['fc8d_b']
    ex.load_blobs(b)
    model.UpdateWorkspaceLr(0, 1e-5)
    return model, ex


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=4)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    blobs = synthetic.init_blobs(20, seed=3)
    mb = synthetic.make_minibatch(synthetic.make_roidb(1, 2000, 20, 600, 1000, seed=11), 20)
    t = {k: torch.from_numpy(v).to(dev) for k, v in mb.items()}
    cases = [('plain', False, False), ('plain, keep dead dX', False, True),
             ('context', True, False), ('context, keep dead dX', True, True)]
    times = {name: [] for name, _c, _k in cases}
    for rnd in range(args.rounds + 1):                   # round 0 warms every shape up
        for name, context, keep in cases:
            model, ex = build(dev, context, keep, blobs)   # (cfg is read while the graph runs)
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


if __name__ == '__main__':
    main()
