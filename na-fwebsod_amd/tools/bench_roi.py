#!/usr/bin/env python3
"""Interleaved in-process timing of the RoIPoolF operand-plane kernels on the bench shape
(2 images 74x124x512, 2 x 2000 proposals): direct vs hierarchical, waves per (roi, slice); and
RoILoopPool (WSL.CONTEXT) on the frame / context rois of the same proposals (75x125 map, both
layouts) beside RoIPoolF on their outer rectangles (`--loop-pool` runs that part alone)."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from detectron.datasets import synthetic  # noqa: E402
from naws_hip import lib as L, ops  # noqa: E402


def _ms(fn, reps=12):
    """Per-call event times of fn (first call dropped)."""
    ts = []
    for r in range(reps + 1):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        torch.cuda.synchronize()
        if r:
            ts.append(s.elapsed_time(e))
        del out
    return ts


def loop_pool_rows(dev):
    """naws_roi_loop_pool_fwd vs naws_roi_pool_f_fwd (no argmax) on the same outer rectangles,
    interleaved round by round: the loop pool reads a subset of that window and writes the same
    bytes.  Prints median, min and the spread (max - min) / median of each, and the ratio."""
    mb = synthetic.make_minibatch(synthetic.make_roidb(2, 2000, 20, 600, 1000, seed=11), 20)
    rois = torch.from_numpy(mb['rois']).to(dev)
    boost = torch.from_numpy(mb['obn_scores'].reshape(-1)).to(dev)
    frame, context = ops.roi_context(rois, 600, 1000, 1.8)
    x = {'NHWC': torch.randn((2, 75, 125, 512), device=dev).relu_()}
    x['NCHW'] = x['NHWC'].permute(0, 3, 1, 2).contiguous()
    for layout in ('NHWC', 'NCHW'):
        for name, r9 in (('frame', frame), ('context', context)):
            outer = r9[:, :5].contiguous()
            a = ops.roi_loop_pool(x[layout], r9, 7, 7, 0.125, boost=boost, layout=layout)
            b = ops.roi_pool_f(x[layout], outer, 7, 7, 0.125, boost=boost, layout=layout)
            share = float((a != b).float().mean())
            assert bool((a <= b).all())          # non-negative features: a subset of the window
            tl, tp = [], []
            for _round in range(4):
                tl += _ms(lambda: ops.roi_loop_pool(x[layout], r9, 7, 7, 0.125, boost=boost,
                                                    layout=layout), 6)
                tp += _ms(lambda: ops.roi_pool_f(x[layout], outer, 7, 7, 0.125, boost=boost,
                                                 layout=layout), 6)
            tl, tp = sorted(tl), sorted(tp)
            ml, mp = tl[len(tl) // 2], tp[len(tp) // 2]
            print('%s %-7s loop pool median %.3f ms (min %.3f, spread %.1f%%) | RoIPoolF on the '
                  'outer rectangles median %.3f ms (min %.3f, spread %.1f%%) | ratio %.2f | bins '
                  'that differ %.1f%%' % (layout, name, ml, tl[0], 100 * (tl[-1] - tl[0]) / ml, mp,
                                          tp[0], 100 * (tp[-1] - tp[0]) / mp, ml / mp,
                                          100 * share), flush=True)


def main():
    dev = torch.device('cuda:0')
    if '--loop-pool' in sys.argv[1:]:
        return loop_pool_rows(dev)
    mb = synthetic.make_minibatch(synthetic.make_roidb(2, 2000, 20, 600, 1000, seed=11), 20)
    rois = torch.from_numpy(mb['rois']).to(dev)
    boost = torch.from_numpy(mb['obn_scores'].reshape(-1)).to(dev)
    x = torch.randn((2, 74, 124, 512), device=dev).relu_()
    amax = ops.amax_word(x).repeat(2)
    variants = [('direct', dict(hier=False), None)] + [
        ("hier nw*10+rg=%d" % nw, dict(hier=True), str(nw)) for nw in (42,)]
    times = {v[0]: [] for v in variants}
    ref = None
    for r in range(8):
        for name, kw, nw in variants:
            if nw is not None:
                L.set_variant('roi_nw', int(nw))
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = ops.roi_pool_f_f16x2(x, rois, amax, 7, 7, 0.125, boost=boost, **kw)
            e.record()
            torch.cuda.synchronize()
            if r == 0:
                if ref is None:
                    ref = out.planes.clone()
                assert torch.equal(out.planes.view(torch.int16), ref.view(torch.int16)), name
            else:
                times[name].append(s.elapsed_time(e))
            del out
    for name, kw in (('fp32 direct', dict(hier=False)), ('fp32 hier', dict(hier=True))):
        ts = []
        for r in range(8):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            out = ops.roi_pool_f(x, rois, 7, 7, 0.125, boost=boost, layout='NHWC', **kw)
            e.record()
            torch.cuda.synchronize()
            if r:
                ts.append(s.elapsed_time(e))
            del out
        times[name] = ts
    ws = torch.empty((2 * x.numel(),), device=dev)
    ts = []
    for r in range(8):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        # maps only: the hier entry with R = 0 rois is a no-op, so time the map build through a
        # 1-roi call
        out = ops.roi_pool_f(x, rois[:1], 7, 7, 0.125, boost=boost[:1], layout='NHWC', hier=True)
        e.record()
        torch.cuda.synchronize()
        if r:
            ts.append(s.elapsed_time(e))
    times['maps + 1 roi'] = ts
    for name, ts in times.items():
        ts = sorted(ts)
        print('%-20s median %.3f ms (min %.3f)' % (name, ts[len(ts) // 2], ts[0]))
    loop_pool_rows(dev)


if __name__ == '__main__':
    main()
