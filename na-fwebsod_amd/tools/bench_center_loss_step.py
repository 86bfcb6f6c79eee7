#!/usr/bin/env python3
"""ms per na_wsddn training iteration on the op-by-op plan (one 600 x 1000 image, 2000 proposals)
with WSL.CENTER_LOSS off and on, interleaved round by round in one process; and, in the same
process, the op pair alone against a torch restatement shaped like the reference's CUDA operator
(detectron/ops/center_loss_op.cu): the score matrix copied to the host, the top-k picked there,
and one .item() per (class, centre) distance - the thing the device-resident kernels replace.
Device-event times for the iterations, wall-clock (synchronised) times for the op pair, since the
restatement's cost IS its host synchronisation."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
from detectron.core import config as c  # noqa: E402
from detectron.core.executor import NetExecutor  # noqa: E402
from detectron.datasets import synthetic  # noqa: E402
import detectron.modeling.model_builder_wsl as mbld  # noqa: E402
from naws_hip import ops  # noqa: E402

YAML = os.path.join(ROOT, 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')


def build(dev, on, blobs):
    c.reset_cfg()
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', 1, 'WSL.CENTER_LOSS', on])
    model = mbld.create('generalized_wsl', train=True)
    ex = NetExecutor(model, dev, force_interpreted=True)
    assert ex.plan == 'interpreted'
    ex.load_blobs(blobs)
    model.UpdateWorkspaceLr(0, 1e-5)
    return model, ex


def reference_shaped(x, p, f, cf, dl, top_k):
    """Forward + feature gradient the way the reference schedules them (host top-k, a blocking
    read per distance)."""
    xh, ph = x.cpu(), p.cpu()                      # two blocking copies (:102-108)
    n, d = f.shape
    chosen, loss = [], 0.0
    for cls in range(cf.shape[0]):
        if xh[cls] < 0.5 or n < top_k:
            continue
        rows = torch.sort(torch.topk(ph[:, cls], top_k).indices).values.to(f.device)
        best, best_m, best_d = float('inf'), -1, None
        for m in range(cf.shape[1]):
            diff = f[rows] - cf[cls, m]
            dot = float((diff * diff).sum().item())          # one blocking read per dot (:201-207)
            if dot < best:
                best, best_m, best_d = dot, m, diff
        chosen.append((rows, best_d))
        loss += best
    df = torch.zeros_like(f)
    alpha = float(dl.item()) / max(len(chosen), 1) / top_k / d   # (:498-504)
    for rows, diff in chosen:
        df[rows] += alpha * diff
    return loss, df


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=4)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    blobs = synthetic.init_blobs(20, seed=3)
    g = torch.Generator().manual_seed(17)
    blobs['center_feature'] = torch.randn((20, 5, 4096), generator=g)
    blobs['center_feature_g'] = torch.zeros((20, 5, 4096))
    blobs['center_feature_n_u'] = torch.zeros((20, 5))
    mb = synthetic.make_minibatch(synthetic.make_roidb(1, 2000, 20, 600, 1000, seed=11), 20)
    t = {k: torch.from_numpy(v).to(dev) for k, v in mb.items()}
    cases = [('center loss off', False), ('center loss on', True)]
    times = {name: [] for name, _on in cases}
    for rnd in range(args.rounds + 1):                   # round 0 warms every shape up
        for name, on in cases:
            model, ex = build(dev, on, blobs)
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
        print('%-18s median %.2f ms/iter (min %.2f, max %.2f, n = %d)' % (
            name, ts[len(ts) // 2], ts[0], ts[-1], len(ts)), flush=True)
    # ---- the op pair alone, half of the 20 classes labelled
    n, cdim, m, top_k, d = 2000, 20, 5, 10, 4096
    x = (torch.arange(cdim, device=dev) % 2 == 0).float()
    p = torch.rand((n, cdim), device=dev)
    f, cf = torch.randn((n, d), device=dev), torch.randn((cdim, m, d), device=dev)
    dcf, ndcf = torch.zeros_like(cf), torch.zeros((cdim, m), device=dev)
    acc_d, acc_n = torch.zeros_like(dcf), torch.zeros_like(ndcf)
    ws = ops.center_loss_workspace(cdim, m, top_k, dev)
    dl = torch.full((1,), 0.4096, device=dev)

    def ours():
        _l, dd, ss, _w = ops.center_loss(x, p, f, cf, top_k, workspace=ws)
        ops.center_loss_update(cf, dcf, ndcf, acc_d, acc_n, top_k, 0.5)
        return ops.center_loss_grad(dd, ss, dl, n, ws, dcf, ndcf)

    wall = {'HIP op pair': [], 'reference-shaped torch': []}
    for rnd in range(args.rounds * 3 + 1):
        for name, fn in (('HIP op pair', ours),
                         ('reference-shaped torch', lambda: reference_shaped(x, p, f, cf, dl, top_k))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                wall[name].append((time.perf_counter() - t0) * 1e3)
    for name, ts in wall.items():
        ts = sorted(ts)
        print('%-24s median %.3f ms wall (min %.3f, max %.3f, n = %d)' % (
            name, ts[len(ts) // 2], ts[0], ts[-1], len(ts)), flush=True)


if __name__ == '__main__':
    main()
