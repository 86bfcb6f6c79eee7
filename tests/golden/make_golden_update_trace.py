#!/usr/bin/env python3
"""The launch-and-sync trace of the engine's update schedule on THIS tree: per scenario, every
C-ABI call with the ordinal of its stream, every event recorded and waited for, and every call of
the gradient exchange (tests/update_trace_rec.py), over a few iterations of the tiny model of
tests/test_gpu_engine.py (two 3 x 64 x 96 images with 24 / 16 proposals, 20 classes, dropout 0.5,
seed 11) that end with flush(); then the SHA-256 of every tensor of state_tensors().  Only API that
exists on both sides of a change to the schedule is used, so the same file runs on the commit
before it - whose output, update_trace_before.json, pins when, where, on which stream and behind
which events every route launches (tests/test_gpu_update_trace.py).

    PYTHONPATH=na-fwebsod_amd python tests/golden/make_golden_update_trace.py [output.json]
"""
import functools
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
try:
    from update_trace_rec import Recorder, pack
finally:
    sys.path.pop(0)

C, SEED = 20, 11
# scenario -> the engine's constructor arguments and:  step 'train' = train_step, 'split' =
# forward_backward + sgd_step;  exchange = (ranks, chunks): an EmulatedExchange in the reducer's
# place;  iters (3);  images (2);  set = engine toggles;  route = {iteration: set_update_route
# arguments before it};  touch = the iteration after which blob('fc7_w') is written through
SCENARIOS = {
    'a_train_step': dict(step='train'),
    'b_deferred': dict(step='split'),
    'c_inline': dict(step='split', set=dict(defer_update=False)),
    'd_unfused_planes': dict(step='split', set=dict(fused_planes=False)),
    'e_dirty_planes': dict(step='split', touch=0),
    'f_fp32': dict(step='train', ctor=dict(mfma_dtype='fp32')),
    'f_fp32x3': dict(step='train', ctor=dict(mfma_dtype='fp32x3')),
    'f_bf16': dict(step='train', ctor=dict(mfma_dtype='bf16')),
    'g_iter_size_2': dict(step='split', ctor=dict(iter_size=2), iters=4),
    'h_pipelined_eager': dict(step='train', exchange=(2, 4)),
    'i_pipelined_after': dict(step='split', exchange=(2, 4)),
    'j_unpipelined': dict(step='train', exchange=(4, 2), ctor=dict(pipeline_update=False)),
    'k_sharded_then_default': dict(step='train', exchange=(4, 2),
                                   route={0: dict(sharded_update=True), 2: dict()}),
    'l_one_image': dict(step='split', images=1),
}


@functools.lru_cache(maxsize=None)
def _inputs(images):
    """(minibatch, blobs, seg) of tests/test_gpu_engine.py::_setup (its first `images` images)."""
    import numpy as np
    import torch
    from detectron.datasets import synthetic
    roidb = synthetic.make_roidb(2, 24, C, 64, 96, seed=SEED)
    for k in ('boxes', 'obn_scores', 'gt_classes'):
        roidb[1][k] = roidb[1][k][:16]
    mb = synthetic.make_minibatch(roidb[:images], C)
    blobs = synthetic.init_blobs(C, seed=SEED)
    for k in list(blobs):     # non-zero biases so the bias paths are exercised
        if k.endswith('_b'):
            blobs[k] = torch.randn(blobs[k].shape, generator=torch.Generator().manual_seed(1)) * 0.05
    seg = [0] + np.cumsum(np.bincount(mb['rois'][:, 0].astype(np.int64), minlength=images)).tolist()
    return mb, blobs, seg


def _sha256(t):
    import torch
    v = t.detach().contiguous().view(-1)
    v = v.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[v.element_size()])
    h = hashlib.sha256()
    for o in range(0, v.numel(), 1 << 26):
        h.update(v[o:o + (1 << 26)].cpu().numpy().tobytes())
    return h.hexdigest()


def run(dev, name):
    """(rows, digests): the recorded schedule of scenario `name` and {tensor: SHA-256} of the
    engine's state after its last flush()."""
    import torch
    from naws_hip.engine import WsddnEngine
    from naws_hip.reducer import EmulatedExchange
    sc = SCENARIOS[name]
    images = sc.get('images', 2)
    mb, blobs, seg = _inputs(images)
    t = {k: torch.from_numpy(v).to(dev) for k, v in mb.items()}
    args = (t['data'], t['rois'], t['obn_scores'], t['labels_oh'])
    eng = WsddnEngine(C + 1, dev, dropout=0.5, gpu_num=2, seed=SEED,
                      **dict(dict(mfma_dtype='fp16x2'), **sc.get('ctor', {})))
    eng.set_conv_blobs(blobs)
    eng.set_head_blobs(blobs)
    eng.set_lr(1e-3)
    for k, v in sc.get('set', {}).items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    if 'exchange' in sc:
        eng.reducer = EmulatedExchange(dev, sc['exchange'][0])
        eng.allreduce_chunks = sc['exchange'][1]
    torch.cuda.synchronize()
    iters = sc.get('iters', 3)
    with Recorder() as rec:
        rec.watch(eng.reducer)
        for it in range(iters):
            if it in sc.get('route', {}):
                eng.set_update_route(**sc['route'][it])
            if it == iters - 1:
                eng.set_lr(5e-4)              # (a pending update is joined; the momentum is scaled)
            if sc['step'] == 'train':
                eng.train_step(*args, seg=seg)
            else:
                eng.forward_backward(*args, seg=seg)
                eng.sgd_step()
            if it == sc.get('touch'):
                eng.blob('fc7_w').mul_(0.5)   # planes dirty: the next update takes the exact route
        eng.flush()
    torch.cuda.synchronize()
    digests = {k: _sha256(v) for k, v in sorted(eng.state_tensors().items())}
    return rec.rows, digests


if __name__ == '__main__':
    import torch
    out = {}
    for name in sorted(SCENARIOS):
        rows, digests = run(torch.device('cuda:0'), name)
        out[name] = dict(trace=rows, digests=digests)
        print(name, len(rows), 'rows;', len(digests), 'tensors', flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'update_trace_before.json')
    with open(path, 'w') as f:      # (update_trace_rec.pack: each distinct row once + indices)
        json.dump(pack(out), f, separators=(',', ':'), sort_keys=True)
