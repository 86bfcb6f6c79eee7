"""The fc head of every arithmetic plan, bit for bit against the code as it was before the head
was written once over naws_hip.head_arith (tests/golden/head_plans_before.json).

record() uses only what the engine offered before that change (WsddnEngine, set_conv_blobs,
set_head_blobs, forward_backward, train_step, head_forward, state_tensors and the toggles
fuse_wgrad_update / fused_planes), so this file run as a script against a checkout of the parent,
`python tests/test_gpu_head_plans.py OUT.json`, writes the fixture.

Shapes: the tiny case of tests/test_gpu_engine.py (2 images of 64 x 96, 24 + 16 proposals, biases
non-zero).  Rt = 40 is no multiple of 16, 32 or 64: every transposing split pads K under every
plan.  C = 21 takes the padded ld8 route of fc8."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'head_plans_before.json')
PLANS = ('fp32', 'fp32x3', 'fp16x2', 'bf16')
CLASSES = (20, 21)
# train_step routes: as shipped (16-bit plans with a wgrad-epilogue update: fc6_w updated there);
# the deferred kernel alone; the element-wise kernel + re-split
ROUTES = {'fp32': ('shipped',), 'fp32x3': ('shipped',), 'bf16': ('shipped', 'deferred'),
          'fp16x2': ('shipped', 'deferred', 'unfused_planes')}
CASES = (['fb-%s-%d' % (p, c) for p in PLANS for c in CLASSES]
         + ['steps-%s-%d-%s' % (p, c, r) for p in PLANS for c in CLASSES for r in ROUTES[p]])
_INPUTS = {}


def _inputs(c):
    """(minibatch, blobs) of tests/test_gpu_engine.py::_setup, made once per class count."""
    if c not in _INPUTS:
        import torch
        from detectron.datasets import synthetic
        roidb = synthetic.make_roidb(2, 24, c, 64, 96, seed=11)
        for k in ('boxes', 'obn_scores', 'gt_classes'):
            roidb[1][k] = roidb[1][k][:16]
        mb = synthetic.make_minibatch(roidb, c)
        blobs = synthetic.init_blobs(c, seed=11)
        for k in list(blobs):
            if k.endswith('_b'):
                blobs[k] = torch.randn(blobs[k].shape, generator=torch.Generator().manual_seed(1)) * 0.05
        _INPUTS[c] = (mb, blobs)
    return _INPUTS[c]


def _engine(dev, plan, c):
    import torch
    from naws_hip.engine import WsddnEngine
    mb, blobs = _inputs(c)
    eng = WsddnEngine(c + 1, dev, dropout=0.5, gpu_num=2, seed=11, mfma_dtype=plan)
    eng.set_conv_blobs(blobs)
    eng.set_head_blobs(blobs)
    t = {k: torch.from_numpy(v).to(dev) for k, v in mb.items()}
    return eng, (t['data'], t['rois'], t['obn_scores'], t['labels_oh'])


def _digest(t):
    """SHA-256 of a tensor's bytes (any dtype, any strides)."""
    import torch
    return hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy()
                          .tobytes()).hexdigest()


def record(dev, case):
    import torch
    kind, plan, c = case.split('-')[:3]
    eng, args = _engine(dev, plan, int(c))
    out = {}
    if kind == 'fb':
        r = eng.forward_backward(*args)
        for k in ('loss_cls', 'loss_cls_noise'):
            out[k] = r[k].float().cpu().numpy().view(np.uint32).tolist()
        out['logits'], out['d_logits'] = _digest(r['logits'].float()), _digest(r['d_logits'].float())
        for name, _ in eng.arena.specs:
            out['grad_' + name] = _digest(eng.grad_blob(name))
        # a caller's own fp32 features: every plan's conversion of roi_feat
        x = torch.randn((args[1].shape[0], eng.k6), generator=torch.Generator().manual_seed(5)).to(dev)
        for tag, kw in (('train', dict(train=True)), ('test', dict(train=False, both_branches=False))):
            for k, v in zip(('h6', 'h7', 'logits'), eng.head_forward(x, **kw)):
                out['head_%s_%s' % (tag, k)] = _digest(v)
    else:
        route = case.split('-')[3]
        eng.set_lr(1e-3)
        if route in ('deferred', 'unfused_planes'):
            eng.fuse_wgrad_update = False
        if route == 'unfused_planes':
            eng.fused_planes = False
        for _ in range(2):
            eng.train_step(*args)
        for k, v in sorted(eng.state_tensors().items()):
            out[k] = _digest(v)
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_head_is_bit_identical_to_parent(dev, case):
    """forward_backward (losses, logits, d_logits, all 16 gradient blobs), head_forward on a
    caller's fp32 features (train / test), and the state after two train_step calls on every
    update route of one process: identical, bit for bit, to what the parent of this change
    computed."""
    want = json.load(open(FIXTURE))[case]
    got = record(dev, case)
    assert sorted(got) == sorted(want)
    diff = [k for k in sorted(want) if got[k] != want[k]]
    assert not diff, (case, diff)


if __name__ == '__main__':
    for p in (ROOT, os.path.join(ROOT, 'na-fwebsod_amd')):
        sys.path.insert(0, p)
    import torch
    rec = {case: record(torch.device('cuda:0'), case) for case in CASES}
    with open(sys.argv[1], 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
