#!/usr/bin/env python3
"""The C-ABI launch trace of the op-by-op plan of THIS tree: every `naws_hip.lib.call` of two
training iterations of the tiny model (one 3 x 48 x 64 image, 12 rois, 20 classes; dropout on, a
fixed RNG_SEED) for seven builds - the entry's name and every argument that is not a pointer (ints
and the u64 seed exactly, floats by repr), a pointer only as null / not null.  Run on an MI355X on
the commit before the operator table existed, its output (opbyop_call_trace_before.json) pins
that the table-driven executor launches the same kernels in the same order at the same shapes and
scalars (tests/test_gpu_op_table.py).

    PYTHONPATH=na-fwebsod_amd python tests/golden/make_golden_opbyop_call_trace.py [output.json]
"""
import json
import os
import sys

from make_golden_op_signatures import BUILDS as _B, create

HERE = os.path.dirname(os.path.abspath(__file__))
NFG, SEED = 20, 3
# build name -> (build of make_golden_op_signatures, conv body frozen, further cfg keys)
BUILDS = {
    'na_wsddn': ('na_wsddn', True, []),
    'center_loss': ('center_loss', True, ['NAWS.CENTER_LOSS_TOP_K', 4]),
    'trainable_body': ('na_wsddn', False, []),
    'roi_align_trainable': ('roi_align', False, []),
    'wsddn_context_oicr': ('wsddn_context_oicr', True, []),
    'min_entropy': ('min_entropy', True, []),
    'conv4': ('conv4', True, []),
}
assert all(b in _B for b, _f, _e in BUILDS.values())


def _plain(name, args):
    from naws_hip import lib as L
    row = [name]
    for kind, v in zip(L.PROTOTYPES[name], args):
        v = getattr(v, 'value', v)
        if kind is L.p:
            row.append(bool(v))                          # not null
        elif kind is L.f32:
            row.append(repr(float(v)))
        else:
            row.append(int(v))
    return row


def trace(dev, name):
    """(calls, losses): the recorded calls of two NetExecutor.run() iterations of one build and the
    loss blobs fetched after each."""
    import torch
    from detectron.core import config as c
    from detectron.core.executor import NetExecutor
    from detectron.datasets import synthetic
    from naws_hip import lib as L
    build, frozen, extra = BUILDS[name]
    calls, losses = [], []
    real = L.call

    def recording(entry, *args):
        calls.append(_plain(entry, args))
        return real(entry, *args)
    try:
        model = create(build, True, frozen, num_gpus=1, extra=['RNG_SEED', SEED] + extra)
        ex = NetExecutor(model, dev, force_interpreted=True, disable_dropout=False)
        assert ex.plan == 'interpreted'
        ex.init_params(seed=7)
        model.UpdateWorkspaceLr(0, 1e-3)
        mb = synthetic.make_minibatch(synthetic.make_roidb(1, 12, NFG, 48, 64, seed=5), NFG)
        feed = {k: torch.from_numpy(v).to(dev) for k, v in mb.items()}
        torch.cuda.synchronize()
        L.call = recording
        for _it in range(2):
            ex.feed(feed)
            ex.run()
            L.call = real
            losses.append({l: float(ex.fetch(l).reshape(-1)[0].item()) for l in model.losses})
            L.call = recording
    finally:
        L.call = real
        c.reset_cfg()
    return calls, losses


if __name__ == '__main__':
    import torch
    out = {}
    for name in sorted(BUILDS):
        out[name], losses = trace(torch.device('cuda:0'), name)
        print(name, len(out[name]), 'calls; losses', losses, flush=True)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, 'opbyop_call_trace_before.json')
    with open(path, 'w') as f:
        json.dump(out, f, separators=(',', ':'))
