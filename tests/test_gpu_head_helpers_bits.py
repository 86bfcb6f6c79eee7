"""The head's bandwidth-bound helpers, bit for bit against the code as it was before their kernels
were rewritten for the HBM rate (tests/golden/head_helpers_before.json): dZ7 = gate(dL W8) with its
row / column maxima (naws_gemm_f32_amax, NN form), the two fc8 products (naws_gemm_f32_splitk),
the loss tail's softmax + entropy gate (naws_wsddn_outputs_fwd, naws_entropy_gate_fwd) and conv1_1
(naws_conv3x3_c3_nchw_to_nhwc_fwd).

record() uses only entry points and wrappers the parent of that change had, so this file run as a
script against a checkout of the parent, `python tests/test_gpu_head_helpers_bits.py OUT.json`,
writes the fixture (the convention of tests/test_gpu_head_plans.py).

Shapes are the smallest that reach the branches: Rt = 1, 40 (the tiny model's, no multiple of 16)
and 257 (one row past a tile; with 4096 columns the only one above the short-K kernel's 2^20
element threshold); C = 21 gives ld8 = 44, the padded fc8 route; K = Rt = 257 is no multiple of the
split-K slice length.  Every output lives in a guard-banded buffer (tests/guard.py) whose bands
must still hold the sentinel; the GEMM outputs are the engine's batch-2 column-interleaved views of
a row-strided (non-contiguous) matrix."""
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'head_helpers_before.json')
RTS = (1, 40, 257)
CLASSES = (20, 21)
SEGS = {'24+16': (24, 16), '1+39': (1, 39)}
CONVS = {'1x9x33': (1, 9, 33), '2x64x96': (2, 64, 96)}
CASES = (['dz7-%d-%d-%d' % (r, c, h) for r in RTS for c in CLASSES for h in (4096, 64)]
         + ['fc8fwd-%d-%d-%d' % (r, c, k) for r in RTS for c in CLASSES for k in (4, 1)]
         + ['fc8wgrad-%d-%d-%d' % (r, c, k) for r in RTS for c in CLASSES for k in (4, 1)]
         + ['tail-%s-%d' % (s, c) for s in SEGS for c in CLASSES]
         + ['conv11-%s' % s for s in CONVS])


def _digest(t):
    """SHA-256 of a tensor's bytes (any dtype, any strides)."""
    import torch
    return hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy()
                          .tobytes()).hexdigest()


def _randn(shape, seed, dev, scale=1.0):
    import torch
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)


def _interleaved(g2d, width):
    """The engine's [2, rows, width] view of a [rows, 2 * width] matrix (row stride kept)."""
    import torch
    rows = g2d.shape[0]
    return torch.as_strided(g2d, (2, rows, width), (width, g2d.stride(0), 1), g2d.storage_offset())


def _h7(rt, hid, dev, ld):
    """ReLU + Dropout-like activations [rt, 2 * hid] with row stride ld: exact zeros, negatives
    (which the gate must treat as closed) and positives."""
    import torch
    import guard
    h = torch.randn((rt, 2 * hid), generator=torch.Generator().manual_seed(7))
    h[torch.rand((rt, 2 * hid), generator=torch.Generator().manual_seed(8)) < 0.4] = 0.0
    return guard.place(h.to(dev), ld=ld)


def _dl(rt, c, dev):
    """dL [rt, 2 * ld8] with zero padding columns, as the engine makes it for an odd 2C."""
    import torch
    ld8 = (2 * c + 3) // 4 * 4
    dl = torch.zeros((rt, 2, ld8))
    dl[:, :, :2 * c] = torch.randn((rt, 2, 2 * c), generator=torch.Generator().manual_seed(3)) * 1e-3
    return dl.view(rt, 2 * ld8).to(dev), ld8


def _w8(c, hid, dev):
    import torch
    ld8 = (2 * c + 3) // 4 * 4
    w = torch.zeros((2, ld8, hid))
    w[:, :2 * c] = torch.randn((2, 2 * c, hid), generator=torch.Generator().manual_seed(4)) * 0.02
    return w.to(dev)


def _rec_dz7(dev, rt, c, hid):
    import torch
    import guard
    from naws_hip import lib as L, ops
    dl, ld8 = _dl(rt, c, dev)
    dlv = dl.view(rt, 2, ld8).permute(1, 0, 2)
    w8 = _w8(c, hid, dev)
    ld = 2 * hid + 8                                    # a row gap: non-contiguous out and aux
    h7 = _h7(rt, hid, dev, ld)
    gout = guard.carve((rt, 2 * hid), torch.float32, dev, ld=ld)
    grow = guard.carve((2 * rt,), torch.int32, dev)
    gcol = guard.carve((2 * hid,), torch.int32, dev)
    grow.t.zero_()
    gcol.t.zero_()
    ops.gemm(dlv, w8, False, False, out=_interleaved(gout.t, hid), epilogue=L.EPI_GATE_POS,
             aux=_interleaved(h7.t, hid), alpha=2.0, rowmax=grow.t, colmax=gcol.t)
    torch.cuda.synchronize()
    for g, what in ((gout, 'dZ7'), (grow, 'rowmax'), (gcol, 'colmax'), (h7, 'h7')):
        g.check(what)
    return {'dz7': _digest(gout.t), 'rowmax': _digest(grow.t), 'colmax': _digest(gcol.t)}


def _rec_fc8(dev, kind, rt, c, ks):
    import torch
    import guard
    from naws_hip import lib as L, ops
    hid = 4096
    dl, ld8 = _dl(rt, c, dev)
    h7 = _h7(rt, hid, dev, 2 * hid)
    h7v = _interleaved(h7.t, hid)
    if kind == 'fc8fwd':                                # logits = h7 W8^T + b8: [2, rt, ld8] views
        w8 = _w8(c, hid, dev)
        b8 = _randn((2, ld8), 5, dev, 0.05)
        gout = guard.carve((rt, 2 * ld8), torch.float32, dev, ld=2 * ld8 + 4)
        need = rt * ld8 * 2 * ks
        gws = guard.carve((need,), torch.float32, dev)
        ops.gemm_splitk(h7v, w8, False, True, out=_interleaved(gout.t, ld8), epilogue=L.EPI_BIAS,
                        bias=b8, ksplit=ks, workspace=gws.t)
    else:                                               # dW8 = dL^T h7: [2, ld8, 4096]
        dlv = dl.view(rt, 2, ld8).permute(1, 0, 2)
        gout = guard.carve((2, ld8, hid), torch.float32, dev, ld=hid + 4,
                           batch_stride=ld8 * (hid + 4) + 8)
        need = ld8 * hid * 2 * ks
        gws = guard.carve((need,), torch.float32, dev)
        ops.gemm_splitk(dlv, h7v, True, False, out=gout.t, ksplit=ks, workspace=gws.t)
    torch.cuda.synchronize()
    gout.check(kind)
    gws.check(kind + ' workspace')
    return {'out': _digest(gout.t)}


def _rec_tail(dev, segs, c):
    import torch
    import guard
    from naws_hip import lib as L
    lens = SEGS[segs]
    rt, nseg = sum(lens), len(lens)
    ld8 = (2 * c + 3) // 4 * 4
    seg_off = torch.tensor([0] + [sum(lens[:i + 1]) for i in range(nseg)], dtype=torch.int32).to(dev)
    lg = _randn((rt, 2 * ld8), 9, dev, 1.5)
    lv = [lg[:, o:o + c] for o in (0, c, ld8, ld8 + c)]
    g = torch.Generator().manual_seed(10)
    xy = torch.randint(0, 60, (rt, 2), generator=g)
    wh = torch.randint(1, 40, (rt, 2), generator=g)
    img = torch.cat([torch.full((n, 1), i) for i, n in enumerate(lens)])
    rois = torch.cat([img, xy, xy + wh], 1).float().to(dev)
    rois[1, 1:] = rois[0, 1:]                           # a duplicate box: IoU 1 off the diagonal
    labels = (torch.rand((nseg, c), generator=g) < 0.3).float().to(dev)
    outs = [guard.carve((2 * rt * c,), torch.float32, dev) for _ in range(3)]     # ac, ad, rp
    gcp = guard.carve((2 * nseg * c,), torch.float32, dev)
    s = torch.cuda.current_stream().cuda_stream
    L.call('naws_wsddn_outputs_fwd', lv[0].data_ptr(), lv[1].data_ptr(), lv[2].data_ptr(),
           lv[3].data_ptr(), lg.stride(0), seg_off.data_ptr(), nseg, rt, c, outs[0].t.data_ptr(),
           outs[1].t.data_ptr(), outs[2].t.data_ptr(), gcp.t.data_ptr(), s)
    nws = L.load().naws_entropy_gate_workspace_floats(rt, c, nseg, max(lens))
    gws = guard.carve((max(int(nws), 4),), torch.float32, dev)
    gate = [guard.carve((nseg * c,), torch.float32, dev) for _ in range(4)]
    L.call('naws_entropy_gate_fwd', rois.data_ptr(), outs[2].t.data_ptr(), gcp.t.data_ptr(),
           labels.data_ptr(), seg_off.data_ptr(), nseg, rt, c, max(lens), gws.t.data_ptr(),
           gate[0].t.data_ptr(), gate[1].t.data_ptr(), gate[2].t.data_ptr(), gate[3].t.data_ptr(), s)
    torch.cuda.synchronize()
    out = {}
    names = ('alpha_cls', 'alpha_det', 'rois_pred', 'cls_prob', 'class_weight',
             'class_weight_noise', 'hatE_sum', 'hatE_sum_norm')
    for name, gd in zip(names, outs + [gcp] + gate):
        gd.check(name)
        out[name] = _digest(gd.t)
    gws.check('gate workspace')
    return out


def _rec_conv(dev, shape):
    import torch
    import guard
    from naws_hip import ops
    n, h, w = CONVS[shape]
    x = _randn((n, 3, h, w), 12, dev)
    wt = _randn((64, 3, 3, 3), 13, dev, 0.2)
    b = _randn((64,), 14, dev, 0.1)
    gout = guard.carve((n, h, w, 64), torch.float32, dev)
    ops.conv3x3_c3_nchw_to_nhwc(x, wt, b, relu=True, out=gout.t)
    torch.cuda.synchronize()
    gout.check('conv1_1')
    return {'y': _digest(gout.t)}


def record(dev, case):
    p = case.split('-')
    if p[0] == 'dz7':
        return _rec_dz7(dev, int(p[1]), int(p[2]), int(p[3]))
    if p[0] in ('fc8fwd', 'fc8wgrad'):
        return _rec_fc8(dev, p[0], int(p[1]), int(p[2]), int(p[3]))
    if p[0] == 'tail':
        return _rec_tail(dev, p[1], int(p[2]))
    return _rec_conv(dev, p[1])


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES)
def test_helper_is_bit_identical_to_parent(dev, case):
    """Every output of the entry point (maxima included) has the digest the parent of the kernel
    rewrite produced, and nothing outside the outputs was written."""
    want = json.load(open(FIXTURE))[case]
    got = record(dev, case)
    assert sorted(got) == sorted(want)
    diff = [k for k in sorted(want) if got[k] != want[k]]
    assert not diff, (case, diff)


if __name__ == '__main__':
    for p in (ROOT, os.path.join(ROOT, 'na-fwebsod_amd'), os.path.join(ROOT, 'tests')):
        sys.path.insert(0, p)
    import torch
    rec = {case: record(torch.device('cuda:0'), case) for case in CASES}
    with open(sys.argv[1], 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
