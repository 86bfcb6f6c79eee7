"""The sized workspaces (naws_*_workspace_*()): every entry that takes one runs with a workspace
carved from a sentinel-filled buffer (tests/guard.py) at EXACTLY its declared size, at one residue
shape of its own test.  The result must be what the call with the wrapper's own allocation gives,
bit for bit, the guard around the workspace intact, and a workspace one element short refused with
a TypeError (the contract of conv3x3_nhwc_wgrad's `workspace`)."""
import numpy as np
import pytest
import torch

import guard
import tail_ref as T
from helpers import make_rois

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _declared(sizer, *dims):
    from naws_hip import lib as L
    need = int(getattr(L.load(), sizer)(*dims))
    assert need > 0
    return need


def _check(dev, need, dtype, run):
    """run(workspace) -> tensor or tuple of tensors."""
    def outs(ws):
        o = run(ws)
        return o if isinstance(o, (tuple, list)) else (o,)
    want = outs(None)
    gws = guard.carve((need,), dtype, dev)
    got = outs(gws.t)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert guard.same_bits(g, w)
    gws.check('workspace')
    if need > 4:                      # (the wrappers round their own allocation up to 4 elements)
        with pytest.raises(TypeError):
            run(gws.t[:need - 1])
    with pytest.raises(TypeError):
        run(torch.empty((need,), device=dev, dtype=torch.float64))


def _conv_case(dev, cin, cout, h, w):
    rng = np.random.default_rng(48)
    x = np.maximum(rng.standard_normal((2, h, w, cin)), 0).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, cout).astype(np.float32)
    return _t(x, dev), _t(wt, dev), _t(b, dev)


# (128 -> 256 at 19 x 23, dilation 1: tests/test_gpu_h2.py test_conv3x3_winograd_f16x2)
WINO = (128, 256, 19, 23)


def test_winograd_fp32_workspace(dev):
    from naws_hip import ops
    cin, cout, h, w = WINO
    x, wt, b = _conv_case(dev, *WINO)
    u = ops.winograd_weight_transform(wt)
    need = _declared('naws_winograd_workspace_floats', 2, h, w, cin, cout, 1)
    _check(dev, need, torch.float32,
           lambda ws: ops.conv3x3_winograd_nhwc(x, u, b, 1, True, workspace=ws))


def test_winograd_f32x3_workspace(dev):
    from naws_hip import ops
    cin, cout, h, w = WINO
    x, wt, b = _conv_case(dev, *WINO)
    u3 = ops.split_bf16x3(ops.winograd_weight_transform(wt))
    need = _declared('naws_winograd_f32x3_workspace_floats', 2, h, w, cin, cout, 1)
    _check(dev, need, torch.float32,
           lambda ws: ops.conv3x3_winograd_nhwc_f32x3(x, u3, b, 1, True, workspace=ws))


@pytest.mark.parametrize('cin,cout', [(128, 256), (256, 256)])    # three kernels / the fused kernel
def test_winograd_f16x2_workspace(dev, cin, cout):
    from naws_hip import ops
    h, w = WINO[2:]
    x, wt, b = _conv_case(dev, cin, cout, h, w)
    u2 = ops.split_f16x2(ops.winograd_weight_transform(wt))
    need = _declared('naws_winograd_f16x2_workspace_floats', 2, h, w, cin, cout, 1)
    # (amax_in None: the entry takes max|x| itself, into the last word of the workspace)
    _check(dev, need, torch.float32,
           lambda ws: ops.conv3x3_winograd_nhwc_f16x2(x, u2, b, 1, True, workspace=ws))


def test_winograd4_f16x2_workspace(dev):
    from naws_hip import ops
    cin, cout, h, w = WINO
    x, wt, b = _conv_case(dev, *WINO)
    u4 = ops.split_f16x2(ops.winograd4_weight_transform(wt))
    need = _declared('naws_winograd4_f16x2_workspace_floats', 2, h, w, cin, cout, 1)
    _check(dev, need, torch.float32,
           lambda ws: ops.conv3x3_winograd_nhwc_f16x2(x, u4, b, 1, True, workspace=ws))


@pytest.mark.parametrize('form', ['fp32', 'f16x2'])
def test_roi_pool_hier_workspace(dev, form):
    """20 x 30 map, 2 x 40 rois, 128 channels: tests/test_gpu_ops.py
    test_roi_pool_hierarchical_bitexact."""
    from naws_hip import ops
    rng = np.random.default_rng(600)
    n, c, h, w = 2, 128, 20, 30
    x = _t(rng.standard_normal((n, h, w, c)).astype(np.float32), dev)
    rois = _t(make_rois(rng, n, 40, h * 8, w * 8), dev)
    boost = _t((rng.uniform(0, 1, rois.shape[0]) + 1).astype(np.float32), dev)
    need = _declared('naws_roi_pool_workspace_floats', n, c, h, w)
    if form == 'fp32':
        _check(dev, need, torch.float32, lambda ws: ops.roi_pool_f(
            x, rois, 7, 7, 0.125, boost=boost, layout='NHWC', hier=True, workspace=ws))
    else:
        amax = torch.tensor([np.float32(8.0).view(np.int32)] * n, device=dev, dtype=torch.int32)

        def run(ws):
            op = ops.roi_pool_f_f16x2(x, rois, amax, 7, 7, 0.125, boost=boost, hier=True, workspace=ws)
            return op.planes, op.scales[1]
        _check(dev, need, torch.float32, run)


@pytest.mark.parametrize('r,c', [(65, 2), (300, 5)])               # tests/test_gpu_nms.py
def test_nms_workspace(dev, r, c):
    from naws_hip import ops
    rng = np.random.default_rng(41 + r)
    xy = rng.integers(0, 80, (r, 2)).astype(np.float32)
    wh = rng.integers(1, 60, (r, 2)).astype(np.float32)
    boxes = _t(np.hstack([xy, xy + wh]).astype(np.float32), dev)
    sc = _t(rng.integers(0, 200, (r, c)).astype(np.float32) / 200.0, dev)
    nbytes = _declared('naws_nms_workspace_bytes', c, r)
    assert nbytes % 4 == 0
    _check(dev, nbytes // 4, torch.int32,
           lambda ws: ops.nms_per_class(boxes, sc, 0.3, 0.3, workspace=ws).to(torch.int32))


def test_entropy_gate_workspace(dev):
    """The ragged segments at C = 21 of tests/test_gpu_tail_edges.py."""
    from naws_hip import ops
    lens, c, _ = T.GATE_CASES[1]
    rois, rp, cp, labels = (_t(np.array(a), dev) for a in T.gate_inputs(lens, c))   # (cached: copies)
    seg = _t(T.seg_of(lens), dev)
    need = _declared('naws_entropy_gate_workspace_floats', sum(lens), c, len(lens), max(lens))
    _check(dev, need, torch.float32,
           lambda ws: ops.entropy_gate(rois, rp, cp, labels, seg, max(lens), workspace=ws))


def test_roi_label_workspace(dev):
    """n = 517, 80 classes, top_k = 2: tests/test_gpu_oicr.py test_roi_label_bitexact."""
    from naws_hip import ops
    n, c, top_k = 517, 80, 2
    rng = np.random.default_rng(n + c)
    rois = _t(make_rois(rng, 1, n, 600, 1000), dev)
    u = ops.roi_iou(rois)
    s = _t(rng.uniform(0, 1, (n, c)).astype(np.float32), dev)
    lab = np.zeros((1, c), np.float32)
    lab[0, rng.choice(c, size=3, replace=False)] = 1
    lab = _t(lab, dev)
    nbytes = _declared('naws_roi_label_workspace_bytes', n, c, top_k)
    assert nbytes % 4 == 0
    _check(dev, nbytes // 4, torch.int32,
           lambda ws: ops.roi_label(s, u, lab, None, 0.5, 0.5, 0.1, top_k, workspace=ws))


@pytest.mark.parametrize('weighted', [False, True])
def test_softmax_with_loss_n_workspace(dev, weighted):
    """n = 333, 81 classes: tests/test_gpu_oicr.py test_softmax_with_loss_n_fwd_bwd."""
    from naws_hip import ops
    n, d = 333, 81
    rng = np.random.default_rng(n)
    x = _t((rng.standard_normal((n, d)) * 4).astype(np.float32), dev)
    t = _t(rng.integers(0, d, (n,)).astype(np.int32), dev)
    w = _t(rng.uniform(0, 1, (n,)).astype(np.float32), dev) if weighted else None
    need = _declared('naws_softmax_with_loss_n_workspace_floats', n)
    _check(dev, need, torch.float32, lambda ws: ops.softmax_with_loss_n(x, t, w, 1.0, workspace=ws))
    p = ops.softmax_with_loss_n(x, t, w, 1.0)[0]
    dl = torch.tensor([0.7], device=dev)
    _check(dev, need, torch.float32,
           lambda ws: ops.softmax_with_loss_n_grad(t, w, p, dl, 1.0, workspace=ws))
