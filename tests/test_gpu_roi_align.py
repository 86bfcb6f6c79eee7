"""GPU parity of RoIAlign / RoIAlignGradient (FAST_RCNN.ROI_XFORM_METHOD RoIAlign) against the
float64 references of tests/roi_align_ref.py.

The bounds are derived, not measured.  An output element is a sum of n reference terms (one per
valid sample pair and tap) whose absolute values sum to S: evaluated in float32 in ANY order, with
or without FMA, each term is rounded once and takes part in at most n - 1 additions, so the error
is at most (n + 16) 2^-24 S - the 16 covers forming 1 - l, the pre-summed weights of the separable
form and the division by the sample count.  The same holds for dX with its T terms of absolute sum
A, atomics included.  An element with S = 0 (A = 0) has no term at all and must be bitwise 0."""
import os

import numpy as np
import pytest
import torch

import guard
import roi_align_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, 'na-fwebsod_amd', 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
U = 2.0 ** -24
CMAX = 96
CHANNELS = (32, 64, 96)
SCALE = 0.125
_REF = {}


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _x(c=CMAX):
    return np.random.default_rng(17).standard_normal(
        (ref.MAP_N, c, ref.MAP_H, ref.MAP_W)).astype(np.float32)


def _dy(r, c, ph, pw):
    return np.random.default_rng(23).standard_normal((r, c, ph, pw)).astype(np.float32)


def _reference(key, rois, ph, pw, scale, sampling, c=CMAX):
    """The float64 forward and backward of one configuration at c channels, computed once."""
    k = (key, ph, pw, scale, sampling, c)
    if k not in _REF:
        x = _x(c)
        dy = _dy(len(rois), c, ph, pw)
        _REF[k] = dict(x=x, dy=dy, fwd=ref.forward64(x, rois, ph, pw, scale, sampling),
                       bwd=ref.backward64(dy, rois, x.shape, scale, sampling))
    return _REF[k]


def _check_forward(got, y, n, S, what):
    err = np.abs(got.astype(np.float64) - y)
    bound = (n + 16) * U * S
    live = S > 0
    worst = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print('%s: max err %.3g, max err / bound %.3g, up to %d terms' % (what, err.max() if err.size else 0.0, worst, n.max() if n.size else 0))
    assert got.shape == y.shape
    assert (err <= bound).all(), what
    assert not _bits(got)[~live].any(), what + ': an element without a term is not +0'
    return worst


def _check_backward(got, dx, T, A, what):
    err = np.abs(got.astype(np.float64) - dx)
    bound = (T + 16) * U * A
    live = A > 0
    worst = float((err[live] / bound[live]).max()) if live.any() else 0.0
    print('%s: max err %.3g, max err / bound %.3g, up to %d terms' % (what, err.max() if err.size else 0.0, worst, T.max() if T.size else 0))
    assert got.shape == dx.shape
    assert (err <= bound).all(), what
    assert not _bits(got)[np.broadcast_to(T == 0, got.shape)].any(), what + ': outside every window'
    return worst


def _forward_both_layouts(dev, x, rois, ph, pw, scale, sampling):
    from naws_hip import ops
    rr = _t(rois, dev)
    a = ops.roi_align(_t(x, dev), rr, ph, pw, scale, sampling, layout='NCHW')
    b = ops.roi_align(_t(x.transpose(0, 2, 3, 1), dev), rr, ph, pw, scale, sampling, layout='NHWC')
    assert torch.equal(a, b)               # one kernel form: the wrapper only transposes
    return a.cpu().numpy()


def _backward_both_layouts(dev, dy, rois, shape, scale, sampling):
    from naws_hip import ops
    n, c, h, w = shape
    rr = _t(rois, dev)
    a = ops.roi_align_grad(_t(dy, dev), rr, shape, scale, sampling, layout='NCHW').cpu().numpy()
    b = ops.roi_align_grad(_t(dy, dev), rr, (n, h, w, c), scale, sampling, layout='NHWC')
    assert a.shape == tuple(shape) and b.shape == (n, h, w, c)
    return a, b.cpu().numpy().transpose(0, 3, 1, 2)


# --------------------------------------------------------------------------------- forward ----
@pytest.mark.parametrize('sampling', ref.SAMPLINGS)
@pytest.mark.parametrize('ph,pw', ref.POOLINGS)
def test_forward_case_list(dev, ph, pw, sampling):
    """The ten rois of the case list on the 13 x 17 map, N = 2, C in {32, 64, 96} (a half tile, one
    tile, one and a half), both layouts of the wrapper; two calls are bit-identical."""
    rois = ref.case_rois()
    r = _reference('cases', rois, ph, pw, SCALE, sampling)
    y, n, S = r['fwd']
    for c in CHANNELS:
        got = _forward_both_layouts(dev, r['x'][:, :c], rois, ph, pw, SCALE, sampling)
        _check_forward(got, y[:, :c], n, S[:, :c], '%dx%d s%d C%d' % (ph, pw, sampling, c))
        again = _forward_both_layouts(dev, r['x'][:, :c], rois, ph, pw, SCALE, sampling)
        assert np.array_equal(_bits(got), _bits(again))
    names = [k for k, _ in ref.CASE_ROIS]
    assert not _bits(got[names.index('wholly_outside')]).any()


def test_forward_other_scale_and_many_channel_tiles(dev):
    """spatial_scale 0.0625 once; C = 320: five channel tiles, so two workgroups per roi."""
    rois = ref.case_rois()
    r = _reference('cases', rois, 7, 7, 0.0625, 0, c=32)
    got = _forward_both_layouts(dev, r['x'], rois, 7, 7, 0.0625, 0)
    _check_forward(got, *r['fwd'], 'scale 0.0625')
    r = _reference('cases', rois, 3, 5, SCALE, 2, c=320)
    got = _forward_both_layouts(dev, r['x'], rois, 3, 5, SCALE, 2)
    _check_forward(got, *r['fwd'], 'C 320')
    a, b = _backward_both_layouts(dev, r['dy'], rois, r['x'].shape, SCALE, 2)
    _check_backward(a, *r['bwd'], 'C 320 backward')


SPECIAL = [(k, np.array([ref.CASE_ROIS[0][1], roi, ref.CASE_ROIS[5][1]], np.float32))
           for k, roi in ref.INVALID_ROIS]
SPECIAL += [('R%d' % k, ref.rois_many(k)) for k in (0, 1, 130)]


@pytest.mark.parametrize('name,rois', SPECIAL, ids=[k for k, _ in SPECIAL])
def test_special_rois_forward_and_backward(dev, name, rois):
    """A batch index of 2 and of -1, a NaN coordinate, a roi 1e6 wide (the 1024 cap) - each between
    two good rois: its Y is +0 and it adds nothing to dX - and R = 0, 1, 130 (dX is zero-filled
    when R = 0).  7 x 7, adaptive sampling, C = 96."""
    r = _reference(name, rois, 7, 7, SCALE, 0)
    got = _forward_both_layouts(dev, r['x'], rois, 7, 7, SCALE, 0)
    _check_forward(got, *r['fwd'], name)
    a, b = _backward_both_layouts(dev, r['dy'], rois, r['x'].shape, SCALE, 0)
    _check_backward(a, *r['bwd'], name + ' backward NCHW')
    _check_backward(b, *r['bwd'], name + ' backward NHWC')
    if len(rois) == 3:
        assert not _bits(got[1]).any() and got[0].any() and got[2].any()
        # the same dY rows on the good rois alone: the invalid roi's row changes nothing
        want = ref.backward64(r['dy'][[0, 2]], rois[[0, 2]], r['x'].shape, SCALE, 0)
        assert np.array_equal(want[1], r['bwd'][1]) and np.abs(want[0] - r['bwd'][0]).max() == 0
    if len(rois) == 0:
        assert got.shape == (0, CMAX, 7, 7) and not _bits(a).any() and not _bits(b).any()


def test_geometry_probe(dev):
    """An 8 x 8 map with C = 64, channel k one-hot at pixel k: Y IS the weight table (every bin's
    summed tap weights over the sample count), so the geometry itself is compared - same bound,
    and the zero pattern must equal the reference's."""
    from naws_hip import ops
    x = np.zeros((1, 64, 8, 8), np.float32)
    x.reshape(64, 64)[np.arange(64), np.arange(64)] = 1.0
    rois = np.array([(0, 8, 16, 50, 40), (0, 0, 0, 63, 63), (0, -12, -9, 30, 20), (0, 40, 30, 90, 80),
                     (0, 33.3, 21.7, 35.1, 22.2), (0, 16, 8, 48, 56), (0, 50, 40, 30, 20),
                     (0, 200, 200, 300, 300), (0, -9, -9, 72, 72), (0, 56, 56, 64, 64)], np.float32)
    for ph, pw in ref.POOLINGS:
        for sampling in ref.SAMPLINGS:
            y, n, S = ref.forward64(x, rois, ph, pw, SCALE, sampling)
            got = ops.roi_align(_t(x, dev), _t(rois, dev), ph, pw, SCALE, sampling).cpu().numpy()
            _check_forward(got, y, n, S, 'probe %dx%d s%d' % (ph, pw, sampling))
            assert np.array_equal(got == 0, y == 0)
            # a bin's weights sum to (valid sample pairs) / (all pairs) <= 1
            assert (got.sum(axis=1) <= 1 + 1e-5).all()


# -------------------------------------------------------------------------------- backward ----
@pytest.mark.parametrize('sampling', ref.SAMPLINGS)
@pytest.mark.parametrize('ph,pw', ref.POOLINGS)
def test_backward_case_list(dev, ph, pw, sampling):
    rois = ref.case_rois()
    r = _reference('cases', rois, ph, pw, SCALE, sampling)
    dx, T, A = r['bwd']
    for c in CHANNELS:
        shape = (ref.MAP_N, c, ref.MAP_H, ref.MAP_W)
        a, b = _backward_both_layouts(dev, r['dy'][:, :c], rois, shape, SCALE, sampling)
        _check_backward(a, dx[:, :c], T, A[:, :c], 'bwd %dx%d s%d C%d NCHW' % (ph, pw, sampling, c))
        _check_backward(b, dx[:, :c], T, A[:, :c], 'bwd %dx%d s%d C%d NHWC' % (ph, pw, sampling, c))
    assert (T == 0).any() and (T > 0).any()


def test_ops_layer(dev):
    """detectron.ops.RoIAlign / RoIAlignGradient are the same numbers."""
    import detectron.ops as O
    rois = ref.case_rois()
    r = _reference('cases', rois, 7, 7, SCALE, 2)
    x, rr = _t(r['x'], dev), _t(rois, dev)
    y = O.RoIAlign(x, rr, 7, 7, SCALE, 2)
    assert isinstance(y, torch.Tensor)
    _check_forward(y.cpu().numpy(), *r['fwd'], 'O.RoIAlign')
    dx = O.RoIAlignGradient(x, rr, _t(r['dy'], dev), 7, 7, SCALE, 2)
    _check_backward(dx.cpu().numpy(), *r['bwd'], 'O.RoIAlignGradient')


# ----------------------------------------------------------------------------- guard bands ----
@pytest.mark.parametrize('aligned', [True, False])
def test_guard_bands(dev, aligned):
    """Y and dX carved out of a sentinel-filled buffer (on a 16-byte boundary and one word off it),
    X, rois and dY inside poison, C = 96 (masked lanes), the invalid rois among the good ones:
    nothing outside the views is written, every element of the views is, and the values equal the
    plain call's.  The C ABI takes dense tensors only: a strided view is refused before a launch
    and leaves its buffer untouched."""
    from naws_hip import ops
    rois = np.concatenate([ref.case_rois(), np.array([r for _, r in ref.INVALID_ROIS], np.float32)])
    c, ph, pw = 96, 3, 5
    x = _x(c).transpose(0, 2, 3, 1)                                     # NHWC
    dy = _dy(len(rois), c, ph, pw)
    gx, gr, gdy = (guard.place(_t(v, dev), aligned=aligned) for v in (x, rois, dy))
    for sampling in (0, 2):
        plain = ops.roi_align(_t(x, dev), _t(rois, dev), ph, pw, SCALE, sampling, layout='NHWC')
        gy = guard.carve(plain.shape, device=dev, aligned=aligned)
        ops.roi_align(gx.t, gr.t, ph, pw, SCALE, sampling, layout='NHWC', out=gy.t)
        torch.cuda.synchronize()
        gy.check('Y')
        assert guard.same_bits(gy.t, plain)                  # (no NaN: every element was written)
        ref_dx = ops.roi_align_grad(_t(dy, dev), _t(rois, dev), x.shape, SCALE, sampling,
                                    layout='NHWC')
        gdx = guard.carve(x.shape, device=dev, aligned=aligned)
        ops.roi_align_grad(gdy.t, gr.t, x.shape, SCALE, sampling, layout='NHWC', out=gdx.t)
        torch.cuda.synchronize()
        gdx.check('dX')
        assert not torch.isnan(gdx.t).any()
        d64 = ref.backward64(dy, rois, (ref.MAP_N, c, ref.MAP_H, ref.MAP_W), SCALE, sampling)
        _check_backward(gdx.t.cpu().numpy().transpose(0, 3, 1, 2), *d64, 'guarded dX')
        _check_backward(ref_dx.cpu().numpy().transpose(0, 3, 1, 2), *d64, 'plain dX')
        for g in (gx, gr, gdy):
            g.check('an input')
    # strided views: rows of Y [R, C*ph*pw] with a gap, pixels of dX [N*H*W, C] with a gap
    sy = guard.carve((len(rois), c * ph * pw), device=dev, ld=c * ph * pw + 3)
    sdx = guard.carve((ref.MAP_N * ref.MAP_H * ref.MAP_W, c), device=dev, ld=c + 5)
    with pytest.raises(ValueError):
        ops.roi_align(gx.t, gr.t, ph, pw, SCALE, 0, layout='NHWC',
                      out=sy.t.as_strided((len(rois), c, ph, pw), (sy.ld, ph * pw, pw, 1)))
    with pytest.raises(ValueError):
        ops.roi_align_grad(gdy.t, gr.t, x.shape, SCALE, 0, layout='NHWC',
                           out=sdx.t.as_strided(x.shape, (ref.MAP_H * ref.MAP_W * sdx.ld,
                                                          ref.MAP_W * sdx.ld, sdx.ld, 1)))
    torch.cuda.synchronize()
    for g in (sy, sdx):
        g.check('a refused view')
        assert guard.holds_sentinel(g.t)


# ------------------------------------------------------------------------------ end to end ----
NFG = 20
BOUND = 5e-4          # of max|ref| per gradient blob: tests/test_gpu_body_backward.py's BOUND
WSDDN = ['WEBLY.WEBLY_ON', False, 'FAST_RCNN.ROI_BOX_HEAD', 'wsl_heads.add_VGG16_roi_2fc_head']
MODELS = {'na_wsddn': [], 'wsddn': WSDDN}


def _inputs():
    from test_gpu_body_backward import _inputs as tiny
    return tiny('na_wsddn')           # 3 x 48 x 64, 12 rois, 20 classes; non-zero conv biases


def _run(dev, name, sampling, frozen, train):
    """One NetExecutor.run() of the tiny model under ROI_XFORM_METHOD RoIAlign with every forward
    op's outputs recorded."""
    from detectron.core import config as c
    from detectron.core.executor import NetExecutor
    import detectron.modeling.model_builder_wsl as mbld
    c.reset_cfg()
    try:
        c.merge_cfg_from_file(YAML)
        c.merge_cfg_from_list(['NUM_GPUS', 1, 'TRAIN.FREEZE_CONV_BODY', frozen,
                               'FAST_RCNN.ROI_XFORM_METHOD', 'RoIAlign',
                               'FAST_RCNN.ROI_XFORM_SAMPLING_RATIO', sampling] + MODELS[name])
        c.assert_and_infer_cfg(make_immutable=False)
        model = mbld.create('generalized_wsl', train=train)
        ex = NetExecutor(model, dev, disable_dropout=True)
        assert ex.plan == 'interpreted'                    # never the fused engine, unforced
        assert [o.type for o in model.net.ops].count('RoIAlign') == 1
        blobs, mb = _inputs()
        ex.load_blobs({k: v.clone() for k, v in blobs.items()})
        snaps = []
        fwd = ex._forward

        def recording(idx, op, ws):
            fwd(idx, op, ws)
            snaps.append([ws.get(o) for o in op.outputs])      # (Concat's dims blob is never made)
        ex._forward = recording
        if train:
            model.UpdateWorkspaceLr(0, 1e-3)
        ex.feed({k: torch.from_numpy(v).to(dev) for k, v in mb.items()})
        ex.run()
        torch.cuda.synchronize()
        out = dict(model=model, blobs=blobs, mb=mb, snaps=snaps,
                   cls_prob=ex.fetch('cls_prob').cpu().numpy())
        if train:
            out['grads'] = {p: ex.ws[g].cpu().numpy().copy() for p, g in model.param_to_grad.items()}
            out['losses'] = {l: ex.ws[l].reshape(-1)[0].item() for l in model.losses}
    finally:
        c.reset_cfg()
    return out


@pytest.mark.parametrize('sampling', [2, 0])
@pytest.mark.parametrize('name', sorted(MODELS))
def test_trainable_body_end_to_end(dev, name, sampling):
    """Every gradient blob of one iteration (conv3_1..conv5_3 through RoIAlignGradient, and the
    head) within 5e-4 of max|ref| of the graph restated in torch CPU double.  fc8d_b (and
    noisy_fc8d_b) are exactly zero in exact arithmetic - the detection softmax runs over the rois -
    and are measured against the terms they sum, as tests/test_gpu_body_backward.py does."""
    r = _run(dev, name, sampling, frozen=False, train=True)
    model = r['model']
    assert 'RoIAlignGradient' in [o.type for o in model.grad_ops]
    body = {'conv%d_%d%s' % (i, j, s) for i in (3, 4, 5) for j in (1, 2, 3) for s in ('_w', '_b')}
    assert body <= set(model.TrainableParams())
    want, terms, _ = ref.graph64(model, r['blobs'], r['mb'], r['snaps'])
    worst = {}
    for p in sorted(model.param_to_grad):
        got = r['grads'][p].reshape(want[p].shape)
        if p in terms and np.abs(want[p]).max() <= 2.0 ** -40 * terms[p]:
            assert p in ('fc8d_b', 'noisy_fc8d_b'), p
            worst[p] = float(np.abs(got - want[p]).max() / terms[p])
            continue
        assert np.abs(want[p]).max() > 0, p
        worst[p] = float(np.abs(got - want[p]).max() / np.abs(want[p]).max())
    for p in sorted(worst, key=worst.get, reverse=True)[:6]:
        print('%s s%d %s: max err / max|ref| = %.3g' % (name, sampling, p, worst[p]))
    print('%s s%d worst over the 18 body blobs: %.3g' % (name, sampling,
                                                       max(worst[p] for p in body)))
    for p, v in worst.items():
        assert v <= BOUND, (p, v)


@pytest.mark.parametrize('sampling', [2, 0])
@pytest.mark.parametrize('name', sorted(MODELS))
def test_frozen_body_forward_values(dev, name, sampling):
    """Frozen body, train and test mode: cls_prob within 1e-5 of its maximum and every loss within
    1e-4 (relative) of the float64 restatement - the bounds the README states for the plans."""
    for train in (True, False):
        r = _run(dev, name, sampling, frozen=True, train=train)
        model = r['model']
        assert not [o for o in model.grad_ops if o.type.startswith(('RoI', 'Conv'))]
        grads, _, env = ref.graph64(model, r['blobs'], r['mb'], r['snaps'])
        cp = env['cls_prob'].detach().numpy()
        err = float(np.abs(r['cls_prob'] - cp).max() / np.abs(cp).max())
        print('%s s%d %s: cls_prob max err / max = %.3g' % (name, sampling,
                                                          'train' if train else 'test', err))
        assert r['cls_prob'].shape == cp.shape and err <= 1e-5
        if not train:
            continue
        assert model.losses
        for l in model.losses:
            a, b = r['losses'][l], float(env[l].detach().reshape(-1)[0])
            print('   %s: %.6g against %.6g' % (l, a, b))
            assert abs(a - b) <= 1e-4 * abs(b), l
        for p in sorted(grads):                          # the head's gradients, same bound as above
            w = grads[p]
            if np.abs(w).max() > 1e-12:
                e = float(np.abs(r['grads'][p].reshape(w.shape) - w).max() / np.abs(w).max())
                assert e <= BOUND, (p, e)


def test_inference_entry_point(dev):
    """One im_detect_all call on a synthetic image under RoIAlign: the interpreted route (the
    device-resident one needs an engine), finite detections."""
    from detectron.core import config as c
    from detectron.core import test_wsl
    from detectron.core.executor import NetExecutor
    from detectron.datasets import synthetic
    import detectron.modeling.model_builder_wsl as mbld
    c.reset_cfg()
    try:
        c.merge_cfg_from_file(YAML)
        c.merge_cfg_from_list(['NUM_GPUS', 1, 'FAST_RCNN.ROI_XFORM_METHOD', 'RoIAlign',
                               'FAST_RCNN.ROI_XFORM_SAMPLING_RATIO', 2, 'TEST.SCALE', 64,
                               'TEST.MAX_SIZE', 200, 'TEST.DETECTIONS_PER_IM', 20,
                               'MODEL.NUM_CLASSES', NFG + 1])
        c.assert_and_infer_cfg(make_immutable=False)
        model = mbld.create('generalized_wsl', train=False)
        ex = NetExecutor(model, dev)
        assert ex.plan == 'interpreted' and ex.engine is None
        ex.load_blobs(synthetic.init_blobs(NFG, seed=3))
        e = synthetic.make_roidb(1, 40, NFG, 64, 96, seed=9)[0]
        im = np.random.default_rng(e['seed']).integers(0, 256, (64, 96, 3), dtype=np.uint8)
        assert not test_wsl.device_post_supported(ex, im, len(e['boxes']))
        cls_boxes = test_wsl.im_detect_all(ex, im, e['boxes'], e['obn_scores'])
        assert ex.plan == 'interpreted'
        assert len(cls_boxes) == NFG + 1
        assert 0 < sum(len(b) for b in cls_boxes[1:]) <= 20
        assert all(np.isfinite(b).all() for b in cls_boxes[1:])
    finally:
        c.reset_cfg()
