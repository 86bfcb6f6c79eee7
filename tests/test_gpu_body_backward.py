"""GPU parity of the trainable conv body (TRAIN.FREEZE_CONV_BODY False on the op-by-op plan)
against the float64 references of tests/body_grad_ref.py: the conv data / weight / bias gradients,
the max-pool gradient (bit for bit), the RoIPoolF gradient, one training iteration of na_wsddn and
of plain WSDDN + WSL.OICR end to end, and the frozen-body run against the values recorded before
the trainable body existed (tests/golden/frozen_body_before.json)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import body_grad_ref as bgr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, 'na-fwebsod_amd', 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
FROZEN = os.path.join(ROOT, 'tests', 'golden', 'frozen_body_before.json')
BOUND = 5e-4          # of max|ref| per tensor: the project's gradient bound against float64
BODY = ['conv%d_%d' % (i, j) for i, n in ((3, 3), (4, 3), (5, 3)) for j in range(1, n + 1)]
FROZEN_CONVS = ['conv1_1', 'conv1_2', 'conv2_1', 'conv2_2']


def _t(a, dev, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ratio(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------------------------- conv ----
def _conv_case(cin, cout, n, h, w, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) * (2.0 / (9 * cin)) ** 0.5).astype(np.float32)
    b = rng.standard_normal((cout,)).astype(np.float32)
    dy = rng.standard_normal((n, cout, h, w)).astype(np.float32)
    return x, wt, b, dy


@pytest.mark.parametrize('dilation', [1, 2])
@pytest.mark.parametrize('cin,cout', [(32, 64), (64, 32)])
def test_conv_gradient_op(dev, cin, cout, dilation):
    """ConvGradient (N = 1, 9 x 13: a tile residue in both directions) against autograd in float64,
    each tensor within 5e-4 of max|ref|; three wrong backward statements miss that by >= 100x."""
    import detectron.ops as O
    x, wt, b, dy = _conv_case(cin, cout, 1, 9, 13, 100 * cin + dilation)
    dx, dw, db = bgr.conv_grads(x, wt, b, dy, dilation)
    gw, gb, gx = O.ConvGradient(_t(x, dev), _t(wt, dev), _t(dy, dev), pad=dilation,
                                dilation=dilation)
    got = dict(dx=gx.cpu().numpy(), dw=gw.cpu().numpy(), db=gb.cpu().numpy())
    for k, ref in (('dx', dx), ('dw', dw), ('db', db)):
        print('Cin %d Cout %d d %d %s: max err / max|ref| = %.3g' % (cin, cout, dilation, k,
                                                                  _ratio(got[k], ref)))
    for k, ref in (('dx', dx), ('dw', dw), ('db', db)):
        assert got[k].shape == ref.shape and _ratio(got[k], ref) <= BOUND, k
    none = O.ConvGradient(_t(x, dev), _t(wt, dev), _t(dy, dev), pad=dilation, dilation=dilation,
                          need_dx=False)
    assert none[2] is None and torch.equal(none[0], gw) and torch.equal(none[1], gb)
    for kind in ('no_flip', 'no_swap') + (('dilation1',) if dilation == 2 else ()):
        wx, ww = bgr.conv_grads_wrong(kind, x, wt, b, dy, dilation)
        rx, rw = _ratio(got['dx'], wx), _ratio(got['dw'], ww)
        print('  wrong reference %s: dx %.3g dw %.3g' % (kind, rx, rw))
        assert rx >= 100 * BOUND and rw >= 100 * BOUND, kind


@pytest.mark.parametrize('dilation', [1, 2])
def test_conv_wgrad_two_images_cabi(dev, dilation):
    """N = 2 at the C ABI (NHWC): the zero rows between the images keep the taps of one image out
    of the other.  Two calls are bit-identical (split-K sums its slices in a fixed order)."""
    from naws_hip import ops
    cin, cout = 32, 64
    x, wt, b, dy = _conv_case(cin, cout, 2, 9, 13, 7 + dilation)
    _, dw, db = bgr.conv_grads(x, wt, b, dy, dilation)
    xh, dyh = _t(x.transpose(0, 2, 3, 1), dev), _t(dy.transpose(0, 2, 3, 1), dev)
    gw, gb = ops.conv3x3_nhwc_wgrad(xh, dyh, dilation)
    gw2, gb2 = ops.conv3x3_nhwc_wgrad(xh, dyh, dilation)
    print('N 2 d %d: dw %.3g db %.3g' % (dilation, _ratio(gw.cpu().numpy(), dw),
                                       _ratio(gb.cpu().numpy(), db)))
    assert _ratio(gw.cpu().numpy(), dw) <= BOUND and _ratio(gb.cpu().numpy(), db) <= BOUND
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2)
    # the data gradient of the same pair through the packed W'
    dx, _, _ = bgr.conv_grads(x, wt, b, dy, dilation)
    gx = ops.conv3x3_nhwc(dyh, ops.conv3x3_dgrad_pack_weight(_t(wt, dev)), None, dilation,
                          relu=False)
    assert _ratio(gx.cpu().numpy().transpose(0, 3, 1, 2), dx) <= BOUND


# --------------------------------------------------------------------------------- max-pool ----
@pytest.mark.parametrize('stride', [2, 1])
def test_maxpool_gradient_bit_exact(dev, stride):
    """C = 32, 7 x 9: odd sizes (stride 2 drops the last row and column: they get 0), stride 1 puts
    every interior pixel in four windows.  Tie-free input; bit-equal to the float32 restatement
    that adds the windows in ascending index."""
    from naws_hip import ops
    rng = np.random.default_rng(11 + stride)
    n, h, w, c = 2, 7, 9, 32
    x = rng.permutation(n * h * w * c).astype(np.float32).reshape(n, h, w, c) / 64.0 - 100.0
    assert bgr.tie_free(x, stride)
    y, _ = bgr.maxpool_select(x, stride)
    dy = rng.standard_normal(y.shape).astype(np.float32)
    want = bgr.maxpool_grad32(x, dy, stride)
    gy = ops.maxpool2x2_nhwc(_t(x, dev), stride)
    assert np.array_equal(_bits(gy.cpu().numpy()), _bits(y))
    got = ops.maxpool2x2_nhwc_grad(_t(x, dev), gy, _t(dy, dev), stride).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    if stride == 2:
        assert not got[:, 6].any() and not got[:, :, 8].any() and got[:, :6, :8].any()
    else:       # every window's gradient lands exactly once
        assert abs(float(got.astype(np.float64).sum() - dy.astype(np.float64).sum())) < 1e-3
        assert (np.count_nonzero(got) <= dy.size)


def test_maxpool_gradient_all_zero_input(dev):
    """A window tied at 0 (after ReLU): wherever the rule puts its gradient, ReluGradient zeroes it."""
    import detectron.ops as O
    x = torch.zeros((1, 32, 7, 9), device=dev)
    y = O.MaxPool(x, kernel=2, pad=0, stride=2)
    dy = torch.randn(y.shape, device=dev)
    dx = O.MaxPoolGradient(x, y, dy, kernel=2, pad=0, stride=2)
    assert float(dx.abs().sum()) > 0                      # the rule does put it somewhere (on a)
    assert not O.ReluGradient(x, dx).any()


# ---------------------------------------------------------------------------------- RoIPoolF ----
def test_roi_pool_f_gradient(dev):
    """Feature 2 x 32 x 10 x 14 (NCHW), 24 rois of both images with a 1-pixel roi, a roi outside
    the image (every bin empty) and three identical rois.  Per element within n_e 2^-24 sum|terms|
    of the float64 scatter through the forward's own argmax (the worst case of ANY summation order,
    so it holds under atomics); elements nothing contributes to are exactly 0."""
    import detectron.ops as O
    from helpers import make_rois
    rng = np.random.default_rng(21)
    n, c, h, w = 2, 32, 10, 14
    x = rng.standard_normal((n, c, h, w)).astype(np.float32)
    rois = make_rois(rng, n, 12, h * 8, w * 8, degenerate=False)
    rois[1, 1:] = [40, 24, 40, 24]                                   # 1-pixel
    rois[2, 1:] = [w * 16, h * 16, w * 16 + 50, h * 16 + 50]         # outside: all bins empty
    rois[3:6, 1:] = [8, 8, 70, 60]                                   # three identical
    rois[15:18, 1:] = [16, 0, 100, 40]                               # and three in the other image
    assert set(rois[:, 0]) == {0.0, 1.0} and rois.shape == (24, 5)
    xr, rr = _t(x, dev), _t(rois, dev)
    y, am = O.RoIPoolF(xr, rr, 7, 7, 0.125)
    amn = am.cpu().numpy()
    assert (amn[2] == -1).all() and (amn[1] >= 0).all() and np.array_equal(amn[3], amn[4])
    dy = rng.standard_normal(y.shape).astype(np.float32)
    got = O.RoIPoolFGradient(xr, rr, am, _t(dy, dev)).cpu().numpy()
    ref, cnt, asum = bgr.roi_pool_grad64(dy, amn, rois, (n, c, h, w))
    assert cnt.max() >= 3 * 4                # the identical rois share an argmax across many bins
    err = np.abs(got - ref)
    bound = cnt * 2.0 ** -24 * asum
    print('RoIPoolF grad: max err %.3g, max err / bound %.3g, up to %d terms per element'
          % (err.max(), (err[cnt > 0] / np.maximum(bound[cnt > 0], 1e-300)).max(), cnt.max()))
    assert (err <= bound).all()
    assert not got[cnt == 0].any() and got.shape == x.shape
    # NHWC at the tensor level: the same sums
    from naws_hip import ops
    g2 = ops.roi_pool_f_grad(_t(dy, dev), am, rr, (n, h, w, c), layout='NHWC').cpu().numpy()
    assert (np.abs(g2.transpose(0, 3, 1, 2) - ref) <= bound).all()
    # no rois: a zero gradient
    z = ops.roi_pool_f_grad(torch.empty((0, c, 7, 7), device=dev),
                            torch.empty((0, c, 7, 7), device=dev, dtype=torch.int32),
                            torch.empty((0, 5), device=dev), (n, c, h, w))
    assert z.shape == (n, c, h, w) and not z.any()


# -------------------------------------------------------------------------------- end to end ----
NFG = 20
MODELS = {'na_wsddn': [], 'wsddn_oicr': ['WEBLY.WEBLY_ON', False, 'WSL.OICR', True,
                                         'FAST_RCNN.ROI_BOX_HEAD',
                                         'wsl_heads.add_VGG16_roi_2fc_head']}
_RUNS = {}


def _inputs(name):
    from detectron.datasets import synthetic
    blobs = synthetic.init_blobs(NFG, seed=3)
    g = torch.Generator().manual_seed(5)
    if name == 'wsddn_oicr':
        for k in (1, 2, 3):
            blobs['cls_score%d_w' % k] = torch.randn((NFG + 1, 4096), generator=g) * 0.01
            blobs['cls_score%d_b' % k] = torch.randn((NFG + 1,), generator=g) * 0.01
    for k in list(blobs):                       # biases that are not zero: db then matters
        if k.endswith('_b') and k.startswith('conv'):
            blobs[k] = torch.randn(blobs[k].shape, generator=g) * 0.05
    mb = synthetic.make_minibatch(synthetic.make_roidb(1, 12, NFG, 48, 64, seed=5), NFG)
    return blobs, mb


def _run(dev, name, frozen, lr=1e-3):
    """One NetExecutor.run() of the tiny model (3 x 48 x 64, 12 rois, 20 classes, dropout off) with
    every forward op's outputs recorded."""
    key = (name, frozen)
    if key in _RUNS:
        return _RUNS[key]
    from detectron.core import config as c
    from detectron.core.executor import NetExecutor
    import detectron.modeling.model_builder_wsl as mbld
    c.reset_cfg()
    try:
        c.merge_cfg_from_file(YAML)
        c.merge_cfg_from_list(['NUM_GPUS', 1, 'TRAIN.FREEZE_CONV_BODY', frozen] + MODELS[name])
        c.assert_and_infer_cfg(make_immutable=False)
        model = mbld.create('generalized_wsl', train=True)
        ex = NetExecutor(model, dev, disable_dropout=True, force_interpreted=True)
        assert ex.plan == 'interpreted'
        blobs, mb = _inputs(name)
        ex.load_blobs({k: v.clone() for k, v in blobs.items()})
        snaps = []
        fwd = ex._forward

        def recording(idx, op, ws):
            fwd(idx, op, ws)
            snaps.append([ws[o] for o in op.outputs])
        ex._forward = recording
        model.UpdateWorkspaceLr(0, lr)
        ex.feed({k: torch.from_numpy(v).to(dev) for k, v in mb.items()})
        ex.run()
        torch.cuda.synchronize()
        grads = {p: ex.ws[g].cpu().numpy().copy() for p, g in model.param_to_grad.items()}
        losses = {l: ex.ws[l].reshape(-1)[0].item() for l in model.losses}
        after = {k: v.cpu() for k, v in ex.blobs(with_momentum=False).items()}
    finally:
        c.reset_cfg()
    _RUNS[key] = dict(model=model, blobs=blobs, mb=mb, snaps=snaps, grads=grads, losses=losses,
                      after=after)
    return _RUNS[key]


@pytest.mark.parametrize('name', sorted(MODELS))
def test_trainable_body_end_to_end(dev, name):
    """Every gradient blob of one iteration within 5e-4 of max|ref| of the graph restated in torch
    CPU double (ReLU masks, pool selections and RoIPoolF's argmax taken from the GPU forward); after
    the step conv1_1..conv2_2 are bit-identical to their initial values and all 18 trainable conv
    blobs have moved.

    One kind of blob has no max|ref| to be measured against: fc8d_b and noisy_fc8d_b.  The detection
    softmax runs over the rois, so a per-class bias changes nothing and the exact gradient is zero
    (float64 leaves ~1e-17 of cancellation noise, float32 ~1e-9).  Where the reference is below
    2^-40 of the terms it sums (max_c sum_r |dY[r,c]|), the 5e-4 is taken of those terms instead:
    the quantity a sum's rounding error scales with.  Every other blob keeps max|ref|."""
    r = _run(dev, name, False)
    model = r['model']
    trainable = set(model.TrainableParams())
    body = {b + s for b in BODY for s in ('_w', '_b')}
    assert body <= trainable and len(body) == 18
    assert not {b + s for b in FROZEN_CONVS for s in ('_w', '_b')} & set(model.param_to_grad)
    ref, terms = bgr.graph_grads64(model, r['blobs'], r['mb'], r['snaps'])
    worst, cancelled = {}, []
    for p in sorted(model.param_to_grad):
        got = r['grads'][p].reshape(ref[p].shape)
        if p in terms and np.abs(ref[p]).max() <= 2.0 ** -40 * terms[p]:
            cancelled.append(p)
            worst[p] = float(np.abs(got - ref[p]).max() / terms[p])
            continue
        assert np.abs(ref[p]).max() > 0, p
        worst[p] = _ratio(got, ref[p])
    print('%s exact-zero bias gradients (measured against their terms): %s' % (name, cancelled))
    assert set(cancelled) <= {'fc8d_b', 'noisy_fc8d_b'}
    for p in sorted(worst, key=worst.get, reverse=True)[:6]:
        print('%s %s: max err / max|ref| = %.3g' % (name, p, worst[p]))
    print('%s worst over the 18 body blobs: %.3g' % (name, max(worst[p] for p in body)))
    for p, v in worst.items():
        assert v <= BOUND, (p, v)
    for b in FROZEN_CONVS:
        for s in ('_w', '_b'):
            assert np.array_equal(_bits(r['after'][b + s].numpy()), _bits(r['blobs'][b + s].numpy()))
    for p in sorted(body):
        assert not torch.equal(r['after'][p], r['blobs'][p]), p
    _RUNS.pop((name, False), None)


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def frozen_record(dev):
    """Losses (bit patterns) and head gradients (SHA-256 of the float32 bytes) of the frozen-body
    run of both tiny models: what tests/golden/frozen_body_before.json holds, recorded with the
    code as it was before the trainable body existed."""
    out = {}
    for name in sorted(MODELS):
        r = _run(dev, name, True)
        out[name] = dict(
            losses={k: int(np.float32(v).view(np.uint32)) for k, v in sorted(r['losses'].items())},
            grads={p: _digest(g) for p, g in sorted(r['grads'].items())})
        _RUNS.pop((name, True), None)
    return out


def test_frozen_body_run_is_unchanged(dev):
    """TRAIN.FREEZE_CONV_BODY True on the same tiny models: the losses and every head gradient are
    identical, bit for bit, to the values the parent of this change produced."""
    want = json.load(open(FROZEN))
    got = frozen_record(dev)
    for name in sorted(MODELS):
        assert sorted(got[name]['grads']) == sorted(want[name]['grads'])
        assert not [p for p in got[name]['grads'] if p.startswith('conv')]
        assert got[name]['losses'] == want[name]['losses'], name
        diff = [p for p in want[name]['grads'] if got[name]['grads'][p] != want[name]['grads'][p]]
        assert not diff, (name, diff)

