"""The ResNet18-WS body on the GPU: naws_conv2d_nhwc_fwd on every layer form of the body against
F.conv2d in float64, naws_affine_channel_fwd bit for bit against a float32 multiply and add, and the
body, one training step of a tiny plain WSDDN over it (3 x 67 x 93, 12 rois, 20 classes, a 256-wide
2-fc head, dropout off) and one test image on the op-by-op plan against the float64 restatement of
tests/resnet_ref.py.

Bounds, the ones the VGG-16 bodies are held to (tests/test_gpu_deeplab_body.py): a layer / the body
within 1e-4 of each output channel's pre-activation RMS, the loss within 1e-4 (relative), the fc8
logits within 1e-5 of max|logit|."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guard
import resnet_ref as rref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, 'na-fwebsod_amd', 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
CONV5, CONV4 = 'ResNet18.add_ResNet18_conv5_body', 'ResNet18.add_ResNet18_conv4_body'
CH_BOUND, LOSS_BOUND, LOGIT_BOUND = 1e-4, 1e-4, 1e-5

# (name, n, h, w, cin, cout, kernel, stride, pad, dilation)
LAYERS = [
    ('stem 7x7 s2, odd sizes, K 147', 1, 67, 93, 3, 64, 7, 2, 3, 1),
    ('stem 7x7 s2, 4 x 4 outputs: M below a tile', 1, 7, 7, 3, 64, 7, 2, 3, 1),
    ('stem 7x7 s2, one output row of 4 pixels', 1, 1, 7, 3, 64, 7, 2, 3, 1),
    ('3x3 s2 p1, odd height', 1, 17, 24, 64, 128, 3, 2, 1, 1),
    ('3x3 s2 p1, odd width', 1, 18, 23, 64, 128, 3, 2, 1, 1),
    ('1x1 s2', 1, 9, 12, 64, 128, 1, 2, 0, 1),
    ('1x1 s1', 1, 9, 12, 256, 512, 1, 1, 0, 1),
    ('3x3 s1 d2 p2 on the new entry', 1, 5, 6, 64, 64, 3, 1, 2, 2),
]


def _layer_inputs(n, h, w, cin, cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.3
    return x, wt, b


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _conv(dev, x, wt, b, k, s, p, d, relu, out=None):
    from naws_hip import ops
    return ops.conv2d_nhwc(_nhwc(x).to(dev), ops.conv2d_pack_weight(wt.to(dev)),
                           None if b is None else b.to(dev), k, s, p, d, relu, out=out)


def _check_layer(tag, got_nhwc, x, wt, b, s, p, d, relu):
    pre = F.conv2d(x.double(), wt.double(), None if b is None else b.double(), s, p, d)
    want = F.relu(pre) if relu else pre
    got = got_nhwc.permute(0, 3, 1, 2).cpu().numpy()
    assert got.shape == tuple(want.shape), (tag, got.shape, tuple(want.shape))
    rms = pre.pow(2).mean(dim=(0, 2, 3)).sqrt().numpy()
    err = rref.channel_error(got, want.numpy(), rms)
    print('%s bias %s relu %s: max err / channel RMS %.3g' % (tag, b is not None, relu, err))
    assert np.isfinite(got).all() and err <= CH_BOUND, (tag, err)
    return err


# ----------------------------------------------------------------------------- single layers ----
@pytest.mark.parametrize('case', LAYERS, ids=[c[0] for c in LAYERS])
def test_conv2d_layer_against_float64(dev, case):
    tag, n, h, w, cin, cout, k, s, p, d = case
    from naws_hip import ops
    x, wt, b = _layer_inputs(n, h, w, cin, cout, k, seed=h * 100 + w + k)
    assert ops.conv2d_out_size(h, w, k, s, p, d) == ((h + 2 * p - d * (k - 1) - 1) // s + 1,
                                                     (w + 2 * p - d * (k - 1) - 1) // s + 1)
    for bias in (None, b):
        for relu in (False, True):
            got = _conv(dev, x, wt, bias, k, s, p, d, relu)
            _check_layer(tag, got, x, wt, bias, s, p, d, relu)
            assert torch.equal(got, _conv(dev, x, wt, bias, k, s, p, d, relu))        # a second call
    if k == 7:
        wp = ops.conv2d_pack_weight(wt.to(dev)).cpu()
        assert wp.shape == (cout, 160) and bool((wp[:, 147:] == 0).all())            # the K padding
        assert torch.equal(wp[:, :147].reshape(cout, 7, 7, 3), wt.permute(0, 2, 3, 1))


def test_op_layer_routes(dev):
    """O.Conv: 3x3 / s1 / d2 / p2, 512 -> 512 on 5 x 6 stays on naws_conv3x3_nhwc_fwd - bit for bit
    what the parent's route gives -; a strided form goes to the new entry; b may be None."""
    import detectron.ops as O
    from naws_hip import ops
    x, wt, b = _layer_inputs(1, 5, 6, 512, 512, 3, seed=11)
    got = O.Conv(x.to(dev), wt.to(dev), b.to(dev), kernel=3, pad=2, stride=1, dilation=2)
    old = ops.nhwc_to_nchw(ops.conv3x3_nhwc(ops.nchw_to_nhwc(x.to(dev)), ops.conv3x3_pack_weight(wt.to(dev)),
                                            b.to(dev), 2, False))
    assert torch.equal(got, old)
    _check_layer('O.Conv 3x3 s1 d2 p2 512', got.permute(0, 2, 3, 1), x, wt, b, 1, 2, 2, False)
    nb = O.Conv(x.to(dev), wt.to(dev), None, kernel=3, pad=2, stride=1, dilation=2)
    _check_layer('O.Conv 3x3 s1 d2 p2 512', nb.permute(0, 2, 3, 1), x, wt, None, 1, 2, 2, False)
    x, wt, b = _layer_inputs(1, 17, 24, 64, 128, 3, seed=12)
    got = O.Conv(x.to(dev), wt.to(dev), None, kernel=3, pad=1, stride=2)
    assert tuple(got.shape) == (1, 128, 9, 12)
    _check_layer('O.Conv 3x3 s2 p1', got.permute(0, 2, 3, 1), x, wt, None, 2, 1, 1, False)
    with pytest.raises(O.NawsError):
        O.ConvGradient(x.to(dev), wt.to(dev), got, kernel=3, pad=1, stride=2)
    for kw in (dict(kernel=5, pad=2), dict(kernel=3, pad=1, stride=3), dict(kernel=3, pad=5)):
        with pytest.raises(O.NawsError):
            O.Conv(x.to(dev), torch.zeros((128, 64, kw['kernel'], kw['kernel']), device=dev), None, **kw)


def _int_inputs(n, cin, cout, k, h, w, seed):
    """Integers (x, weight in [-4, 4], bias in [-64, 64]): every partial sum of a convolution of
    K <= 49 * 32 stays an integer below 2^24, so fp32 in any order gives the float64 result."""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.integers(-4, 5, (n, cin, h, w)).astype(np.float32))
    wt = torch.from_numpy(rng.integers(-4, 5, (cout, cin, k, k)).astype(np.float32))
    b = torch.from_numpy(rng.integers(-64, 65, (cout,)).astype(np.float32))
    return x, wt, b


@pytest.mark.parametrize('k,s,d', [(k, s, d) for k in (1, 3, 7) for s in (1, 2) for d in (1, 2)])
def test_op_conv_domain_exact(dev, k, s, d):
    """O.Conv, NCHW, N = 2 on 9 x 11 (15 x 17 where the window is wider than 9): kernel x stride x
    dilation at the natural pad dilation * (kernel - 1) / 2 and at pad 0, Cin 3 and 32, bias or None,
    ReLU or not - both routes and the seam between them - EQUAL to F.conv2d in float64 (integer
    inputs).  Every row is run before the failures are reported."""
    import detectron.ops as O
    span, failed = d * (k - 1) + 1, []
    for p in sorted({d * (k - 1) // 2, 0}):
        h, w = (9, 11) if span - 2 * p <= 9 else (span - 2 * p + 2, span - 2 * p + 4)
        for cin in (3, 32):
            x, wt, b = _int_inputs(2, cin, 32, k, h, w, seed=1000 * k + 100 * s + 10 * d + p + cin)
            pre = F.conv2d(x.double(), wt.double(), None, s, p, d)
            for bias in (b, None):
                y = pre if bias is None else pre + b.double().view(1, -1, 1, 1)
                assert float(y.abs().max()) < 2 ** 24
                for relu in (False, True):
                    want = y.relu() if relu else y
                    assert not relu or (bool((want == 0).any()) and bool((want > 0).any()))
                    row = 'cin %d kernel %d stride %d pad %d dilation %d bias %s relu %s' % (
                        cin, k, s, p, d, bias is not None, relu)
                    try:
                        got = O.Conv(x.to(dev), wt.to(dev), None if bias is None else bias.to(dev),
                                     kernel=k, pad=p, stride=s, dilation=d, relu=relu)
                    except O.NawsError as e:
                        failed.append('%s: %s' % (row, e))
                        continue
                    assert tuple(got.shape) == tuple(want.shape), row
                    if not torch.equal(got.double().cpu(), want):
                        failed.append('%s: %d of %d values differ' % (
                            row, int((got.double().cpu() != want).sum()), want.numel()))
    assert not failed, '\n'.join(failed)


def test_op_conv_seam(dev):
    """What the 3x3 / stride 1 / pad == dilation route served correctly keeps that route, bit for
    bit: Cin 3 at dilation 1 is conv3x3_c3_nchw_to_nhwc (Cout 16: a width only that entry takes);
    bias None with ReLU stays on naws_conv3x3_nhwc_fwd (Cout 36: % 4, not % 32) and is max(conv, 0).
    A weight that does not match (Cin, kernel, kernel) is ERR_SHAPE on both routes."""
    import detectron.ops as O
    from naws_hip import lib, ops
    x, wt, b = _layer_inputs(2, 9, 11, 3, 16, 3, seed=21)
    for bias in (b.to(dev), None):
        for relu in (False, True):
            got = O.Conv(x.to(dev), wt.to(dev), bias, kernel=3, pad=1, relu=relu)
            old = ops.nhwc_to_nchw(ops.conv3x3_c3_nchw_to_nhwc(x.to(dev), wt.to(dev), bias, relu))
            assert torch.equal(got, old)
            _check_layer('O.Conv 3x3 s1 p1 cin 3', got.permute(0, 2, 3, 1), x, wt,
                         None if bias is None else b, 1, 1, 1, relu)
    x, wt, b = _layer_inputs(2, 9, 11, 32, 36, 3, seed=22)
    for dil in (1, 2):
        conv = O.Conv(x.to(dev), wt.to(dev), None, kernel=3, pad=dil, dilation=dil)
        got = O.Conv(x.to(dev), wt.to(dev), None, kernel=3, pad=dil, dilation=dil, relu=True)
        assert torch.equal(got, torch.clamp(conv, min=0)) and bool((got == 0).any())
        _check_layer('O.Conv 3x3 s1 cout 36', got.permute(0, 2, 3, 1), x, wt, None, 1, dil, dil, True)
    x = torch.zeros((1, 32, 9, 11), device=dev)
    for kw in (dict(kernel=3, pad=1), dict(kernel=3, pad=2, dilation=2),              # the old route
               dict(kernel=3, pad=1, stride=2), dict(kernel=1, pad=0)):               # the new one
        k = kw['kernel']
        for shape in ((32, 64, k, k), (32, 32, k + 2, k + 2), (32, 32, k, k + 2), (32, 32, k)):
            with pytest.raises(O.NawsError) as e:
                O.Conv(x, torch.zeros(shape, device=dev), None, **kw)
            assert e.value.code == lib.ERR_SHAPE, (kw, shape)
    with pytest.raises(O.NawsError) as e:                                             # Cin 3
        O.Conv(x[:, :3].contiguous(), torch.zeros((32, 32, 3, 3), device=dev), None, kernel=3, pad=1)
    assert e.value.code == lib.ERR_SHAPE


@pytest.mark.parametrize('case', [LAYERS[0], LAYERS[3], LAYERS[5]], ids=['7x7', '3x3s2', '1x1s2'])
def test_images_do_not_mix(dev, case):
    """N = 2, image 1 all zeros but one pixel of 100 (inputs are N(0, 1)) at the top-left corner -
    the tap a window of image 0's last row would reach if it ran on into the next image: image 0's
    output is, bit for bit, what it is alone, and both images are within the bound."""
    tag, _n, h, w, cin, cout, k, s, p, d = case
    x, wt, b = _layer_inputs(2, h, w, cin, cout, k, seed=5)
    x[1] = 0
    x[1, :, 0, 0] = 100.0
    both = _conv(dev, x, wt, b, k, s, p, d, False)
    alone = _conv(dev, x[:1], wt, b, k, s, p, d, False)
    assert torch.equal(both[0], alone[0])
    assert float(both[0].abs().max()) < 30 < float(both[1].abs().max())
    _check_layer(tag + ', two images', both, x, wt, b, s, p, d, False)


def test_conv2d_grid_stride(dev):
    """More 64-pixel tiles than the launch has workgroups along M: the grid-stride loop."""
    from naws_hip import lib
    cap = int(lib.load().naws_conv2d_max_grid_m())
    h = w = 258
    assert (h * w + 63) // 64 > cap and (h * w) % 64 != 0
    x, wt, b = _layer_inputs(1, h, w, 32, 32, 1, seed=3)
    got = _conv(dev, x, wt, b, 1, 1, 0, 1, True)
    _check_layer('1x1 s1 32 -> 32 on 258 x 258', got, x, wt, b, 1, 0, 1, True)


@pytest.mark.parametrize('case', [LAYERS[0], LAYERS[4]], ids=['7x7', '3x3s2'])
def test_conv2d_guard_bands(dev, case):
    """Y carved from a sentinel-filled buffer, X inside poison: nothing around Y is written and no
    NaN from around X reaches the result; a strided view is refused."""
    from naws_hip import ops
    tag, n, h, w, cin, cout, k, s, p, d = case
    x, wt, b = _layer_inputs(n, h, w, cin, cout, k, seed=9)
    gx = guard.place(_nhwc(x).to(dev))
    ho, wo = ops.conv2d_out_size(h, w, k, s, p, d)
    gy = guard.carve((n, ho, wo, cout), torch.float32, dev)
    wp = ops.conv2d_pack_weight(wt.to(dev))
    ret = ops.conv2d_nhwc(gx.t, wp, b.to(dev), k, s, p, d, True, out=gy.t)
    torch.cuda.synchronize()
    assert ret.data_ptr() == gy.t.data_ptr()
    _check_layer(tag + ', guarded', gy.t, x, wt, b, s, p, d, True)
    gy.check('out')
    gx.check('x')
    view = _nhwc(x).to(dev)[:, :, ::2, :]
    with pytest.raises(ValueError):
        ops.conv2d_nhwc(view, wp, None, k, s, p, d)
    with pytest.raises(ops.L.NawsError):
        ops.conv2d_nhwc(gx.t, wp, None, k, s, p, d, out=torch.zeros((n, ho, wo + 1, cout), device=dev))


# ----------------------------------------------------------------------------- AffineChannel ----
@pytest.mark.parametrize('shape', [(2, 64, 5, 7), (1, 3, 1, 1), (2, 5, 3, 3), (1, 64, 34, 47)])
def test_affine_channel_bit_exact(dev, shape):
    """Bit-equal to a float32 multiply followed by a float32 add; H * W no multiple of 4; in place;
    ReLU; guard bands around Y; tensors off 16 bytes."""
    from naws_hip import ops
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g) * 3
    s = torch.rand((shape[1],), generator=g) + 0.5
    b = torch.rand((shape[1],), generator=g) - 0.5
    assert (shape[2] * shape[3]) % 4 != 0
    prod = x * s.view(1, -1, 1, 1)
    want = prod + b.view(1, -1, 1, 1)
    got = ops.affine_channel(x.to(dev), s.to(dev), b.to(dev))
    assert guard.same_bits(got.cpu(), want)
    assert guard.same_bits(ops.affine_channel(x.to(dev), s.to(dev), b.to(dev), relu=True).cpu(),
                           torch.clamp(want, min=0))
    xi = x.to(dev)
    ret = ops.affine_channel(xi, s.to(dev), b.to(dev), out=xi)                        # in place
    assert ret.data_ptr() == xi.data_ptr() and guard.same_bits(xi.cpu(), want)
    for aligned in (True, False):
        gx = guard.place(x.to(dev)) if aligned else None
        gy = guard.carve(shape, torch.float32, dev, aligned=aligned)
        ops.affine_channel(gx.t if aligned else x.to(dev), s.to(dev), b.to(dev), out=gy.t)
        torch.cuda.synchronize()
        assert guard.same_bits(gy.t.cpu(), want)
        gy.check('out')
        if aligned:
            gx.check('x')
    view = torch.cat([x, x], 1).to(dev)[:, ::2]                     # every other channel: a strided view
    assert not view.is_contiguous()
    with pytest.raises(ValueError):
        ops.affine_channel(view, s.to(dev), b.to(dev))
    import detectron.ops as O
    assert guard.same_bits(O.AffineChannel(x.to(dev), s.to(dev), b.to(dev)).cpu(), want)


# -------------------------------------------------------------------------------- whole body ----
def _cfg(body, dilation, extra=()):
    from detectron.core import config as c
    c.reset_cfg()
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', 1, 'WEBLY.WEBLY_ON', False, 'TRAIN.FREEZE_CONV_BODY', True,
                           'MODEL.CONV_BODY', body, 'RESNETS.TRANS_FUNC', 'residual_transformation',
                           'RESNETS.RES5_DILATION', dilation, 'FAST_RCNN.ROI_BOX_HEAD',
                           'wsl_heads.add_ResNet_roi_2fc_head', 'FAST_RCNN.MLP_HEAD_DIM', rref.HIDDEN,
                           'MODEL.NUM_CLASSES', rref.NFG + 1] + list(extra))
    c.assert_and_infer_cfg(make_immutable=False)
    return c


def _body_only(dev, body, dilation):
    """The body's feature map from the op-by-op plan (a model of the body's ops alone)."""
    from detectron.core.executor import NetExecutor
    from detectron.modeling import ResNet18
    from detectron.modeling.detector import DetectionModelHelper
    _cfg(body, dilation)
    m = DetectionModelHelper(name='body', train=False, num_classes=rref.NFG + 1)
    blob, dim, scale = getattr(ResNet18, body.split('.')[1])(m)
    ex = NetExecutor(m, dev)
    assert ex.plan == 'interpreted' and ex.engine is None
    blobs, mb = rref.inputs()
    ex.load_blobs({k: v.clone() for k, v in blobs.items() if k in m.params})
    ex.feed({'data': torch.from_numpy(mb['data']).to(dev)})
    ex.run()
    torch.cuda.synchronize()
    return ex.ws[blob].cpu().numpy(), dim, scale


@pytest.mark.parametrize('body,dilation,shape', [(CONV5, 1, (1, 512, 3, 3)), (CONV5, 2, (1, 512, 5, 6)),
                                                 (CONV4, 1, (1, 256, 5, 6))])
def test_body_against_float64(dev, cfgmod, body, dilation, shape):
    kind = 'conv4' if body == CONV4 else 'conv5'
    ref = rref.reference(kind, dilation)
    fmap, dim, scale = _body_only(dev, body, dilation)
    assert fmap.shape == shape == ref['fmap'].shape and dim == shape[1] and scale == ref['scale']
    ce = rref.channel_error(fmap, ref['fmap'], ref['rms'])
    print('%s d%d: feature map max err / channel RMS %.3g' % (kind, dilation, ce))
    assert ce <= CH_BOUND
    blobs, mb = rref.inputs()
    for wrong in ('pad0', 'sc_affine', 'res2'):
        bad, brms = rref.body64(mb['data'], blobs, kind, dilation, wrong=wrong)
        miss = rref.channel_error(fmap, bad.numpy(), brms)
        print('   wrong reference %s: %.3g' % (wrong, miss))
        assert miss >= 100 * CH_BOUND, wrong


def _executor(dev, train, extra=(), more_blobs=None):
    from detectron.core.executor import NetExecutor
    import detectron.modeling.model_builder_wsl as mbld
    _cfg(CONV5, 1, extra)
    model = mbld.create('generalized_wsl', train=train)
    ex = NetExecutor(model, dev, disable_dropout=True)
    assert ex.plan == 'interpreted' and ex.engine is None              # unforced
    blobs, _mb = rref.inputs()
    blobs = dict(blobs, **(more_blobs or {}))
    assert sorted(model.params) == sorted(blobs)
    ex.load_blobs({k: v.clone() for k, v in blobs.items()})
    return model, ex


def _step(dev, model, ex, lr=1e-3):
    _blobs, mb = rref.inputs()
    model.UpdateWorkspaceLr(0, lr)
    ex.feed({k: torch.from_numpy(v).to(dev) for k, v in mb.items()})
    ex.run()
    torch.cuda.synchronize()


def test_training_step_of_plain_wsddn(dev, cfgmod):
    from detectron.core.config import cfg
    model, ex = _executor(dev, True)
    ref = rref.reference('conv5', 1, bool(cfg.WSL.MEAN_LOSS))
    blobs, _mb = rref.inputs()
    body = [n for n, _s in rref.golden()['conv5_d1_train']['params']]
    assert not set(body) & set(model.TrainableParams())
    _step(dev, model, ex)
    fmap = ex.ws['res5_1_sum'].cpu().numpy()
    ce = rref.channel_error(fmap, ref['fmap'], ref['rms'])
    logits = np.concatenate([ex.ws[k].cpu().numpy() for k in ('fc8c', 'fc8d')], 1)
    le = float(np.abs(logits - ref['logits']).max() / np.abs(ref['logits']).max())
    loss = float(ex.ws['loss_cls'].reshape(-1)[0])
    print('feature map %.3g; logits max err / max %.3g; loss_cls %.7g against %.7g' % (
        ce, le, loss, ref['loss']))
    assert ce <= CH_BOUND and le <= LOGIT_BOUND
    assert np.isfinite(loss) and abs(loss - ref['loss']) <= LOSS_BOUND * abs(ref['loss'])
    after = ex.blobs(False)
    for n in body:
        assert guard.same_bits(after[n].cpu(), blobs[n]), n
    # (fc8d_b is left out: the detection softmax runs over the rois, a per-class constant added to
    # every roi cancels in it, so that bias has a zero gradient by construction)
    for n in ('fc6_w', 'fc6_b', 'fc7_w', 'fc7_b', 'fc8c_w', 'fc8c_b', 'fc8d_w'):
        assert not torch.equal(after[n].cpu(), blobs[n]), n


def test_training_step_with_oicr(dev, cfgmod):
    g = torch.Generator().manual_seed(2)
    more = {}
    for k in (1, 2, 3):
        more['cls_score%d_w' % k] = torch.randn((rref.NFG + 1, rref.HIDDEN), generator=g) * 0.01
        more['cls_score%d_b' % k] = torch.zeros((rref.NFG + 1,))
    model, ex = _executor(dev, True, extra=['WSL.OICR', True], more_blobs=more)
    _step(dev, model, ex)
    assert model.losses == ['loss_cls', 'loss_cls1', 'loss_cls2', 'loss_cls3']
    for l in model.losses:
        v = float(ex.ws[l].reshape(-1)[0])
        print(l, v)
        assert np.isfinite(v) and v > 0
    assert not torch.equal(ex.blobs(False)['cls_score1_w'].cpu(), more['cls_score1_w'])


def test_one_image_through_im_detect_all(dev, cfgmod):
    """The test-mode model through core/test_wsl.py as it is.  A score is a product of two
    softmax entries; fc8 logits off by at most e = LOGIT_BOUND * max|logit| move a softmax entry by
    a factor within exp(+-2e), the product by one within exp(+-4e): |score - float64| <= (exp(4e) -
    1) * float64 score, plus one float32 rounding of the score."""
    from detectron.core import test_wsl
    from detectron.datasets import synthetic
    model, ex = _executor(dev, False, extra=['TEST.SCALE', rref.H, 'TEST.MAX_SIZE', 200,
                                             'TEST.SCORE_THRESH', 0.0, 'TEST.DETECTIONS_PER_IM', 30])
    e = synthetic.make_roidb(1, rref.R, rref.NFG, rref.H, rref.W, seed=5)[0]
    im = np.rint(synthetic.make_image(e).transpose(1, 2, 0) + synthetic.PIXEL_MEANS_BGR).astype(np.uint8)
    scores, boxes = test_wsl.im_detect_bbox(ex, im, rref.H, 200, e['boxes'], e['obn_scores'])
    assert scores.shape == (rref.R, rref.NFG + 1) and boxes.shape == (rref.R, 4 * (rref.NFG + 1))
    blobs, mb = rref.inputs()
    data = ex.ws['data'].cpu().numpy()                  # the image blob the network saw
    assert data.shape == mb['data'].shape
    fmap, _rms = rref.body64(data, blobs, 'conv5', 1)
    # the rois the network saw: projected at scale 1, then deduplicated on the DEDUP_BOXES grid (the
    # detection softmax runs over the unique ones; every proposal gets its representative's scores)
    from detectron.core.config import cfg
    rois, index, inv = test_wsl.dedup_rois(test_wsl.project_rois(e['boxes'], 1.0), cfg.DEDUP_BOXES)
    assert np.array_equal(ex.ws['rois'].cpu().numpy(), rois) and len(index) <= rref.R
    mb = dict(mb, rois=rois.astype(np.float32),
              obn_scores=(e['obn_scores'] + 1.0).astype(np.float32)[index, :])
    want = rref.head64(fmap, 1.0 / 32.0, blobs, mb, False)
    want['rois_pred'] = want['rois_pred'][inv, :]
    eps = LOGIT_BOUND * np.abs(want['logits']).max()
    err = np.abs(scores[:, 1:] - want['rois_pred'])
    tol = (np.exp(4 * eps) - 1 + 2.0 ** -23) * want['rois_pred']
    print('scores: max err %.3g, max score %.3g, worst err / tolerance %.3g' % (
        err.max(), want['rois_pred'].max(), (err / tol).max()))
    assert (err <= tol).all() and np.array_equal(scores[:, 0], scores[:, 1])
    cls_boxes = test_wsl.im_detect_all(ex, im, e['boxes'], e['obn_scores'])
    assert len(cls_boxes) == rref.NFG + 1
    n_det = sum(len(b) for b in cls_boxes[1:])
    assert 0 < n_det <= 30
    for j in range(1, rref.NFG + 1):
        for det in cls_boxes[j]:
            assert det[4] in scores[:, j]
