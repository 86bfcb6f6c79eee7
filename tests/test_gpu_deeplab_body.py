"""The DeepLab VGG-16 body on the GPU: naws_maxpool3x3_nhwc_fwd bit for bit against torch's
max_pool2d(x, 3, stride, 1) (pads with -inf, floors: the contract), the op layer, and a tiny
na_wsddn (3 x 50 x 66, 12 rois, 20 classes, dropout off) over the DeepLab and the conv4 body on
both execution plans against the float64 restatement of tests/deeplab_ref.py.

Bounds, the ones the origin body is held to: conv5_3 within 1e-4 of each channel's pre-activation
RMS, losses within 1e-4 (relative), fc8 logits within 1e-5 of max|logit|
(tests/test_gpu_fullsize_oracle.py); the head parameters of the two plans after one step within
2e-3 of the applied update (tests/test_gpu_graph.py test_fused_plan_equals_op_by_op_plan)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deeplab_ref as dref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, 'na-fwebsod_amd', 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
DEEPLAB = 'VGG16.add_VGG16_conv5_body_deeplab'
CONV4 = 'VGG16.add_VGG16_conv4_body_origin'
SHAPES = [(1, 1, 1, 4), (1, 2, 2, 4), (2, 8, 8, 64), (2, 9, 7, 64), (1, 7, 10, 132)]
CH_BOUND, LOSS_BOUND, LOGIT_BOUND = 1e-4, 1e-4, 1e-5


def _pool_ref(x_nhwc, stride):
    return F.max_pool2d(x_nhwc.permute(0, 3, 1, 2), 3, stride, 1).permute(0, 2, 3, 1).contiguous()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                               b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------ pool kernel ----
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('shape', SHAPES)
def test_maxpool3x3_bit_exact(dev, shape, stride):
    from naws_hip import ops
    rng = np.random.default_rng(sum(shape) + stride)
    cases = {'signed': rng.standard_normal(shape).astype(np.float32) * 3.0,
             # every value negative: a maximum that starts at 0 returns 0
             'negative': -np.abs(rng.standard_normal(shape).astype(np.float32)) - 0.5}
    last = -np.abs(rng.standard_normal(shape).astype(np.float32)) - 0.5
    last[:, -1, -1, :] = 7.0        # the maximum in the last row and column: a window clipped one short
    cases['last'] = last
    for name, x in cases.items():
        xt = torch.from_numpy(x)
        want = _pool_ref(xt, stride)
        n, h, w, c = shape
        assert tuple(want.shape) == (n, (h - 1) // stride + 1, (w - 1) // stride + 1, c)
        got = ops.maxpool3x3_nhwc(xt.to(dev), stride)
        assert _same_bits(got.cpu(), want), (name, shape, stride)
        if name == 'negative':
            assert float(got.max()) < 0
        if name == 'last':
            assert bool((got[:, -1, -1, :] == 7.0).all())
        out = torch.full(tuple(want.shape), float('nan'), device=dev)
        ret = ops.maxpool3x3_nhwc(xt.to(dev), stride, out=out)
        assert ret.data_ptr() == out.data_ptr() and _same_bits(out.cpu(), want)
        assert _same_bits(ops.maxpool3x3_nhwc(xt.to(dev), stride).cpu(), want)     # a second call
    with pytest.raises(Exception):
        ops.maxpool3x3_nhwc(torch.zeros(shape, device=dev), 3)
    with pytest.raises(Exception):
        ops.maxpool3x3_nhwc(torch.zeros(shape, device=dev), stride,
                            out=torch.zeros((1, 1, 1, 8), device=dev))


def test_maxpool3x3_grid_stride(dev):
    """More work items than the launch's lanes (4096 workgroups x 256): the grid-stride loop."""
    from naws_hip import ops
    for stride, (h, w) in ((1, (130, 1038)), (2, (258, 2070))):
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        assert ho * ((wo + 3) // 4) * 32 > 4096 * 256 and wo % 4 != 0
        x = torch.randn((1, h, w, 128), generator=torch.Generator().manual_seed(stride))
        assert _same_bits(ops.maxpool3x3_nhwc(x.to(dev), stride).cpu(), _pool_ref(x, stride))


@pytest.mark.parametrize('stride', [1, 2])
def test_op_layer_maxpool(dev, stride):
    import detectron.ops as O
    x = torch.randn((2, 8, 9, 7), generator=torch.Generator().manual_seed(stride))
    got = O.MaxPool(x.to(dev), kernel=3, pad=1, stride=stride)
    assert _same_bits(got.cpu(), F.max_pool2d(x, 3, stride, 1))
    assert _same_bits(O.MaxPool(x.to(dev), kernel=2, pad=0, stride=stride).cpu(),
                      F.max_pool2d(x, 2, stride, 0))
    for k, p, s in ((3, 0, 2), (5, 2, 2), (3, 1, 3)):
        with pytest.raises(O.NawsError):
            O.MaxPool(x.to(dev), kernel=k, pad=p, stride=s)
    y = O.MaxPool(x.to(dev), kernel=3, pad=1, stride=stride)
    with pytest.raises(O.NawsError):
        O.MaxPoolGradient(x.to(dev), y, torch.ones_like(y), kernel=3, pad=1, stride=stride)


# ------------------------------------------------------------------------------- whole model ----
def _executor(dev, body, dilation, train, interpreted=False, plan=None):
    """(model, executor) of the tiny na_wsddn over `body`, loaded with deeplab_ref.inputs()."""
    from detectron.core import config as c
    from detectron.core.executor import NetExecutor
    import detectron.modeling.model_builder_wsl as mbld
    c.reset_cfg()
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', 1, 'TRAIN.FREEZE_CONV_BODY', True, 'MODEL.CONV_BODY', body,
                           'WSL.DILATION', dilation, 'MODEL.NUM_CLASSES', dref.NFG + 1]
                          + (['NAWS.MFMA_DTYPE', plan] if plan else []))
    c.assert_and_infer_cfg(make_immutable=False)
    model = mbld.create('generalized_wsl', train=train)
    ex = NetExecutor(model, dev, disable_dropout=True, force_interpreted=interpreted)
    blobs, _mb = dref.inputs()
    ex.load_blobs({k: v.clone() for k, v in blobs.items()})
    return model, ex


def _step(dev, model, ex, lr=1e-3):
    _blobs, mb = dref.inputs()
    model.UpdateWorkspaceLr(0, lr)
    ex.feed({k: torch.from_numpy(v).to(dev) for k, v in mb.items()})
    ex.run()
    torch.cuda.synchronize()


def _check_values(tag, fmap_nchw, logits, losses, ref):
    ce = dref.channel_error(fmap_nchw, ref['fmap'], ref['rms'])
    le = float(np.abs(logits - ref['logits']).max() / np.abs(ref['logits']).max())
    print('%s: feature map max err / channel RMS %.3g; logits max err / max %.3g' % (tag, ce, le))
    for got, want, name in zip(losses, ref['losses'], ('loss_cls', 'loss_cls_noise')):
        print('   %s: %.7g against %.7g' % (name, got, want))
    assert fmap_nchw.shape == ref['fmap'].shape and ce <= CH_BOUND
    assert le <= LOGIT_BOUND
    for got, want in zip(losses, ref['losses']):
        assert np.isfinite(got) and abs(got - want) <= LOSS_BOUND * abs(want)
    return ce


@pytest.mark.parametrize('dilation', [2, 1])
def test_deeplab_body_op_by_op(dev, cfgmod, dilation):
    ref = dref.reference('deeplab', dilation)
    assert ref['fmap'].shape[2:] == ((7, 9) if dilation == 2 else (4, 5))
    model, ex = _executor(dev, DEEPLAB, dilation, True, interpreted=True)
    assert ex.plan == 'interpreted'
    _step(dev, model, ex)
    fmap = ex.ws['conv5_3'].cpu().numpy()
    logits = np.concatenate([ex.ws[k].cpu().numpy() for k in dref.LOGIT_KEYS], 1)
    losses = [float(ex.ws[l].reshape(-1)[0]) for l in ('loss_cls', 'loss_cls_noise')]
    _check_values('deeplab d%d op-by-op' % dilation, fmap, logits, losses, ref)
    # a deliberately wrong reference (kernel-2 pools) misses the feature-map bound by >= 100 x
    blobs, mb = dref.inputs()
    wrong, wrms = dref.body64(mb['data'], blobs, 'deeplab', dilation, wrong='k2')
    miss = dref.channel_error(fmap, wrong.numpy(), wrms)
    print('   wrong reference (kernel-2 pools): %.3g' % miss)
    assert miss >= 100 * CH_BOUND


def test_conv4_body_op_by_op(dev, cfgmod):
    ref = dref.reference('conv4', 1)
    assert ref['fmap'].shape == (1, 512, 6, 8)
    model, ex = _executor(dev, CONV4, 1, True)
    assert ex.plan == 'interpreted' and ex.engine is None            # unforced
    assert 'conv5_1_w' not in model.params
    _step(dev, model, ex)
    fmap = ex.ws['conv4_3'].cpu().numpy()
    logits = np.concatenate([ex.ws[k].cpu().numpy() for k in dref.LOGIT_KEYS], 1)
    losses = [float(ex.ws[l].reshape(-1)[0]) for l in ('loss_cls', 'loss_cls_noise')]
    _check_values('conv4 op-by-op', fmap, logits, losses, ref)


@pytest.mark.parametrize('plan', ['fp16x2', 'fp32x3', 'fp32'])
@pytest.mark.parametrize('dilation', [2, 1])
def test_deeplab_body_fused(dev, cfgmod, dilation, plan):
    ref = dref.reference('deeplab', dilation)
    model, ex = _executor(dev, DEEPLAB, dilation, True, plan=plan)
    assert ex.plan == 'fused' and ex.engine.body == 'deeplab' and ex.engine.mfma_dtype == plan
    assert ex.engine.spatial_scale == ref['scale']
    eng = ex.engine
    _blobs, mb = dref.inputs()
    t = {k: torch.from_numpy(v).to(dev) for k, v in mb.items()}
    fmap = eng.conv_body(t['data']).permute(0, 3, 1, 2).cpu().numpy()
    out = eng.forward_backward(t['data'], t['rois'], t['obn_scores'], t['labels_oh'])
    c, ld8 = dref.NFG, eng.ld8
    logits = torch.cat([out['logits'].float()[:, o:o + c] for o in (0, c, ld8, ld8 + c)], 1)
    losses = [float(out[k][0]) for k in ('loss_cls', 'loss_cls_noise')]
    _check_values('deeplab d%d fused %s' % (dilation, plan), fmap, logits.cpu().numpy(), losses, ref)


GATED = ('fc6', '_[noisy]_fc6', 'fc7', '_[noisy]_fc7')       # the four ReLU outputs of the head


@pytest.mark.parametrize('plan', ['fp16x2', 'fp32x3', 'fp32'])
@pytest.mark.parametrize('dilation', [2, 1])
def test_deeplab_fused_step_equals_op_by_op_step(dev, cfgmod, dilation, plan):
    """One training step on both plans: every head parameter within 2e-3 of the applied update
    (+ 1e-9), the bound of tests/test_gpu_graph.py test_fused_plan_equals_op_by_op_plan.

    The backward pass is discontinuous in the forward values at a ReLU: a unit whose pre-activation
    is next to zero may come out as 0 in one plan and as a tiny positive number in the other - both
    within the forward bound -, and its gradient then is all or nothing.  At WSL.DILATION 2 these
    inputs have one such unit: _[noisy]_fc7 of roi 0, unit 3063, is 3.4e-7 on the op-by-op plan
    (the other rois of that unit reach 10), and without further care row 3063 of _[noisy]_fc7_w
    alone differs by 0.135 of the largest update (every other row: one fp32 ulp of the parameter),
    on all three plans alike.  So the gates are taken out of the comparison, and nothing else:
      * the fused plan's four ReLU outputs are read first;
      * the op-by-op run is made to take the same side wherever its gate differs, by writing the
        fused plan's value (0 or the tiny number) into its blob right behind the Relu op;
      * every such element must be UNDECIDABLE: its float64 pre-activation within 1e-4 of the
        unit's pre-activation RMS of zero - the per-unit forward bound of
        tests/test_gpu_fullsize_oracle.py; a gate that differs anywhere else fails the test."""
    ref = dref.reference('deeplab', dilation)
    model, ex = _executor(dev, DEEPLAB, dilation, True, plan=plan)
    assert ex.plan == 'fused'
    before = {k: v.clone().cpu() for k, v in ex.blobs(False).items()}
    eng = ex.engine
    _blobs, mb = dref.inputs()
    t = {k: torch.from_numpy(v).to(dev) for k, v in mb.items()}
    h6, h7, _lg = eng.head_forward(eng._roi_features(eng.conv_body(t['data']), t['rois'],
                                                     t['obn_scores']), train=True)
    fused_act = {'fc6': h6[:, :4096], '_[noisy]_fc6': h6[:, 4096:],
                 'fc7': h7[:, :4096], '_[noisy]_fc7': h7[:, 4096:]}
    fused_act = {k: v.float().clone() for k, v in fused_act.items()}
    assert all(tuple(v.shape) == (dref.R, 4096) for v in fused_act.values())
    _step(dev, model, ex)
    m2, interp = _executor(dev, DEEPLAB, dilation, True, interpreted=True, plan=plan)
    fwd, moved, hooked = interp._forward, [], set()

    def same_gates(idx, op, ws):
        fwd(idx, op, ws)
        if op.type == 'Relu' and op.outputs[0] in GATED:
            name = op.outputs[0]
            hooked.add(name)
            mine, theirs = ws[name], fused_act[name]
            flip = (mine > 0) != (theirs > 0)
            for r, u in flip.nonzero().cpu().tolist():
                moved.append((name, r, u, float(mine[r, u]), float(theirs[r, u])))
            ws[name] = torch.where(flip, theirs, mine)
    interp._forward = same_gates
    _step(dev, m2, interp)
    assert hooked == set(GATED)
    for name, r, u, a, b in moved:
        z, rms = float(ref['preact'][name][r, u]), float(ref['preact_rms'][name][u])
        print('d%d %s gate of %s[%d, %d]: op-by-op %.3g, fused %.3g, float64 pre-activation %.3g, '
              'unit RMS %.3g' % (dilation, plan, name, r, u, a, b, z, rms))
        assert abs(z) <= 1e-4 * rms, (name, r, u, z, rms)
    fb, ib = ex.blobs(False), interp.blobs(False)
    assert sorted(model.TrainableParams()) == sorted(m2.TrainableParams())
    worst = {}
    for name in model.TrainableParams():
        a, b = fb[name].cpu().numpy(), ib[name].cpu().numpy()
        upd = np.abs(b - before[name].numpy()).max()
        worst[name] = (float(np.abs(a - b).max()), float(upd))
    for name, (d, upd) in sorted(worst.items(), key=lambda kv: -kv[1][0] / (kv[1][1] + 1e-30))[:6]:
        print('d%d %s %s: max|diff| %.3g, max|update| %.3g' % (dilation, plan, name, d, upd))
    assert torch.equal(fb['conv4_2_w'].cpu(), before['conv4_2_w'])
    for name, (d, upd) in worst.items():
        assert d <= 2e-3 * upd + 1e-9, name


def test_inference_plans_and_the_tta_pair(dev, cfgmod):
    """Inference lands on the fused plan; a plain + mirrored pair (different roi counts after the
    dedup of the mirrored boxes is not needed: the counts are made different here) as ONE batch of
    two images returns the scores of two single calls, bit for bit."""
    from detectron.core import test_wsl
    from detectron.datasets import synthetic
    _m4, ex4 = _executor(dev, CONV4, 1, False)
    assert ex4.plan == 'interpreted'
    del _m4, ex4
    _model, ex = _executor(dev, DEEPLAB, 2, False)
    assert ex.plan == 'fused' and ex.engine.body == 'deeplab'
    from detectron.core import config as c
    c.merge_cfg_from_list(['TEST.SCALE', 50, 'TEST.MAX_SIZE', 200])
    e = synthetic.make_roidb(1, 40, dref.NFG, 50, 66, seed=9)[0]
    im = (synthetic.make_image(e).transpose(1, 2, 0) + synthetic.PIXEL_MEANS_BGR).astype(np.float32)
    # two images with different roi counts in one batch: engine.infer over segments [0, 40, 64]
    data = torch.from_numpy(np.stack([synthetic.make_image(e), synthetic.make_image(e)[:, :, ::-1].copy()]))
    boxes = e['boxes']
    flipped = test_wsl.flip_boxes(boxes, 66)[:24]
    rois = np.vstack([np.hstack([np.zeros((40, 1), np.float32), boxes]),
                      np.hstack([np.ones((24, 1), np.float32), flipped])]).astype(np.float32)
    obn = np.vstack([e['obn_scores'] + 1.0, e['obn_scores'][:24] + 1.0]).astype(np.float32)
    ex.feed(dict(data=data.to(dev), rois=torch.from_numpy(rois).to(dev),
                 obn_scores=torch.from_numpy(obn).to(dev), _seg=[0, 40, 64]))
    ex.run()
    both = ex.fetch('cls_prob').cpu().numpy().reshape(64, -1)
    singles = []
    for b, (lo, hi) in enumerate(((0, 40), (40, 64))):
        r = rois[lo:hi].copy()
        r[:, 0] = 0
        ex.feed(dict(data=data[b:b + 1].to(dev), rois=torch.from_numpy(r).to(dev),
                     obn_scores=torch.from_numpy(obn[lo:hi]).to(dev), _seg=[0, hi - lo]))
        ex.run()
        singles.append(ex.fetch('cls_prob').cpu().numpy().reshape(hi - lo, -1))
    print('pair vs singles: max |diff| %.3g / %.3g' % (np.abs(both[:40] - singles[0]).max(),
                                                       np.abs(both[40:] - singles[1]).max()))
    assert np.isfinite(both).all()
    assert np.array_equal(both[:40], singles[0]) and np.array_equal(both[40:], singles[1])
    # and through the entry point: im_detect_bbox_pair against the two single calls
    p0, p1 = test_wsl.im_detect_bbox_pair(ex, im, 50, 200, boxes, e['obn_scores'])
    q0, _ = test_wsl.im_detect_bbox(ex, im, 50, 200, boxes, e['obn_scores'])
    q1, _ = test_wsl.im_detect_bbox_hflip(ex, im, 50, 200, boxes, e['obn_scores'])
    print('im_detect_bbox_pair vs singles: max |diff| %.3g / %.3g' % (np.abs(p0 - q0).max(),
                                                                      np.abs(p1 - q1).max()))
    assert p0.shape == (40, dref.NFG + 1)
    assert np.array_equal(p0, q0) and np.array_equal(p1, q1)
