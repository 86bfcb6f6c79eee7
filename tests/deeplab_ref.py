"""float64 restatement (torch CPU double) of na_wsddn over the DeepLab VGG-16 body and over the
conv4 body - a helper module of tests/test_gpu_deeplab_body.py, forward only (both bodies run
frozen there).

  body64        conv2d / relu / max_pool2d: the DeepLab body pools with (3, stride, 1) - torch pads
                with -inf and floors, the contract of naws_maxpool3x3_nhwc_fwd -, the conv4 body
                with (2, 2, 0) and stops after conv4_3.  Also returns the per-channel RMS of the last
                layer's PRE-activation: the yardstick of the per-channel bound
                (tests/test_gpu_fullsize_oracle.py _region_relmax).  `wrong` makes a deliberately
                wrong body: 'k2' takes the stride-2 pools with kernel 2 / pad 0 (ceil sizes, so
                the shapes still agree).
  reference     body64 -> RoIPoolF (the bins' argmax from the CPU oracle on the map rounded to
                float32, the values gathered from the float64 map) x boost -> the two 2-fc branches,
                fc8, WSDDN outputs and both weighted cross entropies in float64
                (oracle.head_float64; the entropy-gate weights are StopGradient constants taken from
                the oracle's fp32 loss tail, as tests/test_gpu_fullsize_oracle.py takes them).
Everything is computed once per (body, dilation) and shared; callers must not modify it."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

NFG = 20
H, W, R = 50, 66, 12            # levels 50/25/13/7 and 66/33/17/9: even, odd, odd, odd
LOGIT_KEYS = ('fc8c', 'fc8d', 'noisy_fc8c', 'noisy_fc8d')
_BLOCKS = ((1, 2), (2, 2), (3, 3), (4, 3))


@functools.lru_cache(maxsize=None)
def inputs():
    """(blobs, minibatch): seeded Kaiming weights with non-zero conv biases, one 3 x 50 x 66 image,
    12 proposals, 20 classes."""
    from detectron.datasets import synthetic
    blobs = synthetic.init_blobs(NFG, seed=3)
    g = torch.Generator().manual_seed(5)
    for k in list(blobs):
        if k.endswith('_b') and k.startswith('conv'):
            blobs[k] = torch.randn(blobs[k].shape, generator=g) * 0.05
    mb = synthetic.make_minibatch(synthetic.make_roidb(1, R, NFG, H, W, seed=5), NFG)
    assert mb['data'].shape == (1, 3, H, W) and mb['rois'].shape == (R, 5)
    return blobs, mb


def body64(data, blobs, body, dilation, wrong=None):
    """-> (feature map NCHW float64, per-channel RMS of its pre-activation)."""
    x = torch.as_tensor(data).double()
    dil5 = 2 if dilation == 2 else 1
    layers = [('conv%d_%d' % (i, j), 1) for i, n in _BLOCKS for j in range(1, n + 1)]

    def pool(x, idx):
        if body == 'conv4':
            return F.max_pool2d(x, 2, 2, 0)
        stride = 1 if idx == 4 and dilation == 2 else 2
        if wrong == 'k2' and stride == 2:
            return F.max_pool2d(x, 2, 2, 0, ceil_mode=True)
        return F.max_pool2d(x, 3, stride, 1)

    rms = None
    for name, d in layers + ([] if body == 'conv4' else [('conv5_%d' % j, dil5) for j in (1, 2, 3)]):
        i, j = int(name[4]), int(name[6])
        if j == 1 and i > 1:
            x = pool(x, i - 1)
        x = F.conv2d(x, blobs[name + '_w'].double(), blobs[name + '_b'].double(), stride=1,
                     padding=d, dilation=d)
        rms = x.pow(2).mean(dim=(0, 2, 3)).sqrt().numpy()
        x = F.relu(x)
    return x, rms


def roi_feat64(fmap, rois, obn_scores, scale):
    """RoIPoolF (7 x 7) x RoIFeatureBoost of a float64 NCHW map -> [R, C, 7, 7] float64."""
    from oracle import oracle
    m = fmap.numpy()
    _, am = oracle.roi_pool_f(m.astype(np.float32), rois, 7, 7, scale)
    n, c, h, w = m.shape
    src = m.reshape(n, c, h * w)[rois[:, 0].astype(np.int64)]
    got = np.take_along_axis(src, np.maximum(am, 0).reshape(len(rois), c, 49).astype(np.int64), 2)
    got = got.reshape(am.shape)
    got[am < 0] = 0.0
    return got * obn_scores.reshape(-1, 1, 1, 1).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(body, dilation):
    """dict(fmap [1,512,h,w], rms [512], scale, logits [R, 4C], losses (loss_cls, loss_cls_noise),
    cls_prob [C], preact / preact_rms: the pre-activations [R, 4096] of fc6, _[noisy]_fc6, fc7,
    _[noisy]_fc7 and their per-unit RMS) in float64."""
    from oracle import oracle
    blobs, mb = inputs()
    fmap, rms = body64(mb['data'], blobs, body, dilation)
    scale = 1.0 / 16.0 if (body == 'deeplab' and dilation != 2) else 1.0 / 8.0
    feat = roi_feat64(fmap, mb['rois'], mb['obn_scores'], scale)
    x32 = feat.reshape(R, -1).astype(np.float32)
    act = oracle.head_forward(torch.from_numpy(x32), blobs, {}, train=False)
    tail = oracle.loss_tail({k: act[k].numpy() for k in LOGIT_KEYS}, mb['rois'], mb['labels_oh'][0])
    cw = [(tail['class_weight'], tail['class_weight_noise'])]
    arb = oracle.head_float64(feat, mb['rois'], mb['labels_oh'], blobs, {}, cw, train=False)
    # the pre-activations of the four ReLUs of the head and each unit's RMS over the rois
    preact = {}
    x64 = torch.from_numpy(feat.reshape(R, -1))
    for pre in ('', '_[noisy]_'):
        z6 = F.linear(x64, blobs[pre + 'fc6_w'].double(), blobs[pre + 'fc6_b'].double())
        z7 = F.linear(F.relu(z6), blobs[pre + 'fc7_w'].double(), blobs[pre + 'fc7_b'].double())
        preact[pre + 'fc6'], preact[pre + 'fc7'] = z6.numpy(), z7.numpy()
    prms = {k: np.sqrt((v ** 2).mean(0)) for k, v in preact.items()}
    return dict(preact=preact, preact_rms=prms, fmap=fmap.numpy(), rms=rms, scale=scale,
                logits=arb['logits'], losses=tuple(arb['losses'][0]), cls_prob=arb['cls_prob'][0])


def channel_error(got_nchw, want, rms):
    """max over the channels of (max error of the channel / RMS of its pre-activation)."""
    err = np.abs(np.asarray(got_nchw, np.float64) - want).max(axis=(0, 2, 3))
    live = rms > 0
    assert live.sum() > 0.9 * live.size
    return float((err[live] / rms[live]).max())
