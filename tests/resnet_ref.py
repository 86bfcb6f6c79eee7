"""float64 restatement (torch CPU double) of the ResNet18-WS body and of the plain WSDDN over it - a
helper module of tests/test_resnet18_body_graph.py and tests/test_gpu_resnet18_body.py, forward only
(the body runs frozen).

  inputs        seeded blobs for the parameter list the reference's builders recorded
                (tests/golden/reference_resnet18_body.json): convs MSRA-filled (conv1 scaled by 1/64
                for +-128 pixels), AffineChannel scales in [0.5, 1.5] and shifts in [-0.5, 0.5] - so
                an omitted affine shows -, a HIDDEN-wide 2-fc head; one 3 x 67 x 93 image (maps
                34 x 47, 17 x 24, 9 x 12, 5 x 6, 3 x 3: odd and even at every level), 12 proposals,
                20 classes.
  body64        F.conv2d / F.max_pool2d / affine / sum / relu in float64, written from the layer
                shapes (not through the project's builders) -> (feature map, per-channel RMS of the
                last PRE-activation, the yardstick of the per-channel bound).  `wrong` makes a
                deliberately wrong body, every one of the same output shape:
                  'pad0'       the stride-2 convs index their taps without the `- pad` (the window
                               starts at yo * stride: the padding all sits at the far edge)
                  'sc_affine'  the 1x1 shortcuts without their AffineChannel
                  'res2'       the stride applied in res2_0 (identity shortcut subsampled) instead of
                               res3_0
  reference     body64 -> RoIPoolF x boost (deeplab_ref.roi_feat64) -> fc6 / fc7 / fc8c / fc8d, the
                WSDDN product, the image-level cross entropy, in float64.
Everything is computed once and shared; callers must not modify it."""
import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NFG = 20
H, W, R = 67, 93, 12
HIDDEN = 256
STAGES = ((2, 64), (3, 128), (4, 256), (5, 512))


def golden():
    return json.load(open(os.path.join(ROOT, 'tests', 'golden', 'reference_resnet18_body.json')))


@functools.lru_cache(maxsize=None)
def inputs():
    """(blobs, minibatch): every parameter of the conv5 body and of the 2-fc head + fc8c / fc8d."""
    from detectron.datasets import synthetic
    g = torch.Generator().manual_seed(7)
    blobs = {}
    for name, shape in golden()['conv5_d1_train']['params']:
        if name.endswith('_w'):
            fan_out = shape[0] * shape[2] * shape[3]
            blobs[name] = torch.randn(shape, generator=g) * (2.0 / fan_out) ** 0.5
            if name == 'conv1_w':
                blobs[name] = blobs[name] / 64.0
        elif name.endswith('_s'):
            blobs[name] = torch.rand(shape, generator=g) + 0.5
        else:
            blobs[name] = torch.rand(shape, generator=g) - 0.5
    k6 = 512 * 7 * 7
    for name, shape, std in (('fc6', (HIDDEN, k6), (2.0 / k6) ** 0.5),
                             ('fc7', (HIDDEN, HIDDEN), (2.0 / HIDDEN) ** 0.5),
                             ('fc8c', (NFG, HIDDEN), (1.0 / HIDDEN) ** 0.5),
                             ('fc8d', (NFG, HIDDEN), (1.0 / HIDDEN) ** 0.5)):
        blobs[name + '_w'] = torch.randn(shape, generator=g) * std
        blobs[name + '_b'] = torch.randn((shape[0],), generator=g) * 0.05
    mb = synthetic.make_minibatch(synthetic.make_roidb(1, R, NFG, H, W, seed=5), NFG)
    assert mb['data'].shape == (1, 3, H, W) and mb['rois'].shape == (R, 5)
    return blobs, mb


def conv64(x, w, stride=1, pad=0, dilation=1, shifted=False):
    """F.conv2d in float64; shifted: the window of output yo starts at yo * stride (no `- pad`),
    the output size unchanged."""
    w = torch.as_tensor(w).double()
    if shifted and pad:
        return F.conv2d(F.pad(x, (0, 2 * pad, 0, 2 * pad)), w, None, stride, 0, dilation)
    return F.conv2d(x, w, None, stride, pad, dilation)


def affine64(x, blobs, name):
    return x * blobs[name + '_s'].double().view(1, -1, 1, 1) + blobs[name + '_b'].double().view(1, -1, 1, 1)


def body64(data, blobs, body='conv5', dilation=1, wrong=None):
    """-> (feature map NCHW float64, per-channel RMS of the last sum before its ReLU)."""
    x = torch.as_tensor(data).double()
    bad_pad = wrong == 'pad0'
    x = conv64(x, blobs['conv1_w'], 2, 3, shifted=bad_pad)
    x = F.relu(affine64(x, blobs, 'res_conv1_bn'))
    x = F.max_pool2d(x, 3, 2, 1)
    dim_in, rms = 64, None
    for stage, dim_out in STAGES[:3 if body == 'conv4' else 4]:
        d = dilation if stage == 5 else 1
        for blk in (0, 1):
            p = 'res%d_%d' % (stage, blk)
            stride = 2 if (dim_in != dim_out and stage != 2 and d == 1) else 1
            if wrong == 'res2' and blk == 0 and stage in (2, 3):
                stride = 2 if stage == 2 else 1
            t = conv64(x, blobs[p + '_branch2a_w'], stride, d, d, shifted=bad_pad and stride == 2)
            t = F.relu(affine64(t, blobs, p + '_branch2a_bn'))
            t = affine64(conv64(t, blobs[p + '_branch2b_w'], 1, d, d), blobs, p + '_branch2b_bn')
            if dim_in != dim_out:
                sc = conv64(x, blobs[p + '_branch1_w'], stride, 0)
                if wrong != 'sc_affine':
                    sc = affine64(sc, blobs, p + '_branch1_bn')
            else:
                sc = x[:, :, ::stride, ::stride]
            x = t + sc
            rms = x.pow(2).mean(dim=(0, 2, 3)).sqrt().numpy()
            x = F.relu(x)
            dim_in = dim_out
    return x, rms


def scale_of(body, dilation):
    return 1.0 / 16.0 if body == 'conv4' else dilation / 32.0


def head64(fmap, scale, blobs, mb, is_mean):
    """-> dict(logits [R, 2C] = fc8c | fc8d, rois_pred [R, C], cls_prob [C], loss) in float64."""
    import deeplab_ref as dref
    feat = dref.roi_feat64(fmap, mb['rois'], mb['obn_scores'], scale)
    x = torch.from_numpy(feat.reshape(feat.shape[0], -1))
    lin = lambda v, n: F.linear(v, blobs[n + '_w'].double(), blobs[n + '_b'].double())
    h = F.relu(lin(F.relu(lin(x, 'fc6')), 'fc7'))
    zc, zd = lin(h, 'fc8c'), lin(h, 'fc8d')
    pred = torch.softmax(zc, 1) * torch.softmax(zd, 0)
    p = pred.sum(0)
    lab = torch.from_numpy(mb['labels_oh'][0]).double()
    ce = -(lab * torch.log(p) + (1 - lab) * torch.log(1 - p)).sum() / (float(lab.numel()) if is_mean
                                                                      else 1.0)
    return dict(logits=torch.cat([zc, zd], 1).numpy(), rois_pred=pred.numpy(), cls_prob=p.numpy(),
                loss=float(ce))


@functools.lru_cache(maxsize=None)
def reference(body, dilation, is_mean=False):
    blobs, mb = inputs()
    fmap, rms = body64(mb['data'], blobs, body, dilation)
    out = dict(fmap=fmap.numpy(), rms=rms, scale=scale_of(body, dilation))
    if body == 'conv5':
        out.update(head64(fmap, out['scale'], blobs, mb, is_mean))
    return out


def channel_error(got_nchw, want, rms):
    """max over the channels of (max error of the channel / RMS of its pre-activation)."""
    err = np.abs(np.asarray(got_nchw, np.float64) - want).max(axis=(0, 2, 3))
    live = rms > 0
    assert live.sum() > 0.9 * live.size
    return float((err[live] / rms[live]).max())


def layer_error(got_nchw, want):
    """The same yardstick for a single layer: the output IS the pre-activation."""
    want = np.asarray(want, np.float64)
    return channel_error(got_nchw, want, np.sqrt((want ** 2).mean(axis=(0, 2, 3))))
