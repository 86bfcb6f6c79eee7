"""ResNet18-WS conv bodies of the WSL path.  Mirrors detectron/modeling/ResNet18.py
(`add_ResNet18_conv4_body`, `add_ResNet18_conv5_body`, `add_stage`, `add_residual_block`,
`residual_transformation`) over the stem and the shortcut of detectron/modeling/ResNet.py
(`basic_bn_stem` :246-256, `basic_bn_shortcut` :203-220): a 7x7 / stride-2 conv, AffineChannel,
ReLU and a 3x3 / stride-2 pool, then four (conv4: three) stages of two basic blocks - two 3x3
ConvAffine, a 1x1 ConvAffine shortcut where the width changes, Sum, ReLU.  Every Conv is
bias-free; AffineChannel stands for the frozen BatchNorm.

The stride of a block is upstream's rule, kept as written: stride_init where the width changes,
the stage is not res2 and the stage is not dilated; 1 otherwise.  So res3 and res4 halve the map,
res2 does not (pool1 already did), and res5 halves it at RESNETS.RES5_DILATION 1 and keeps it,
with dilation-2 / pad-2 3x3 convs, at 2: the body returns scale 1/32 * RES5_DILATION.

No convolution of this body has a backward form, so it runs frozen only
(TRAIN.FREEZE_CONV_BODY True), as the DeepLab VGG-16 body does.  The bottleneck transformation,
the GroupNorm stem / shortcut and grouped convolutions belong to other ResNets and are refused."""
from detectron.core.config import cfg


def add_ResNet18_conv4_body(model):
    return add_shallow_ResNet_convX_body(model, (2, 2, 2))


def add_ResNet18_conv5_body(model):
    return add_shallow_ResNet_convX_body(model, (2, 2, 2, 2))


def _check_cfg(model):
    """The RESNETS switches this body can honour, each refusal naming its key."""
    if model.train and not cfg.TRAIN.FREEZE_CONV_BODY:
        raise NotImplementedError('TRAIN.FREEZE_CONV_BODY: False with a ResNet18 body is not on the '
                                  'hot path: the strided convolutions have no backward form, the '
                                  'body runs frozen only (TRAIN.FREEZE_CONV_BODY: True)')
    if cfg.RESNETS.TRANS_FUNC != 'residual_transformation':
        raise NotImplementedError('RESNETS.TRANS_FUNC: {} is not on the hot path: the ResNet18 body '
                                  'is built of residual_transformation blocks'.format(
                                      cfg.RESNETS.TRANS_FUNC))
    if cfg.RESNETS.STEM_FUNC != 'basic_bn_stem':
        raise NotImplementedError('RESNETS.STEM_FUNC: {} is not on the hot path (no GroupNorm): '
                                  'basic_bn_stem only'.format(cfg.RESNETS.STEM_FUNC))
    if cfg.RESNETS.SHORTCUT_FUNC != 'basic_bn_shortcut':
        raise NotImplementedError('RESNETS.SHORTCUT_FUNC: {} is not on the hot path (no GroupNorm): '
                                  'basic_bn_shortcut only'.format(cfg.RESNETS.SHORTCUT_FUNC))
    if cfg.RESNETS.NUM_GROUPS != 1:
        raise NotImplementedError('RESNETS.NUM_GROUPS: {} is not on the hot path: no grouped '
                                  'convolution'.format(cfg.RESNETS.NUM_GROUPS))


def add_stage(model, prefix, blob_in, n, dim_in, dim_out, dim_inner, dilation, stride_init=2):
    """n residual blocks; all but the last sum in place (the last may be fetched)."""
    for i in range(n):
        blob_in = add_residual_block(model, '{}_{}'.format(prefix, i), blob_in, dim_in, dim_out,
                                     dim_inner, dilation, stride_init, inplace_sum=i < n - 1)
        dim_in = dim_out
    return blob_in, dim_in


def add_shallow_ResNet_convX_body(model, block_counts):
    """The body up to res4 (three counts) or res5 (four) -> (blob, dim, spatial scale)."""
    _check_cfg(model)
    freeze_at = cfg.TRAIN.FREEZE_AT
    assert freeze_at in [0, 2, 3, 4, 5]
    p, dim_in = globals()[cfg.RESNETS.STEM_FUNC](model, 'data')
    (n1, n2, n3) = block_counts[:3]
    s, dim_in = add_stage(model, 'res2', p, n1, dim_in, 64, 0, 1)
    if freeze_at == 2:
        model.StopGradient(s, s)
    s, dim_in = add_stage(model, 'res3', s, n2, dim_in, 128, 0, 1)
    if freeze_at == 3:
        model.StopGradient(s, s)
    s, dim_in = add_stage(model, 'res4', s, n3, dim_in, 256, 0, 1)
    if freeze_at == 4:
        model.StopGradient(s, s)
    if len(block_counts) == 4:
        n4 = block_counts[3]
        s, dim_in = add_stage(model, 'res5', s, n4, dim_in, 512, 0, cfg.RESNETS.RES5_DILATION)
        if freeze_at == 5:
            model.StopGradient(s, s)
        return s, dim_in, 1. / 32. * cfg.RESNETS.RES5_DILATION
    return s, dim_in, 1. / 16.


def add_residual_block(model, prefix, blob_in, dim_in, dim_out, dim_inner, dilation, stride_init=2,
                       inplace_sum=False):
    """prefix = res<stage>_<block>.  pool1 precedes res2, so res2 keeps stride 1."""
    stride = stride_init if (dim_in != dim_out and 'res2' not in prefix and dilation == 1) else 1
    tr = globals()[cfg.RESNETS.TRANS_FUNC](model, blob_in, dim_in, dim_out, stride, prefix, dim_inner,
                                           group=cfg.RESNETS.NUM_GROUPS, dilation=dilation)
    sc = globals()[cfg.RESNETS.SHORTCUT_FUNC](model, prefix, blob_in, dim_in, dim_out, stride)
    if inplace_sum:
        s = model.net.Sum([tr, sc], tr)
    else:
        s = model.net.Sum([tr, sc], prefix + '_sum')
    return model.Relu(s, s)


def basic_bn_shortcut(model, prefix, blob_in, dim_in, dim_out, stride):
    """ResNet.py:203-220: the identity, or a bias-free 1x1 conv + AffineChannel where the width
    changes."""
    if dim_in == dim_out:
        return blob_in
    c = model.Conv(blob_in, prefix + '_branch1', dim_in, dim_out, kernel=1, stride=stride, no_bias=1)
    return model.AffineChannel(c, prefix + '_branch1_bn', dim=dim_out)


def basic_bn_stem(model, data, **kwargs):
    """ResNet.py:246-256: conv1 7x7 / s2 / p3 (no bias), AffineChannel in place, ReLU, pool1."""
    dim = 64
    p = model.Conv(data, 'conv1', 3, dim, 7, pad=3, stride=2, no_bias=1)
    p = model.AffineChannel(p, 'res_conv1_bn', dim=dim, inplace=True)
    p = model.Relu(p, p)
    p = model.MaxPool(p, 'pool1', kernel=3, pad=1, stride=2)
    return p, dim


def residual_transformation(model, blob_in, dim_in, dim_out, stride, prefix, dim_inner, dilation=1,
                            group=1):
    """Two 3x3 ConvAffine (MSRA-filled): the first strided, in place and followed by ReLU."""
    weight_init = ('MSRAFill', {})
    cur = model.ConvAffine(blob_in, prefix + '_branch2a', dim_in, dim_out, kernel=3, stride=stride,
                           pad=1 * dilation, dilation=dilation, group=group, inplace=True,
                           weight_init=weight_init)
    cur = model.Relu(cur, cur)
    cur = model.ConvAffine(cur, prefix + '_branch2b', dim_out, dim_out, kernel=3, stride=1,
                           pad=1 * dilation, dilation=dilation, group=group, inplace=False,
                           weight_init=weight_init)
    return cur
