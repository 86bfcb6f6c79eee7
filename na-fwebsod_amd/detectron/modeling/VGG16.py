"""VGG-16 conv bodies of the WSL path.  Mirrors detectron/modeling/VGG16.py:9-48
(`add_VGG16_conv5_body_origin`): thirteen 3x3 conv + in-place ReLU, k2s2 max-pools after
blocks 1-3, and with WSL.DILATION == 2 a stride-1 pool4 followed by dilation-2 conv5_x
(feature stride 8); FREEZE_AT == 2 stops gradients at pool2 - the only value a trainable body
(TRAIN.FREEZE_CONV_BODY False) accepts.

`add_VGG16_conv4_body_origin` (:61-91) is that body cut after conv4_3 (feature stride 8).
`add_VGG16_conv5_body_deeplab` (:94-140) pools with kernel 3 / pad 1 instead (stride 2 after
blocks 1-3; pool4 at stride 1 when dilated, 2 otherwise), so every level is ceil(H / 2) and
conv5_3 sits at a true 1/8 or 1/16; it has no StopGradient at pool2, so a trainable DeepLab body
would train conv1_1, which has no weight-gradient form: that body runs frozen only.  Parameter
names and shapes are the origin body's."""
from detectron.core.config import cfg

_BLOCKS = (
    (1, (3, 64, 64)),
    (2, (64, 128, 128)),
    (3, (128, 256, 256, 256)),
    (4, (256, 512, 512, 512)),
)


def _conv_relu(model, blob_in, name, dim_in, dim_out, pad, dilation):
    if dilation == 1:
        model.Conv(blob_in, name, dim_in, dim_out, 3, pad=pad, stride=1)
    else:
        model.Conv(blob_in, name, dim_in, dim_out, 3, pad=pad, stride=1, dilation=dilation)
    return model.Relu(name, name)


def add_VGG16_conv5_body_origin(model):
    if model.train and not cfg.TRAIN.FREEZE_CONV_BODY and cfg.TRAIN.FREEZE_AT != 2:
        # conv1_1 has 3 input channels and no weight-gradient form; the body trains from conv3_1
        raise NotImplementedError('TRAIN.FREEZE_AT: {} with TRAIN.FREEZE_CONV_BODY: False is not '
                                  'on the hot path: the trainable body needs TRAIN.FREEZE_AT: 2 '
                                  '(conv3_1 and up)'.format(cfg.TRAIN.FREEZE_AT))
    blob = 'data'
    for idx, dims in _BLOCKS:
        for j in range(1, len(dims)):
            blob = _conv_relu(model, blob, 'conv%d_%d' % (idx, j), dims[j - 1], dims[j], 1, 1)
        if idx < 4:
            blob = model.MaxPool(blob, 'pool%d' % idx, kernel=2, pad=0, stride=2)
            if idx == 2 and cfg.TRAIN.FREEZE_AT == 2:
                model.StopGradient(blob, blob)
    dilated = cfg.WSL.DILATION == 2
    blob = model.MaxPool(blob, 'pool4', kernel=2, pad=0, stride=1 if dilated else 2)
    d = 2 if dilated else 1
    for j in (1, 2, 3):
        blob = _conv_relu(model, blob, 'conv5_%d' % j, 512, 512, d, d)
    return blob, 512, 1. / 8. if dilated else 1. / 16.


def add_VGG16_conv4_body_origin(model):
    if model.train and not cfg.TRAIN.FREEZE_CONV_BODY and cfg.TRAIN.FREEZE_AT != 2:
        raise NotImplementedError('TRAIN.FREEZE_AT: {} with TRAIN.FREEZE_CONV_BODY: False is not '
                                  'on the hot path: the trainable body needs TRAIN.FREEZE_AT: 2 '
                                  '(conv3_1 and up)'.format(cfg.TRAIN.FREEZE_AT))
    blob = 'data'
    for idx, dims in _BLOCKS:
        for j in range(1, len(dims)):
            blob = _conv_relu(model, blob, 'conv%d_%d' % (idx, j), dims[j - 1], dims[j], 1, 1)
        if idx < 4:
            blob = model.MaxPool(blob, 'pool%d' % idx, kernel=2, pad=0, stride=2)
            if idx == 2 and cfg.TRAIN.FREEZE_AT == 2:
                model.StopGradient(blob, blob)
    return blob, 512, 1. / 8.


def add_VGG16_conv5_body_deeplab(model):
    if model.train and not cfg.TRAIN.FREEZE_CONV_BODY:
        # no StopGradient at pool2 upstream (VGG16.py:94-140): the gradient would reach conv1_1,
        # which has 3 input channels and no weight-gradient form, and the 3x3 pool has no backward
        raise NotImplementedError('TRAIN.FREEZE_CONV_BODY: False with MODEL.CONV_BODY '
                                  'VGG16.add_VGG16_conv5_body_deeplab is not on the hot path: the '
                                  'DeepLab body runs frozen only (TRAIN.FREEZE_CONV_BODY: True)')
    dilated = cfg.WSL.DILATION == 2
    blob = 'data'
    for idx, dims in _BLOCKS:
        for j in range(1, len(dims)):
            blob = _conv_relu(model, blob, 'conv%d_%d' % (idx, j), dims[j - 1], dims[j], 1, 1)
        blob = model.MaxPool(blob, 'pool%d' % idx, kernel=3, pad=1,
                             stride=1 if idx == 4 and dilated else 2)
    d = 2 if dilated else 1
    for j in (1, 2, 3):
        blob = _conv_relu(model, blob, 'conv5_%d' % j, 512, 512, d, d)
    return blob, 512, 1. / 8. if dilated else 1. / 16.
