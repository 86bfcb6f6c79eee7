#!/usr/bin/env python3
"""Op traces of the reference's ResNet18-WS builders (build container only; same stub-import
harness and recording model as make_golden_deeplab_body.py / make_golden_context.py):

  reference_resnet18_body.json
    conv5_d1_train / conv5_d1_test   ResNet18.add_ResNet18_conv5_body, RESNETS.RES5_DILATION 1
    conv5_d2_train / conv5_d2_test   the same at RES5_DILATION 2 (res5 at stride 1, dilated)
    conv4_train / conv4_test         ResNet18.add_ResNet18_conv4_body
    head_2fc_train / head_2fc_test   wsl_heads.add_ResNet_roi_2fc_head (:860-895) over
                                     ('res5_1_sum', 512, 1/16), FAST_RCNN.MLP_HEAD_DIM 4096
    each: the ops, the parameters they create (name -> shape, in creation order) and the
    (blob, dim, scale) the builder returns (the head: blob, dim)
    resnets                          the RESNETS node's defaults and WSL.MLP_HEAD_DIM's, before any
                                     override
    freeze_at                        TRAIN.FREEZE_AT the traces were taken under

The builders (ResNet18.py, ResNet.py's stem and shortcut, wsl_heads.py) are the reference's own,
imported.  The two DetectionModelHelper methods they call that the recording model does not have -
AffineChannel (detector.py:81-105) and ConvAffine (:428-456) - are restated on it: which blob each
returns decides every later name.  Parameter names follow the Caffe2 helpers (`<out>_w`, `<out>_b`
unless no_bias; AffineChannel `<out>_s`, `<out>_b`).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_resnet18_body.py
"""
import json
import os
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_context as ctx  # noqa: E402
import make_golden_from_reference as base  # noqa: E402

REF = base.REF


def recorder(cfg, train):
    """ctx.recorder plus AffineChannel / ConvAffine with the reference helper's return values."""
    m, ops = ctx.recorder(cfg, train)
    cls = type(m)

    def AffineChannel(self, blob_in, blob_out, dim, inplace=False):
        out = str(blob_in) if inplace else blob_out
        ops.append(['AffineChannel', [str(blob_in), blob_out + '_s', blob_out + '_b'], [out],
                    {'dim': int(dim)}])
        return out

    def ConvAffine(self, blob_in, prefix, dim_in, dim_out, kernel, stride, pad, group=1, dilation=1,
                   weight_init=None, bias_init=None, suffix='_bn', inplace=False):
        conv_blob = self.Conv(blob_in, prefix, dim_in, dim_out, kernel, stride=stride, pad=pad,
                              group=group, dilation=dilation, weight_init=weight_init,
                              bias_init=bias_init, no_bias=1)
        return self.AffineChannel(conv_blob, prefix + suffix, dim=dim_out, inplace=inplace)

    cls.AffineChannel, cls.ConvAffine = AffineChannel, ConvAffine
    return m, ops


def params_of(ops):
    """name -> shape of the parameters the Caffe2 helpers create for these ops, in order."""
    out = []
    for t, ins, outs, kw in ops:
        if t == 'Conv':
            dims = kw['dims']
            k = dims[2] if len(dims) > 2 else kw['kernel']
            out.append([outs[0] + '_w', [dims[1], dims[0], k, k]])
            if not kw.get('no_bias'):
                out.append([outs[0] + '_b', [dims[1]]])
        elif t == 'FC' and 'dims' in kw and len(ins) == 1:
            out.append([outs[0] + '_w', [kw['dims'][1], kw['dims'][0]]])
            out.append([outs[0] + '_b', [kw['dims'][1]]])
        elif t == 'AffineChannel':
            out.append([ins[1], [kw['dim']]])
            out.append([ins[2], [kw['dim']]])
    return out


def main():
    sys.dont_write_bytecode = True
    sys.meta_path.insert(0, base._StubFinder())
    sys.path.insert(0, REF)
    import future.utils
    future.utils.iteritems = lambda d: iter(d.items())
    import detectron.utils.env as envu
    envu.yaml_load = lambda s: yaml.load(s, Loader=yaml.FullLoader)
    from detectron.core import config as rcfg
    cfg = rcfg.cfg
    rcfg.merge_cfg_from_file(os.path.join(REF, 'configs/flickr_voc/na_wsddn_V-16-C5_1x.yaml'))
    out = {'resnets': {k: cfg.RESNETS[k] for k in sorted(cfg.RESNETS)},
           'wsl_mlp_head_dim': list(cfg.WSL.MLP_HEAD_DIM)}
    rcfg.merge_cfg_from_list(['NUM_GPUS', 4, 'WEBLY.WEBLY_ON', False,
                              'RESNETS.TRANS_FUNC', 'residual_transformation',
                              'FAST_RCNN.ROI_BOX_HEAD', 'wsl_heads.add_ResNet_roi_2fc_head',
                              'FAST_RCNN.MLP_HEAD_DIM', 4096])
    from detectron.modeling import ResNet18, wsl_heads
    out['freeze_at'] = int(cfg.TRAIN.FREEZE_AT)
    for key, builder, dilation in (('conv5_d1', ResNet18.add_ResNet18_conv5_body, 1),
                                   ('conv5_d2', ResNet18.add_ResNet18_conv5_body, 2),
                                   ('conv4', ResNet18.add_ResNet18_conv4_body, 1)):
        rcfg.merge_cfg_from_list(['RESNETS.RES5_DILATION', dilation])
        for train in (True, False):
            m, ops = recorder(cfg, train)
            blob, dim, scale = builder(m)
            out['%s_%s' % (key, 'train' if train else 'test')] = dict(
                ops=ops, params=params_of(ops), blob=str(blob), dim=int(dim), scale=float(scale))
    rcfg.merge_cfg_from_list(['RESNETS.RES5_DILATION', 1])
    for train in (True, False):
        m, ops = recorder(cfg, train)
        blob, dim = wsl_heads.add_ResNet_roi_2fc_head(m, 'res5_1_sum', 512, 1. / 16.)
        out['head_2fc_%s' % ('train' if train else 'test')] = dict(
            ops=ops, params=params_of(ops), blob=str(blob), dim=int(dim), scale=1. / 16.)
    with open(os.path.join(HERE, 'reference_resnet18_body.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    for k, v in sorted(out.items()):
        if isinstance(v, dict) and 'ops' in v:
            print(k, len(v['ops']), 'ops;', len(v['params']), 'params; convs',
                  sorted({(o[3].get('kernel', (o[3]['dims'] + [0])[2]), o[3].get('stride'),
                           o[3].get('pad'), o[3].get('dilation')) for o in v['ops']
                          if o[0] == 'Conv'}, key=str), 'scale', v['scale'])


if __name__ == '__main__':
    main()
