#!/usr/bin/env python3
"""Op traces of the reference graph builders with WSL.CENTER_LOSS, the multi-centre feature loss
(build container only; same stub-import harness as make_golden_from_reference.py /
make_golden_context.py):

  reference_center_loss.json
    wsl_center_train       generalized_wsl WITHOUT the webly head (WEBLY.WEBLY_ON False,
                           ROI_BOX_HEAD wsl_heads.add_VGG16_roi_2fc_head): conv body, 2-fc head,
                           add_wsl_outputs, add_wsl_losses with add_center_loss
                           (wsl_heads.py:230-276, :425-431)
    na_wsddn_center_train  the noise-aware head of the headline config with the switch on
                           (webly_heads.py:199-206)
    each: ops, losses, metrics, loss_gradients, params (name, shape, initialiser, tags as
    model.create_param received them)
    cfg                    the three reference keys the NAWS.CENTER_LOSS_* knobs stand for

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_center_loss.py
"""
import json
import os
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_from_reference as base  # noqa: E402
import make_golden_context as ctx  # noqa: E402

REF = base.REF


class _Initializers(object):
    @staticmethod
    def Initializer(name, **kw):
        return [str(name), dict(kw)]


class _Tags(object):
    COMPUTED_PARAM = 'COMPUTED_PARAM'


def recorder(cfg, train):
    m, ops = ctx.recorder(cfg, train)
    params = []

    def create_param(param_name, shape, initializer, tags=None):
        params.append(dict(name=str(param_name), shape=[int(s) for s in shape],
                           initializer=initializer, tags=tags))
        return str(param_name)

    m.create_param = create_param
    return m, ops, params


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
    rcfg.merge_cfg_from_list(['NUM_GPUS', 4, 'WSL.CENTER_LOSS', True])
    from detectron.modeling import VGG16, wsl_heads, webly_heads
    for mod in (wsl_heads, webly_heads):
        mod.const_fill = lambda v: ('ConstantFill', {'value': v})
        mod.gauss_fill = lambda s: ('GaussianFill', {'std': s})
    wsl_heads.initializers = _Initializers
    wsl_heads.ParameterTags = _Tags

    out = {'cfg': {'CENTER_LOSS_NUMBER': int(cfg.WSL.CENTER_LOSS_NUMBER),
                   'CENTER_LOSS_TOP_K': int(cfg.WSL.CENTER_LOSS_TOP_K),
                   'CSC_MAX_ITER': int(cfg.WSL.CSC_MAX_ITER)}}

    m, ops, params = recorder(cfg, True)
    blob, dim, scale = VGG16.add_VGG16_conv5_body_origin(m)
    m.StopGradient(blob, blob)
    ls, dims = webly_heads.add_VGG16_roi_2fc_noise_head(m, blob, dim, scale)
    webly_heads.add_webly_outputs(m, ls, dims)
    lg = webly_heads.add_webly_losses(m)
    out['na_wsddn_center_train'] = dict(ops=ops, losses=m.losses, metrics=m.metrics, params=params,
                                        loss_gradients=sorted(lg))

    rcfg.merge_cfg_from_list(['WEBLY.WEBLY_ON', False, 'FAST_RCNN.ROI_BOX_HEAD',
                              'wsl_heads.add_VGG16_roi_2fc_head'])
    m, ops, params = recorder(cfg, True)
    blob, dim, scale = VGG16.add_VGG16_conv5_body_origin(m)
    m.StopGradient(blob, blob)
    blob_frcn, dim_frcn = wsl_heads.add_VGG16_roi_2fc_head(m, blob, dim, scale)
    wsl_heads.add_wsl_outputs(m, blob_frcn, dim_frcn)
    lg = wsl_heads.add_wsl_losses(m)
    out['wsl_center_train'] = dict(ops=ops, losses=m.losses, metrics=m.metrics, params=params,
                                   loss_gradients=sorted(lg))

    with open(os.path.join(HERE, 'reference_center_loss.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    for k, v in sorted(out.items()):
        if 'ops' in v:
            print(k, len(v['ops']), 'ops;', [o[0] for o in v['ops'][-8:]], v['params'])


if __name__ == '__main__':
    main()
