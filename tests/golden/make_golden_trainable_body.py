#!/usr/bin/env python3
"""Op traces of the reference graph builders under TRAIN.FREEZE_CONV_BODY False (build container
only; same stub-import harness and recording model as make_golden_from_reference.py /
make_golden_context.py):

  reference_trainable_body.json
    na_wsddn_train    VGG16 body + webly_heads.add_VGG16_roi_2fc_noise_head + add_webly_outputs +
                      add_webly_losses, the StopGradient on the body's output emitted only
                      `if freeze_conv_body` (model_builder_wsl.py:303-306) - i.e. not
    wsddn_train       the same without the webly head (WEBLY.WEBLY_ON False, ROI_BOX_HEAD
                      wsl_heads.add_VGG16_roi_2fc_head): plain WSDDN
    freeze_at / freeze_conv_body   the two cfg values the traces were taken under

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_trainable_body.py
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
    rcfg.merge_cfg_from_list(['NUM_GPUS', 4, 'TRAIN.FREEZE_CONV_BODY', False])
    from detectron.modeling import VGG16, wsl_heads, webly_heads
    for mod in (wsl_heads, webly_heads):
        mod.const_fill = lambda v: ('ConstantFill', {'value': v})
        mod.gauss_fill = lambda s: ('GaussianFill', {'std': s})

    out = {'freeze_at': int(cfg.TRAIN.FREEZE_AT),
           'freeze_conv_body': bool(cfg.TRAIN.FREEZE_CONV_BODY)}
    for key, webly in (('na_wsddn_train', True), ('wsddn_train', False)):
        if not webly:
            rcfg.merge_cfg_from_list(['WEBLY.WEBLY_ON', False, 'FAST_RCNN.ROI_BOX_HEAD',
                                      'wsl_heads.add_VGG16_roi_2fc_head'])
        m, ops = ctx.recorder(cfg, True)
        blob, dim, scale = VGG16.add_VGG16_conv5_body_origin(m)
        if cfg.TRAIN.FREEZE_CONV_BODY:               # model_builder_wsl.py:303-306
            m.StopGradient(blob, blob)
        if webly:
            ls, dims = webly_heads.add_VGG16_roi_2fc_noise_head(m, blob, dim, scale)
            webly_heads.add_webly_outputs(m, ls, dims)
            lg = webly_heads.add_webly_losses(m)
        else:
            blob_frcn, dim_frcn = wsl_heads.add_VGG16_roi_2fc_head(m, blob, dim, scale)
            wsl_heads.add_wsl_outputs(m, blob_frcn, dim_frcn)
            lg = wsl_heads.add_wsl_losses(m)
        out[key] = dict(ops=ops, losses=m.losses, metrics=m.metrics, loss_gradients=sorted(lg))
    with open(os.path.join(HERE, 'reference_trainable_body.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    for k, v in sorted(out.items()):
        if isinstance(v, dict):
            print(k, len(v['ops']), 'ops; StopGradient at',
                  [o[1][0] for o in v['ops'] if o[0] == 'StopGradient'])


if __name__ == '__main__':
    main()
