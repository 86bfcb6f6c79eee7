#!/usr/bin/env python3
"""Op traces of the reference's two other VGG-16 conv bodies (build container only; same
stub-import harness and recording model as make_golden_from_reference.py / make_golden_context.py /
make_golden_trainable_body.py):

  reference_deeplab_body.json
    deeplab_d2_train / deeplab_d2_test   VGG16.add_VGG16_conv5_body_deeplab (VGG16.py:94-140) under
                                         the shipped yaml (WSL.DILATION 2): kernel-3 / pad-1 pools,
                                         pool4 at stride 1, conv5_x dilated
    deeplab_d1_train / deeplab_d1_test   the same with WSL.DILATION 1: pool4 at stride 2
    conv4_train / conv4_test             VGG16.add_VGG16_conv4_body_origin (:61-91), WSL.DILATION 1
    each: the body's ops, and the (dim, spatial scale) the builder returns
    freeze_at                            TRAIN.FREEZE_AT the traces were taken under

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_deeplab_body.py
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
    rcfg.merge_cfg_from_list(['NUM_GPUS', 4])
    from detectron.modeling import VGG16

    out = {'freeze_at': int(cfg.TRAIN.FREEZE_AT)}
    for key, builder, dilation in (('deeplab_d2', VGG16.add_VGG16_conv5_body_deeplab, 2),
                                   ('deeplab_d1', VGG16.add_VGG16_conv5_body_deeplab, 1),
                                   ('conv4', VGG16.add_VGG16_conv4_body_origin, 1)):
        rcfg.merge_cfg_from_list(['WSL.DILATION', dilation])
        for train in (True, False):
            m, ops = ctx.recorder(cfg, train)
            blob, dim, scale = builder(m)
            out['%s_%s' % (key, 'train' if train else 'test')] = dict(
                ops=ops, blob=str(blob), dim=int(dim), scale=float(scale))
    with open(os.path.join(HERE, 'reference_deeplab_body.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    for k, v in sorted(out.items()):
        if isinstance(v, dict):
            print(k, len(v['ops']), 'ops; pools',
                  [(o[3]['kernel'], o[3]['pad'], o[3]['stride']) for o in v['ops']
                   if o[0] == 'MaxPool'], 'scale', v['scale'])


if __name__ == '__main__':
    main()
