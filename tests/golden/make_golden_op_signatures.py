#!/usr/bin/env python3
"""The forward and backward op lists of every shipped build of THIS tree, as SHA-256 digests over
type, inputs, outputs and all args but `uuid`; a build the generator refuses is recorded as the
exception type it raises.  Run on the commit before the operator table existed, its output
(op_signatures_before.json) pins that the table-driven generator records exactly the ops the two
lists in detector.py recorded (tests/test_op_table.py).

    PYTHONPATH=na-fwebsod_amd python tests/golden/make_golden_op_signatures.py
"""
import json
import os

from make_golden_roipoolf_signatures import HERE, WSDDN, YAML, digest

BUILDS = {
    'na_wsddn': [],
    'center_loss': ['WSL.CENTER_LOSS', True],
    'wsddn_center_loss': WSDDN + ['WSL.CENTER_LOSS', True],
    'roi_align': ['FAST_RCNN.ROI_XFORM_METHOD', 'RoIAlign',
                  'FAST_RCNN.ROI_XFORM_SAMPLING_RATIO', 2],
    'wsddn': WSDDN,
    'wsddn_oicr': WSDDN + ['WSL.OICR', True],
    'wsddn_context': WSDDN + ['WSL.CONTEXT', True],
    'wsddn_context_oicr': WSDDN + ['WSL.CONTEXT', True, 'WSL.OICR', True],
    'min_entropy': ['WSL.MIN_ENTROPY_LOSS', True],
    'conv4': ['MODEL.CONV_BODY', 'VGG16.add_VGG16_conv4_body_origin'],
    'deeplab': ['MODEL.CONV_BODY', 'VGG16.add_VGG16_conv5_body_deeplab'],
}


def create(name, train, frozen, num_gpus=4, extra=()):
    """The model of one build under a freshly reset cfg (left set: the caller resets it)."""
    from detectron.core import config as c
    import detectron.modeling.model_builder_wsl as mb
    c.reset_cfg()
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['NUM_GPUS', num_gpus, 'TRAIN.FREEZE_CONV_BODY', frozen] + BUILDS[name] +
                          list(extra))
    c.assert_and_infer_cfg(make_immutable=False)
    return mb.create(c.cfg.MODEL.TYPE, train=train)


def record():
    from detectron.core import config as c
    out = {}
    for name in sorted(BUILDS):
        for train in (True, False):
            for frozen in (True, False):
                key = '%s/%s/%s' % (name, 'train' if train else 'test',
                                    'frozen' if frozen else 'trainable')
                try:
                    m = create(name, train, frozen)
                except Exception as e:      # a refused build: its exception type is the record
                    out[key] = dict(refused=type(e).__name__)
                    continue
                out[key] = dict(forward=digest(m.net.ops), backward=digest(m.grad_ops),
                                n_forward=len(m.net.ops), n_backward=len(m.grad_ops))
    c.reset_cfg()
    return out


if __name__ == '__main__':
    with open(os.path.join(HERE, 'op_signatures_before.json'), 'w') as f:
        json.dump(record(), f, indent=1, sort_keys=True)
