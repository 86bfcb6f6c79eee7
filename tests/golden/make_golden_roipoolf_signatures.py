#!/usr/bin/env python3
"""The op lists of the RoIPoolF builds of THIS tree, as SHA-256 digests: run on the commit before
RoIAlign was accepted, its output (roipoolf_signatures_before.json) pins that the default pooling
method builds exactly the graphs it built then (tests/test_roi_align.py).

    PYTHONPATH=na-fwebsod_amd python tests/golden/make_golden_roipoolf_signatures.py
"""
import hashlib
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
YAML = os.path.join(ROOT, 'na-fwebsod_amd', 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
WSDDN = ['WEBLY.WEBLY_ON', False, 'FAST_RCNN.ROI_BOX_HEAD', 'wsl_heads.add_VGG16_roi_2fc_head']
BUILDS = {'na_wsddn': [], 'wsddn': WSDDN, 'wsddn_oicr': WSDDN + ['WSL.OICR', True],
          'wsddn_context': WSDDN + ['WSL.CONTEXT', True]}


def digest(ops):
    rows = []
    for o in ops:
        args = {k: v for k, v in o.args.items() if k != 'uuid'}
        rows.append([o.type, list(o.inputs), list(o.outputs), args])
    return hashlib.sha256(json.dumps(rows, sort_keys=True, default=str).encode()).hexdigest()


def record():
    from detectron.core import config as c
    import detectron.modeling.model_builder_wsl as mb
    out = {}
    for name, extra in sorted(BUILDS.items()):
        for train in (True, False):
            for frozen in (True, False):
                if name == 'wsddn_context' and not frozen:
                    continue                        # RoILoopPool has no gradient: refused
                c.reset_cfg()
                c.merge_cfg_from_file(YAML)
                c.merge_cfg_from_list(['NUM_GPUS', 4, 'TRAIN.FREEZE_CONV_BODY', frozen] + extra)
                c.assert_and_infer_cfg(make_immutable=False)
                m = mb.create(c.cfg.MODEL.TYPE, train=train)
                key = '%s/%s/%s' % (name, 'train' if train else 'test',
                                    'frozen' if frozen else 'trainable')
                out[key] = dict(forward=digest(m.net.ops), backward=digest(m.grad_ops),
                                n_forward=len(m.net.ops), n_backward=len(m.grad_ops))
    c.reset_cfg()
    return out


if __name__ == '__main__':
    with open(os.path.join(HERE, 'roipoolf_signatures_before.json'), 'w') as f:
        json.dump(record(), f, indent=1, sort_keys=True)
