#!/usr/bin/env python3
"""Op traces of the reference graph builders under FAST_RCNN.ROI_XFORM_METHOD RoIAlign,
FAST_RCNN.ROI_XFORM_SAMPLING_RATIO 2 (build container only; same stub-import harness and recording
model as make_golden_from_reference.py / make_golden_context.py / make_golden_trainable_body.py):

  reference_roi_align.json
    frozen / trainable          TRAIN.FREEZE_CONV_BODY True / False, each holding
      na_wsddn_train            VGG16 body + webly_heads.add_VGG16_roi_2fc_noise_head +
                                add_webly_outputs + add_webly_losses
      na_wsddn_test             the same graph built with train False (no losses)
      wsddn_train               plain WSDDN (WEBLY.WEBLY_ON False, ROI_BOX_HEAD
                                wsl_heads.add_VGG16_roi_2fc_head)
    roi_xform_method / sampling_ratio   the two cfg values the traces were taken under

The shared recording model stubs RoIFeatureTransform (two outputs, no sampling_ratio), which is the
very method this trace is about.  DetectionModelHelper itself cannot be imported (its base class is
a caffe2 stub), so the method's own source is cut out of the reference's detector.py with `ast` at
run time, compiled as it stands and bound to the recorder: the RoI op below is emitted by the
reference's code, through `self.net.__getattr__(method)(...)`.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_roi_align.py
"""
import ast
import json
import os
import sys
import types

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_context as ctx  # noqa: E402
import make_golden_from_reference as base  # noqa: E402

REF = base.REF
ALIGN = ['FAST_RCNN.ROI_XFORM_METHOD', 'RoIAlign', 'FAST_RCNN.ROI_XFORM_SAMPLING_RATIO', 2]
WSDDN = ['WEBLY.WEBLY_ON', False, 'FAST_RCNN.ROI_BOX_HEAD', 'wsl_heads.add_VGG16_roi_2fc_head']
NA = ['WEBLY.WEBLY_ON', True, 'FAST_RCNN.ROI_BOX_HEAD', 'webly_heads.add_VGG16_roi_2fc_noise_head']


def reference_roi_feature_transform(cfg):
    """DetectionModelHelper.RoIFeatureTransform of the reference, compiled from its file."""
    path = os.path.join(REF, 'detectron', 'modeling', 'detector.py')
    tree = ast.parse(open(path).read(), path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'DetectionModelHelper']
    fn = [n for n in cls[0].body
          if isinstance(n, ast.FunctionDef) and n.name == 'RoIFeatureTransform']
    mod = ast.Module(body=fn, type_ignores=[])
    ns = {'cfg': cfg}
    exec(compile(mod, path, 'exec'), ns)
    return ns['RoIFeatureTransform']


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
    rcfg.merge_cfg_from_list(['NUM_GPUS', 4] + ALIGN)
    from detectron.modeling import VGG16, wsl_heads, webly_heads
    for mod in (wsl_heads, webly_heads):
        mod.const_fill = lambda v: ('ConstantFill', {'value': v})
        mod.gauss_fill = lambda s: ('GaussianFill', {'std': s})

    xform = reference_roi_feature_transform(cfg)
    out = {'roi_xform_method': str(cfg.FAST_RCNN.ROI_XFORM_METHOD),
           'sampling_ratio': int(cfg.FAST_RCNN.ROI_XFORM_SAMPLING_RATIO)}
    for mode, frozen in (('frozen', True), ('trainable', False)):
        rcfg.merge_cfg_from_list(['TRAIN.FREEZE_CONV_BODY', frozen])
        out[mode] = {}
        for key, webly, train in (('na_wsddn_train', True, True), ('na_wsddn_test', True, False),
                                  ('wsddn_train', False, True)):
            rcfg.merge_cfg_from_list(NA if webly else WSDDN)
            m, ops = ctx.recorder(cfg, train)
            m.RoIFeatureTransform = types.MethodType(xform, m)
            blob, dim, scale = VGG16.add_VGG16_conv5_body_origin(m)
            if cfg.TRAIN.FREEZE_CONV_BODY:               # model_builder_wsl.py:303-306
                m.StopGradient(blob, blob)
            lg = []
            if webly:
                ls, dims = webly_heads.add_VGG16_roi_2fc_noise_head(m, blob, dim, scale)
                webly_heads.add_webly_outputs(m, ls, dims)
                if train:
                    lg = webly_heads.add_webly_losses(m)
            else:
                blob_frcn, dim_frcn = wsl_heads.add_VGG16_roi_2fc_head(m, blob, dim, scale)
                wsl_heads.add_wsl_outputs(m, blob_frcn, dim_frcn)
                if train:
                    lg = wsl_heads.add_wsl_losses(m)
            out[mode][key] = dict(ops=ops, losses=m.losses, metrics=m.metrics,
                                  loss_gradients=sorted(lg))
    with open(os.path.join(HERE, 'reference_roi_align.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    for mode in ('frozen', 'trainable'):
        for k, v in sorted(out[mode].items()):
            print(mode, k, len(v['ops']), 'ops;',
                  [o[:3] for o in v['ops'] if o[0].startswith('RoI') and 'Boost' not in o[0]])


if __name__ == '__main__':
    main()
