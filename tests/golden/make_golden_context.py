#!/usr/bin/env python3
"""Op traces of the reference graph builders for WSL.CONTEXT, the contextual WSDDN head (build
container only; same stub-import harness as make_golden_from_reference.py / make_golden_oicr.py):

  reference_context.json
    wsl_context_train / wsl_context_test            generalized_wsl WITHOUT the webly head
                                                    (WEBLY.WEBLY_ON False, ROI_BOX_HEAD
                                                    wsl_heads.add_VGG16_roi_2fc_head) and
                                                    WSL.CONTEXT: conv body, RoIContext, the three
                                                    2-fc streams on shared fc6 / fc7
                                                    (wsl_heads.py:684-766), add_wsl_context_outputs
                                                    (:185-209), add_wsl_losses
    wsl_context_oicr_train / wsl_context_oicr_test  the same with WSL.OICR: the refinement
                                                    branches read the plain stream (:69-76)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_context.py
"""
import json
import os
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_from_reference as base  # noqa: E402

REF = base.REF


def recorder(cfg, train):
    ops = []

    class Rec(object):
        def __init__(self):
            self.train = train
            self.num_classes = cfg.MODEL.NUM_CLASSES
            self.losses, self.metrics = [], []
            self.net = self
            self.param_init_net = self

        def AddLosses(self, l):
            self.losses += l if isinstance(l, list) else [l]

        def AddMetrics(self, m):
            self.metrics += m if isinstance(m, list) else [m]

        def RoIFeatureTransform(self, blobs_in, blob_out, blob_rois='rois', method='RoIPoolF',
                                resolution=7, spatial_scale=1. / 16., sampling_ratio=0):
            ops.append([method, [blobs_in, blob_rois], [blob_out, '_argmax_' + blob_out],
                        {'pooled_h': resolution, 'pooled_w': resolution,
                         'spatial_scale': spatial_scale}])
            return blob_out

        def __getattr__(self, op):
            def f(ins, outs=None, *a, **kw):
                ins_l = ins if isinstance(ins, list) else [ins]
                o = outs if outs is not None else ins
                outs_l = o if isinstance(o, list) else [o]
                kws = {k: (v if isinstance(v, (int, float, str, bool, list, tuple)) else str(v))
                       for k, v in kw.items() if k not in ('weight_init', 'bias_init')}
                if op in ('Conv', 'FC') and a:
                    kws['dims'] = [int(x) for x in a[:3]]
                if op == 'FC' and 'weight_init' in kw:
                    kws['weight_init'] = list(kw['weight_init'])
                if 'uuid' in kws:
                    kws['uuid'] = 0            # random per build (uuid4): not part of the graph
                ops.append([op, [str(x) for x in ins_l], [str(x) for x in outs_l], kws])
                return outs_l[0] if len(outs_l) == 1 else tuple(outs_l)
            return f

    return Rec(), ops


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
    rcfg.merge_cfg_from_list(['NUM_GPUS', 4, 'WEBLY.WEBLY_ON', False, 'WSL.CONTEXT', True,
                              'FAST_RCNN.ROI_BOX_HEAD', 'wsl_heads.add_VGG16_roi_2fc_head'])
    from detectron.modeling import VGG16, wsl_heads
    wsl_heads.const_fill = lambda v: ('ConstantFill', {'value': v})
    wsl_heads.gauss_fill = lambda s: ('GaussianFill', {'std': s})

    out = {'context_ratio_cfg': float(cfg.WSL.CONTEXT_RATIO)}
    for oicr in (False, True):
        rcfg.merge_cfg_from_list(['WSL.OICR', oicr])
        for train in (True, False):
            m, ops = recorder(cfg, train)
            blob, dim, scale = VGG16.add_VGG16_conv5_body_origin(m)
            m.StopGradient(blob, blob)
            blob_frcn, dim_frcn = wsl_heads.add_VGG16_roi_2fc_head(m, blob, dim, scale)
            wsl_heads.add_wsl_outputs(m, blob_frcn, dim_frcn)
            lg = wsl_heads.add_wsl_losses(m) if train else None
            key = 'wsl_context%s_%s' % ('_oicr' if oicr else '', 'train' if train else 'test')
            out[key] = dict(ops=ops, losses=m.losses, metrics=m.metrics,
                            loss_gradients=sorted(lg) if lg else None)
    with open(os.path.join(HERE, 'reference_context.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    for k, v in sorted(out.items()):
        if isinstance(v, dict):
            print(k, len(v['ops']), 'ops;', [o[0] for o in v['ops'][-12:]])


if __name__ == '__main__':
    main()
