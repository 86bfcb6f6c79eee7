#!/usr/bin/env python3
"""Record what the reference's own config loader makes of the `cfg` string this project writes
into detections.pkl and weights files: the reference's load_cfg + merge_cfg_from_cfg (what
tools/reval.py:88-93 does with a detections.pkl) and load_cfg on a weights file's entry
(utils/net_wsl.py:64-66, :277), run in a child interpreter on the imported reference (the two
packages share the name `detectron`).

Runs ONLY where the reference tree is present (make_golden_from_reference.REF).  Writes
reference_cfg_load.json: the dumped string, with the output directory and the repository's
root replaced by the placeholders below, and the lines the reference printed.
tests/test_test_engine_cpu.py checks that this project still writes that very string, so the
recorded verdict holds for it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cfg_load.py
"""
import json
import os
import pickle
import subprocess
import sys
import tempfile
import textwrap

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'na-fwebsod_amd'))
YAML = os.path.join(ROOT, 'na-fwebsod_amd', 'configs', 'flickr_voc', 'na_wsddn_V-16-C5_1x.yaml')
OUTPUT_DIR = '<OUTPUT_DIR>'
ROOT_DIR = '<ROOT_DIR>'

CHILD = textwrap.dedent('''
    import pickle, sys
    sys.dont_write_bytecode = True
    sys.path.insert(0, %r)
    import yaml
    from make_golden_from_reference import REF, _StubFinder
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, REF)
    import future.utils
    future.utils.iteritems = lambda d: iter(d.items())
    import detectron.utils.env as envu
    # (the reference's `yaml.load` without a Loader argument is PyYAML's unsafe loader)
    envu.yaml_load = lambda s: yaml.load(s, Loader=yaml.UnsafeLoader)
    from detectron.core import config as rcfg
    assert rcfg.__file__.startswith(REF)
    dets = pickle.load(open(%r, 'rb'))
    rcfg.merge_cfg_from_cfg(rcfg.load_cfg(dets['cfg']))
    c = rcfg.cfg
    print('MERGED', c.MODEL.NUM_CLASSES, c.TEST.BBOX_AUG.ENABLED, type(c.TEST.BBOX_AUG.SCALES).__name__,
          c.PIXEL_MEANS.shape, len(dets['all_boxes']), len(dets['all_segms'][1]))
    # a weights file written here, read the reference's way (utils/net_wsl.py:64-66, :277)
    saved = rcfg.load_cfg(pickle.load(open(%r, 'rb'))['cfg'])
    print('WEIGHTS_CFG', type(saved).__name__, 'MODEL' in saved, 'BBOX_REG_WEIGHTS' in saved.MODEL,
          saved.MODEL.TYPE, saved.WSL.DILATION)
''')


def dumped_files(out_dir):
    """detections.pkl and model_final.pkl as tests/test_test_engine_cpu.py writes them (its
    _cfg(n_images=2, gpus=1)) -> (their paths, the cfg fields that steer the reader)."""
    from detectron.core import config as c
    from detectron.core import test_engine_wsl as te
    import detectron.utils.env as envu
    from detectron.utils.net_wsl import save_object
    c.reset_cfg()
    c.merge_cfg_from_file(YAML)
    c.merge_cfg_from_list(['OUTPUT_DIR', out_dir, 'NUM_GPUS', 1, 'TEST.DATASETS', '()',
                           'TEST.PROPOSAL_FILES', '()', 'NAWS.SYNTHETIC_TEST_IMAGES', 2,
                           'MODEL.NUM_CLASSES', 4])
    c.assert_and_infer_cfg()
    ab, asg, akp = te.empty_results(4, 2)
    f = os.path.join(out_dir, 'detections.pkl')
    te.save_detections(f, ab, asg, akp)
    wf = os.path.join(out_dir, 'model_final.pkl')
    save_object(dict(blobs={}, cfg=envu.yaml_dump(c.cfg, reference_format=True)), wf)
    return f, wf, bool(c.cfg.TEST.BBOX_AUG.ENABLED)


def main():
    with tempfile.TemporaryDirectory() as d:
        f, wf, aug = dumped_files(d)
        cfgs = [pickle.load(open(p, 'rb'))['cfg'].replace(d, OUTPUT_DIR).replace(ROOT, ROOT_DIR)
                for p in (f, wf)]
        assert cfgs[0] == cfgs[1]
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
        env.pop('PYTHONPATH', None)
        r = subprocess.run([sys.executable, '-c', CHILD % (HERE, f, wf)], capture_output=True,
                           text=True, env=env, cwd=d)
    assert r.returncode == 0, r.stderr[-2000:]
    out = dict(output_dir_placeholder=OUTPUT_DIR, root_dir_placeholder=ROOT_DIR, cfg=cfgs[0],
               bbox_aug_enabled=aug, reference_stdout=[l for l in r.stdout.splitlines() if l.strip()])
    with open(os.path.join(HERE, 'reference_cfg_load.json'), 'w') as fo:
        json.dump(out, fo, indent=1, sort_keys=True)
        fo.write('\n')
    print('\n'.join(out['reference_stdout']))


if __name__ == '__main__':
    main()
