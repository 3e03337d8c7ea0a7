"""Generate tests/golden/reference_configs.json from the REFERENCE's `mv-*` configuration files.

Run where a reference checkout is available:   python -m oracle.make_golden_configs <reference checkout>
Every configs/{detection,grounding,occupancy}/mv-*.py is read unchanged by embodiedscan_amd.config.load_config (the
reference's `_base_` chains included); the fixture keeps what tests/test_configs.py compares and builds from: the `model`
and `optim_wrapper` sections of each file, keyed by its path under configs/.  TEST INFRASTRUCTURE.
"""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(reference_root, out_dir=None):
    sys.path.insert(0, ROOT)
    from embodiedscan_amd.config import load_config
    ref = os.path.join(reference_root, 'configs')
    out_dir = out_dir or os.path.join(ROOT, 'tests', 'golden')
    configs = {}
    for sub in ('detection', 'grounding', 'occupancy'):
        for p in sorted(glob.glob(os.path.join(ref, sub, 'mv-*.py'))):
            cfg = load_config(p)
            configs[os.path.relpath(p, ref)] = dict(model=cfg['model'], optim_wrapper=cfg['optim_wrapper'])
    assert configs, f'no mv-* configurations under {ref}'
    path = os.path.join(out_dir, 'reference_configs.json')
    with open(path, 'w') as f:
        json.dump(dict(what='model and optim_wrapper sections of the reference mv-* configurations, as load_config reads them',
                       configs=configs), f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'wrote {len(configs)} configurations to {path}')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit('usage: python -m oracle.make_golden_configs <reference checkout>')
    main(sys.argv[1])
