"""Generate tests/golden/reference_cont_det_config.json from the REFERENCE's continuous detection configuration.

    python tools/make_golden_cont_det_config.py <reference checkout>

configs/detection/cont-det3d_*.py is read unchanged by embodiedscan_amd.config.load_config; the fixture keeps the settings
tests/test_cont_det_host.py compares configs/cont_det3d.py with and builds from: the `model`, `optim_wrapper`, `train_pipeline` and
`test_pipeline` sections, keyed by the file's path under configs/.  Settings only.  (tests/golden/reference_configs.json stays the
`mv-*` set and reference_cont_configs.json the cont-occ one.)
TEST INFRASTRUCTURE."""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(reference_root, out_dir=None):
    sys.path.insert(0, ROOT)
    from embodiedscan_amd.config import load_config
    ref = os.path.join(reference_root, 'configs')
    configs = {}
    for p in sorted(glob.glob(os.path.join(ref, 'detection', 'cont-*.py'))):
        cfg = load_config(p)
        configs[os.path.relpath(p, ref)] = {k: cfg[k] for k in ('model', 'optim_wrapper', 'train_pipeline', 'test_pipeline')}
    assert configs, f'no cont-* detection configuration under {ref}'
    path = os.path.join(out_dir or os.path.join(ROOT, 'tests', 'golden'), 'reference_cont_det_config.json')
    with open(path, 'w') as f:
        json.dump(dict(what='model, optim_wrapper and pipeline sections of the reference cont-det3d configuration, as load_config reads them',
                       configs=configs), f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'wrote {len(configs)} configuration(s) to {path}')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit('usage: python tools/make_golden_cont_det_config.py <reference checkout>')
    main(sys.argv[1])
