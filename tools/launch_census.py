"""Every call into libes_hip.so of two small bf16 train steps, and a hash of what they computed -- the before / after record of a host-side
refactor: two commits that print the same census queue the same entry points in the same order with the same scalar arguments and leave
the same bits in every loss, gradient and parameter.

    python tools/launch_census.py DIGEST.txt [CALLS.txt]        (run it at both commits, then `cmp` / `diff` the two files)

For mv_3ddet.py, mv_grounding.py and mv_occ.py (inputs and seed of tests/test_gpu_grad_rows_bf16_step.py::_one_step) with ES_GRAPHS=0, every
function of hip._fn wrapped -- launches and host queries alike.  CALLS.txt (when asked for; ~ 8 500 lines): one line per call with the entry's
name, every non-pointer argument by value and every pointer argument as 0 / * (null / non-null; the types are those of hip.PROTOS), then a SHA-256
over the two steps' losses, the gradient arena after step 2 and the parameters after step 2.  DIGEST.txt, the form that is kept under
profiles/: per configuration and step the number of calls and the SHA-256 of those lines, the calls per entry point, and the result hash --
equal digests mean equal call sequences; where they differ, `diff` the two CALLS files."""
import collections
import ctypes
import hashlib
import os
import sys
import textwrap

os.environ['ES_GRAPHS'] = '0'                       # (read when the engine is imported)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _batch(cfg, dev):
    from embodiedscan_amd import pipeline
    from embodiedscan_amd.synth import make_grounding_sample, make_occ_gt, make_scan
    kind = cfg['model']['type']
    if kind == 'DenseFusionOccPredictor':
        sc = make_scan(900, n_views=2, augment=False, render_device=str(dev))
        return pipeline.make_occ_batch([pipeline.upload_scan(sc, dev)], [make_occ_gt(sc, seed=0)])
    scans = [make_scan(900 + i, n_views=2, height=120, width=160, img_size=(128, 128), n_points=12000) for i in range(2)]
    ds = [pipeline.upload_scan(s, dev) for s in scans]
    if kind == 'SparseFeatureFusion3DGrounder':
        return pipeline.make_grounding_batch(ds, [make_grounding_sample(s, seed=i) for i, s in enumerate(scans)])
    return pipeline.make_batch(ds)


def census(name):
    from embodiedscan_amd import engine as E, hip
    from embodiedscan_amd.config import build_detector, build_optim_wrapper, load_config
    dev = torch.device('cuda:0')
    cfg = load_config(os.path.join(ROOT, 'configs', name))
    det = build_detector(cfg, device=dev, seed=0).to(dev)
    optim = build_optim_wrapper(cfg)
    batch = _batch(cfg, dev)
    real, lines = dict(hip._fn), []

    def wrap(fn_name, fn):
        is_ptr = [t is ctypes.c_void_p for t in hip.PROTOS[fn_name][1]]

        def f(*args):
            lines.append(fn_name + ' ' + ' '.join(('*' if a else '0') if p else repr(a) for a, p in zip(args, is_ptr)))
            return fn(*args)
        return f
    old = E.PRECISION[0]
    E.PRECISION[0] = 'bf16'
    hip._fn.update({k: wrap(k, v) for k, v in real.items()})
    h = hashlib.sha256()
    try:
        for step in range(2):
            lines.append(f'# {name} step {step + 1}')
            losses = det.train_step(batch, optim)
            torch.cuda.synchronize()
            h.update(repr(sorted((k, float(v)) for k, v in losses.items())).encode())
    finally:
        hip._fn.update(real)
        E.PRECISION[0] = old
    for t in (det.arena.grad[:det.arena.n_train], det.arena.data):
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return lines, h.hexdigest()


def digest(name, lines, result):
    """the short form of one configuration's census: per step the number of calls and the SHA-256 of their lines, the calls per entry point
    over both steps, the hash of the results"""
    cut = [i for i, ln in enumerate(lines) if ln.startswith('#')] + [len(lines)]
    out = [f'# {name}: {len(lines) - 2} calls']
    for k in range(2):
        part = lines[cut[k] + 1:cut[k + 1]]
        out.append(f'step {k + 1}: {len(part)} calls, sha256 of their lines {hashlib.sha256(chr(10).join(part).encode()).hexdigest()}')
    count = collections.Counter(ln.split(' ', 1)[0] for ln in lines if not ln.startswith('#'))
    out += textwrap.wrap(', '.join(f'{k} x {v}' for k, v in sorted(count.items())), 150, initial_indent='calls: ', subsequent_indent='  ')
    return out + [f'losses, gradient arena and parameters: sha256 {result}']


if __name__ == '__main__':
    calls = open(sys.argv[2], 'w') if len(sys.argv) > 2 else None
    with open(sys.argv[1], 'w') as out:
        for cfg_name in ('mv_3ddet.py', 'mv_grounding.py', 'mv_occ.py'):
            lines, result = census(cfg_name)
            out.write('\n'.join(digest(cfg_name, lines, result)) + '\n')
            if calls is not None:
                calls.write('\n'.join(lines) + f'\n# {cfg_name} sha256 {result}\n')
