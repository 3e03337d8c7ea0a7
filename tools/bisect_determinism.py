"""Which launch makes the grounding step differ between two detector builds in one process?    Builds the grounder
twice from the same seed, runs the loss forward (+ backward) on the same batch, and compares -- in creation order -- a bit checksum of
every engine Var (outputs and gradients), of the frozen text encoder's features and of the losses.  Prints the first difference with the
Python call sites that created it.   python tools/bisect_determinism.py [mv_grounding.py|mv_3ddet.py] [--backward]"""
import os
import sys
import traceback
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from embodiedscan_amd import engine as E, pipeline
from embodiedscan_amd.config import build_detector, load_config
from embodiedscan_amd.synth import make_grounding_sample, make_scan

name = next((a for a in sys.argv[1:] if a.endswith('.py')), 'mv_grounding.py')
backward = '--backward' in sys.argv
dev = torch.device('cuda:0')
cfg = load_config(os.path.join(ROOT, 'configs', name))
scans = [make_scan(900 + i, n_views=4, height=240, width=320, img_size=(256, 256), n_points=30000) for i in range(2)]
anns = [make_grounding_sample(s, seed=i) for i, s in enumerate(scans)]
E.PRECISION[0] = 'bf16'


def bits(t):
    if t is None:
        return None
    t = t.contiguous()
    v = t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int64)
    return (tuple(t.shape), int(v.to(torch.int64).sum().item()), int((v.to(torch.int64) * (torch.arange(v.numel(), device=v.device).reshape(v.shape) % 1021 + 1)).sum().item()))


def run():
    created = []
    orig = E.Var.__init__

    def spy(self, d, rg=True):
        orig(self, d, rg)
        fr = traceback.extract_stack(limit=7)[:-1]
        created.append((self, ' < '.join(f'{os.path.basename(f.filename)}:{f.lineno}:{f.name}' for f in reversed(fr))))
    E.Var.__init__ = spy
    try:
        det = build_detector(cfg, device=dev, seed=0).to(dev)
        ds = [pipeline.upload_scan(s, dev) for s in scans]
        batch = pipeline.make_grounding_batch(ds, anns) if 'grounding' in name else pipeline.make_batch(ds)
        E.TAPE.clear()
        data = det.data_preprocessor(batch, True)
        det._bind()
        det.arena.grad.zero_()
        E.new_grad_epoch()
        losses = det.forward(data['inputs'], data['data_samples'], mode='loss')
        torch.cuda.synchronize()
        rec = [('loss ' + k, bits(v.reshape(1) if torch.is_tensor(v) else torch.tensor([float(v)]))) for k, v in losses.items()]
        if hasattr(det, 'last_text'):
            rec.append(('text hidden', bits(det.last_text['hidden'])))
        fwd = [(site, bits(v.d)) for v, site in created]
        grads = []
        if backward:
            det._backward(None)
            torch.cuda.synchronize()
            grads = [(site, bits(v.g)) for v, site in created]
            rec.append(('arena grad', bits(det.arena.grad[:det.arena.n_train])))
        E.TAPE.clear()
        E.join_wgrad_streams()
        E.release(id(det))
        return rec, fwd, grads
    finally:
        E.Var.__init__ = orig


a, b = run(), run()
ok = True
for what, (x, y) in (('summary', (a[0], b[0])), ('forward Vars', (a[1], b[1])), ('gradients', (a[2], b[2]))):
    print(f'--- {what}: {len(x)} records')
    if len(x) != len(y):
        print(f'    DIFFERENT COUNTS {len(x)} vs {len(y)}')
    shown = 0
    for i, ((s1, h1), (s2, h2)) in enumerate(zip(x, y)):
        if h1 != h2:
            ok = False
            if shown < 6:
                print(f'    #{i} DIFFERS  {h1} vs {h2}\n       {s1}')
            shown += 1
    print(f'    {shown} records differ')
print('bit-identical across builds' if ok else 'NOT bit-identical across builds')
