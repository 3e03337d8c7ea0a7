"""One small bf16 train step of each benchmarked configuration (mv-3ddet, mv-grounding, mv-occ) with engine.GRAD_ROWS_BF16 off and on,
from the same seed: losses and the whole gradient arena are bit-equal.  With the switch off every es_norm_bwd launch is given f32 rows
and every residual join of the image backbone is an es_affine_act_bwd_yh launch, each downsample output one more; with it on the mv-3ddet
step issues es_norm_bwd launches without f32 rows (the K = 27 layers of the sparse backbone and the head's 3x3x3 convolutions), its 13 joins
are 10 es_affine_act_bwd_yh_xh and 3 es_affine_act_bwd_yh_xh2 launches (the downsample blocks), no es_affine_act_bwd_yh launch is left --
none on a downsample output -- and no es_cast_rows_bf16 is issued inside the backward of an image-backbone convolution (one whose input
rows are bf16 activations)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one_step(name, switch):
    from embodiedscan_amd import engine as E, pipeline
    from embodiedscan_amd.config import build_detector, build_optim_wrapper, load_config
    from embodiedscan_amd.synth import make_grounding_sample, make_occ_gt, make_scan
    dev = torch.device('cuda:0')
    cfg = load_config(os.path.join(ROOT, 'configs', name))
    det = build_detector(cfg, device=dev, seed=0).to(dev)
    optim = build_optim_wrapper(cfg)
    kind = cfg['model']['type']
    if kind == 'DenseFusionOccPredictor':
        sc = make_scan(900, n_views=2, augment=False, render_device=str(dev))
        batch = pipeline.make_occ_batch([pipeline.upload_scan(sc, dev)], [make_occ_gt(sc, seed=0)])
    else:
        scans = [make_scan(900 + i, n_views=2, height=120, width=160, img_size=(128, 128), n_points=12000) for i in range(2)]
        ds = [pipeline.upload_scan(s, dev) for s in scans]
        if kind == 'SparseFeatureFusion3DGrounder':
            batch = pipeline.make_grounding_batch(ds, [make_grounding_sample(s, seed=i) for i, s in enumerate(scans)])
        else:
            batch = pipeline.make_batch(ds)
    norm_dx, names, img_casts = [], [], []         # the dx argument of every es_norm_bwd launch; every entry point called; casts (below)
    real_call, real_bwd = E.call, E._conv_backward
    in_img = [0]

    def call(fn, *args):
        names.append(fn)
        if fn == 'es_norm_bwd':
            norm_dx.append(args[17])
        if fn == 'es_cast_rows_bf16' and in_img[0]:
            img_casts.append(args[2:4])
        return real_call(fn, *args)

    def conv_backward(x, *args, **kw):              # the backward of a convolution on bf16 activation rows: the image backbone's
        img = x.d.dtype == torch.bfloat16
        in_img[0] += img
        try:
            return real_bwd(x, *args, **kw)
        finally:
            in_img[0] -= img
    old = E.GRAD_ROWS_BF16[0], E.PRECISION[0], E.call, E._conv_backward
    E.GRAD_ROWS_BF16[0], E.PRECISION[0], E.call, E._conv_backward = switch, 'bf16', call, conv_backward
    try:
        losses = det.train_step(batch, optim)
        torch.cuda.synchronize()
    finally:
        E.GRAD_ROWS_BF16[0], E.PRECISION[0], E.call, E._conv_backward = old
    n = det.arena.n_train
    return {k: float(v) for k, v in losses.items()}, det.arena.grad[:n].clone(), norm_dx, names + ['image cast'] * len(img_casts)


@pytest.mark.parametrize('name', ['mv_3ddet.py', 'mv_grounding.py', 'mv_occ.py'])
def test_step_gradients_bit_equal_with_the_switch_off_and_on(name):
    l0, g0, dx0, n0 = _one_step(name, False)
    l1, g1, dx1, n1 = _one_step(name, True)
    lean = sum(1 for p in dx1 if p == 0)
    one, two = n1.count('es_affine_act_bwd_yh_xh'), n1.count('es_affine_act_bwd_yh_xh2')
    print(f'{name}: {len(dx1)} es_norm_bwd launches, {lean} without f32 rows; of {n0.count("es_affine_act_bwd_yh")} es_affine_act_bwd_yh '
          f'launches {one} joins with bf16 rows, {two} with two scales, {n1.count("es_affine_act_bwd_yh")} left; losses {l1}')
    assert all(np.isfinite(v) for v in l1.values()) and l0 == l1, (l0, l1)
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    assert torch.equal(g0.view(torch.int32), g1.view(torch.int32)), float((g0 - g1).abs().max())
    assert len(dx0) == len(dx1) > 0 and all(p != 0 for p in dx0)
    assert 'es_affine_act_bwd_yh_xh' not in n0 and 'es_affine_act_bwd_yh_xh2' not in n0
    assert n0.count('es_affine_act_bwd_yh') == n1.count('es_affine_act_bwd_yh') + one + 2 * two      # (a two-scale join stands for two launches)
    assert 'image cast' not in n1 and 'image cast' not in n0
    if name == 'mv_3ddet.py':                          # layers 2 - 4 of ResNet-50: 4 + 6 + 3 blocks, the first of each a downsample block
        assert lean > 0 and one == 10 and two == 3 and n1.count('es_affine_act_bwd_yh') == 0
