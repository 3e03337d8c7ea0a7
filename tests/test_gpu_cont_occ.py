"""EmbodiedOccPredictor (continuous occupancy: one prediction per prefix of the frames) on the MI355X against the composed CPU
specification tests/cont_occ_spec.py, at the `_small_cfg` scale of tests/test_gpu_occ.py (base 16, FPN 32, 8 x 8 x 4 voxels, true
3-D widths) with T = 4 views.  The arithmetic is that of DenseFusionOccPredictor over a T-fold batch, so the f32 tolerances are those
of test_occ_detector_train_step_vs_oracle (logits 1e-4, losses 1e-4, parameter gradients median 1e-3 / worst 5e-2 relative L2) and
the bf16 loss tolerance its 2e-2.  No emulated case: the emulator carries kernels and tape operators, not a whole detector step
(its image backbone alone would take hours there); the two new kernels run on it in tests/test_emu_prefix_fusion.py."""
import os

import numpy as np
import pytest
import torch

import cont_occ_spec as CS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _rows(t):
    """(T, C, X, Y, Z) -> channels-last rows (T*X*Y*Z, C), prefix-major"""
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1]).contiguous()


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _small_cfg(fpn_out=32, base=16, n_voxels=(8, 8, 4), name='cont_occ.py'):
    from embodiedscan_amd.config import load_config
    cfg = load_config(os.path.join(ROOT, 'configs', name))
    m = cfg['model']
    m['backbone']['base_channels'] = base
    m['neck'].update(in_channels=[4 * base, 8 * base, 16 * base, 32 * base], out_channels=fpn_out)
    m['neck_3d']['in_channels'] = fpn_out + 512
    m['n_voxels'] = list(n_voxels)
    return cfg


def _sweep_scan(cfg, seed, T):
    """a synthetic scan in the form ScanPipeline(sweeps=True) hands over: the chosen pixels in frame order, the slice indices, one
    cumulative visibility mask per prefix"""
    from embodiedscan_amd.synth import make_occ_gt, make_scan
    scan = make_scan(seed, n_views=T, height=120, width=160, img_size=(128, 128), n_points=20000, n_boxes=10, augment=False)
    order = np.argsort(scan['sel_view'], kind='stable')
    scan['sel_view'], scan['sel_pix'] = scan['sel_view'][order], scan['sel_pix'][order]
    scan['points_slice_indices'] = [0] + np.cumsum(np.bincount(scan['sel_view'], minlength=T)).tolist()
    occ = make_occ_gt(scan, n_voxels=cfg['model']['n_voxels'], prior_range=cfg['prior_generator']['ranges'][0], seed=seed)
    rng = np.random.default_rng(seed)
    seen = rng.random(occ['gt_occupancy_masks'].shape)
    occ['gt_occupancy_masks'] = [occ['gt_occupancy_masks'] & (seen < (t + 1) / T) for t in range(T)]     # grows with t
    return scan, occ


def _case(dev, cfg, seed=21, T=4):
    from embodiedscan_amd import pipeline
    from embodiedscan_amd.config import build_detector
    det = build_detector(cfg, device=dev, seed=0).to(dev)
    scan, occ = _sweep_scan(cfg, seed, T)
    return det, scan, occ, pipeline.upload_scan(scan, dev)


def _spec_args(cfg, scan):
    from oracle import model as OM
    m = cfg['model']
    imgs = OM.preprocess_img(torch.from_numpy(scan['img']), MEAN, STD)[None]
    return imgs, (scan['meta'], m['n_voxels'], m['point_cloud_range'], cfg['prior_generator']['ranges'][0])


def _step(det, dscan, occ, backward=True):
    from embodiedscan_amd import engine as E, pipeline
    E.WEIGHT_VERSION[0] += 1
    E.TAPE.clear()
    batch = pipeline.make_cont_occ_batch(dscan, occ)
    points_host = [p.cpu() for p in batch['inputs']['points']]
    data = det.data_preprocessor(batch, True)
    det._bind()
    det.arena.grad.zero_()
    losses = det.forward(data['inputs'], data['data_samples'], mode='loss')
    if backward:
        E.TAPE.backward()
    else:
        E.TAPE.clear()
        E.join_wgrad_streams()
    torch.cuda.synchronize()
    return losses, points_host, data


def test_cont_occ_train_step_vs_composed_spec(dev):
    """f32: voxel coordinates per prefix and supervision targets bit exact, logits 1e-4, losses 1e-4, parameter gradients median 1e-3 /
    worst 5e-2 relative L2 (the tolerances of test_occ_detector_train_step_vs_oracle: the same arithmetic over a T-fold batch).
    bf16: losses within 2e-2 of the f32 spec, every gradient finite."""
    from embodiedscan_amd import engine as E, sparse
    cfg = _small_cfg()
    T = 4
    det, scan, occ, dscan = _case(dev, cfg, T=T)
    sd = {k: v.cpu() for k, v in det.state_dict().items()}
    names = set(det.arena.grad_dict().keys())
    osd = {k: v.clone().requires_grad_(k in names) for k, v in sd.items()}
    res = {}
    try:
        for mode in ('f32', 'bf16'):
            E.PRECISION[0] = mode
            losses, points_host, data = _step(det, dscan, occ)
            assert len(data['data_samples']) == T and [len(p) for p in points_host] == scan['points_slice_indices'][1:]
            res[mode] = dict(losses={k: float(v) for k, v in losses.items()}, logits=[l['logits'].d.cpu() for l in det.bbox_head.last],
                             gt=[l['gt'].cpu() for l in det.bbox_head.last], grads={k: v.cpu() for k, v in det.arena.grad_dict().items()})
    finally:
        E.PRECISION[0] = 'f32'
    imgs, args = _spec_args(cfg, scan)
    # voxel coordinates of every prefix: the detector's voxelisation call on the T clouds against the spec's, as sets per prefix
    pts_dev = [p.to(dev) for p in points_host]
    cs, _ = sparse.voxelize_range(pts_dev, det.point_cloud_range[:3], det.voxel_size, [n * det.voxel_stride - 1 for n in det.n_voxels])
    want, _ = CS.voxel_coords(points_host, *args[1:])
    got = cs.coords[:cs.n].cpu().numpy()
    assert got.shape == want.shape
    key = lambda c: c[np.lexsort((c[:, 3], c[:, 2], c[:, 1], c[:, 0]))]     # noqa: E731
    np.testing.assert_array_equal(key(got), key(want))
    per_prefix = np.bincount(want[:, 0], minlength=T)
    assert (np.diff(per_prefix) >= 0).all() and per_prefix[0] > 0, 'the clouds are cumulative'
    ol, aux = CS.detector_loss(osd, points_host, imgs, args[0], torch.from_numpy(occ['gt_occupancy']),
                               [torch.from_numpy(m) for m in occ['gt_occupancy_masks']], *args[1:])
    sum(ol.values()).backward()
    for i in range(3):
        np.testing.assert_array_equal(res['f32']['gt'][i].numpy(), aux['parts'][i][3].reshape(-1).numpy())
        e = _rel(res['f32']['logits'][i], _rows(aux['preds'][i].detach()))
        print(f'f32 cont-occ logits level {i}: rel-L2 {e:.2e} (tol 1e-4)')
        assert e < 1e-4
    for mode, tl in (('f32', 1e-4), ('bf16', 2e-2)):
        for k in ol:
            want = float(ol[k].detach())
            e = abs(res[mode]['losses'][k] - want) / abs(want)
            print(f'{mode} {k}: hip {res[mode]["losses"][k]:.6f} spec {want:.6f} rel err {e:.2e} (tol {tl:.0e})')
            assert e < tl
    rel = {k: _rel(v, osd[k].grad) for k, v in res['f32']['grads'].items() if osd[k].grad is not None and float(osd[k].grad.norm()) > 1e-10}
    worst = max(rel, key=rel.get)
    med = float(np.median(list(rel.values())))
    print(f'f32 parameter gradients vs spec autograd: {len(rel)} tensors, median rel-L2 {med:.2e} (tol 1e-3), worst {rel[worst]:.2e} at {worst} (tol 5e-2)')
    assert any(k.startswith('neck.') for k in rel) and any(k.startswith('backbone.') for k in rel), 'the image branch receives gradients'
    assert med < 1e-3 and rel[worst] < 5e-2
    assert all(bool(torch.isfinite(g).all()) for g in res['bf16']['grads'].values())


def test_cont_occ_predict_one_occupancy_per_prefix(dev):
    """mode='predict' attaches an (X, Y, Z) int64 pred_occupancy to each of the T samples, equal to the spec's arg-max on every voxel
    whose spec top-1 / top-2 logit margin exceeds twice the largest logit error measured in the same run; at most half of the voxels
    may be excused that way.  The spec alone (f32 against f64 on the CPU, seed 21, T = 4): largest logit error 2.2e-5 at logits up to
    21, 98.8 % of the voxels have a margin above twice that, 79 % above 2e-3."""
    from embodiedscan_amd import engine as E, pipeline
    cfg = _small_cfg()
    T = 4
    det, scan, occ, dscan = _case(dev, cfg, T=T)
    sd = {k: v.cpu() for k, v in det.state_dict().items()}
    E.TAPE.clear()
    batch = pipeline.make_cont_occ_batch(dscan, occ)
    points_host = [p.cpu() for p in batch['inputs']['points']]
    data = det.data_preprocessor(batch, False)
    det._bind()
    with det._predict_guard():                            # the logits behind the prediction, for the error measurement
        x = det.extract_feat(data['inputs'], data['data_samples'])
        logits = det.bbox_head.forward(x[:1])[0][0].d.cpu()
    out = det.forward(data['inputs'], data['data_samples'], mode='predict')
    torch.cuda.synchronize()
    imgs, args = _spec_args(cfg, scan)
    with torch.no_grad():
        ref = CS.detector_forward(sd, points_host, imgs, *args, training=False)[0]          # (T, C, X, Y, Z)
    X, Y, Z = cfg['model']['n_voxels']
    assert len(out) == T
    err = float((logits.double() - _rows(ref).double()).abs().max())
    top2 = ref.topk(2, dim=1).values
    held = (top2[:, 0] - top2[:, 1]) > 2 * err
    want = ref.argmax(1)
    share = float(held.float().mean())
    print(f'predict: largest logit error {err:.2e} (logits up to {float(ref.abs().max()):.1f}); {share:.1%} of {held.numel()} voxels have a '
          f'margin above twice that')
    assert share >= 0.5, 'more than half of the voxels would be excused by the margin rule'
    for t, ds in enumerate(out):
        p = ds.pred_occupancy.cpu()
        assert p.shape == (X, Y, Z) and p.dtype == torch.int64
        assert torch.equal(p[held[t]], want[t][held[t]]), f'prefix {t}: arg-max differs on a voxel whose margin exceeds twice the logit error'
    assert any(not torch.equal(out[0].pred_occupancy, out[t].pred_occupancy) for t in range(1, T)), 'every prefix got the same prediction'


def test_one_prefix_is_dense_fusion_occ_bit_for_bit(dev):
    """T = 1: losses and parameter gradients are bit-equal to DenseFusionOccPredictor on the same scan and weights"""
    from embodiedscan_amd import engine as E, pipeline
    from embodiedscan_amd.config import build_detector
    cfg = _small_cfg()
    det, scan, occ, dscan = _case(dev, cfg, seed=23, T=1)
    ref = build_detector(_small_cfg(name='mv_occ.py'), device=dev, seed=0).to(dev)
    assert torch.equal(ref.arena.data, det.arena.data)                  # (before a training forward moves the running statistics)
    losses, _, _ = _step(det, dscan, occ)
    la, ga = {k: float(v) for k, v in losses.items()}, det.arena.grad.clone()
    E.WEIGHT_VERSION[0] += 1
    E.TAPE.clear()
    data = ref.data_preprocessor(pipeline.make_occ_batch([dscan], [dict(occ, gt_occupancy_masks=occ['gt_occupancy_masks'][0])]), True)
    ref._bind()
    ref.arena.grad.zero_()
    lb = ref.forward(data['inputs'], data['data_samples'], mode='loss')
    E.TAPE.backward()
    torch.cuda.synchronize()
    assert la == {k: float(v) for k, v in lb.items()}, (la, lb)
    assert torch.equal(ga, ref.arena.grad) and float(ga.abs().sum()) > 0


def test_cont_occ_full_width(dev):
    """the shipped widths (ResNet-50 base 64, FPN 256, neck 768 -> 1536 -> 3072) on 8 x 8 x 4 voxels, T = 3: every loss and gradient
    finite, bf16 losses within 2e-2 of the f32 spec"""
    from embodiedscan_amd import engine as E
    cfg = _small_cfg(fpn_out=256, base=64)
    det, scan, occ, dscan = _case(dev, cfg, seed=22, T=3)
    sd = {k: v.cpu() for k, v in det.state_dict().items()}
    E.PRECISION[0] = 'bf16'
    try:
        losses, points_host, _ = _step(det, dscan, occ)
    finally:
        E.PRECISION[0] = 'f32'
    assert bool(torch.isfinite(det.arena.grad).all())
    imgs, args = _spec_args(cfg, scan)
    with torch.no_grad():
        ol, _ = CS.detector_loss(sd, points_host, imgs, args[0], torch.from_numpy(occ['gt_occupancy']),
                                 [torch.from_numpy(m) for m in occ['gt_occupancy_masks']], *args[1:])
    for k in ol:
        a = float(losses[k])
        e = abs(a - float(ol[k])) / abs(float(ol[k]))
        print(f'full-width bf16 {k}: hip {a:.6f} spec {float(ol[k]):.6f} rel err {e:.2e} (tol 2e-2)')
        assert np.isfinite(a) and e < 2e-2
