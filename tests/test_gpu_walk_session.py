"""Walk sessions (EmbodiedOccPredictor.open_walk / Embodied3DDetector.open_walk: frame in, prediction out) on the MI355X against the
existing batch path on the whole walk, at the scales of tests/test_gpu_cont_occ.py (FPN width 32, 8 x 8 x 4 voxels, seed 21, T = 4,
128 x 128 images, 20 000 points) and tests/test_gpu_cont_det.py (_sweep_scan(44, 3), randomised statistics, nms_pre 300 / iou 0.5 /
score 0.09).

Occupancy, per prefix t: walk.logits against the batch logits, relative L2 <= 1e-4 (the f32 logits tolerance of
test_cont_occ_train_step_vs_composed_spec); pred_occupancy equal on every voxel whose top-1 / top-2 margin in the batch logits exceeds
twice the largest logit difference of the run, with at most half of the voxels excused (the cap of
test_cont_occ_predict_one_occupancy_per_prefix).  Detection, per prefix t: test_gpu_cont_det._same against mode='predict' (labels equal,
scores rtol 2e-5 / atol 1e-7, boxes rtol 3e-4 / atol 2e-4), more than 20 detections in total.  Protocol of both: reset, stale weights,
restored flags, max_frames.  The batch references are computed once per module."""
import pytest
import torch

import test_gpu_cont_det as CD
import test_gpu_cont_occ as CO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _frames(dscan, cloud):
    from embodiedscan_amd import pipeline
    return [(t, cloud[r0:r1], dict(extrinsic=e, intrinsic=i)) for t, (r0, r1), e, i in pipeline.walk_frames(dscan, cloud.shape[0])]


def _const_meta(metainfo):
    """what is constant over the walk: everything but the per-frame matrices"""
    d2i = metainfo['depth2img']
    return dict(metainfo, depth2img={k: v for k, v in d2i.items() if k not in ('extrinsic', 'intrinsic')})


# ------------------------------------------------------------------ occupancy
@pytest.fixture(scope='module')
def occ(dev):
    """the detector, the walk's inputs and the batch path's logits / predictions on the whole walk (computed once, left unchanged)"""
    from embodiedscan_amd import engine as E, pipeline
    cfg = CO._small_cfg()
    T = 4
    det, scan, occ_gt, dscan = CO._case(dev, cfg, seed=21, T=T)
    E.TAPE.clear()
    batch = pipeline.make_cont_occ_batch(dscan, occ_gt)
    cloud = batch['inputs']['points'][-1]
    data = det.data_preprocessor(batch, False)
    imgs = data['inputs']['imgs'].clone()                  # (the preprocessor's buffers are a ring)
    det._bind()
    with det._predict_guard():
        x = det.extract_feat(data['inputs'], data['data_samples'])
        logits = det.bbox_head.forward(x[:1])[0][0].d.clone()
    out = det.forward(data['inputs'], data['data_samples'], mode='predict')
    torch.cuda.synchronize()
    pred = [ds.pred_occupancy.clone() for ds in out]
    X, Y, Z = cfg['model']['n_voxels']
    return dict(det=det, T=T, imgs=imgs, frames=_frames(dscan, cloud), meta=_const_meta(data['data_samples'][0].metainfo),
                logits=logits.view(T, X * Y * Z, -1), pred=pred, dims=(X, Y, Z))


def _occ_pass(walk, c):
    res = []
    for t, rows, d2i in c['frames']:
        p = walk.observe(c['imgs'][0, t], rows, d2i)
        res.append((p.clone(), walk.logits.clone()))
    torch.cuda.synchronize()
    return res


def test_occ_walk_equals_the_batch_path_per_prefix(occ):
    c = occ
    walk = c['det'].open_walk(c['meta'])
    res = _occ_pass(walk, c)
    assert walk.t == c['T'] and walk.state_bytes() > 0
    diff = max(float((l.double() - c['logits'][t].double()).abs().max()) for t, (_, l) in enumerate(res))
    bit = all(torch.equal(l, c['logits'][t]) for t, (_, l) in enumerate(res))
    print(f'occupancy walk: largest logit difference to the batch path {diff:.3e}; logits bit-equal: {bit}')
    held_n = tot = 0
    for t, (p, l) in enumerate(res):
        ref = c['logits'][t]
        e = CO._rel(l, ref)
        print(f'  prefix {t}: logits rel-L2 {e:.2e} (tol 1e-4)')
        assert e <= 1e-4
        top2 = ref.topk(2, dim=1).values
        held = ((top2[:, 0] - top2[:, 1]) > 2 * diff).view(c['dims'])
        held_n, tot = held_n + int(held.sum()), tot + held.numel()
        assert p.shape == c['dims'] and p.dtype == torch.int64
        assert torch.equal(p[held], c['pred'][t][held]), f'prefix {t}: arg-max differs on a voxel whose margin exceeds twice the logit difference'
    print(f'  {held_n / tot:.1%} of {tot} voxels have a margin above twice that')
    assert held_n / tot >= 0.5, 'more than half of the voxels would be excused by the margin rule'
    assert any(not torch.equal(res[0][0], res[t][0]) for t in range(1, c['T'])), 'every prefix got the same prediction'


def test_occ_walk_protocol(occ):
    from embodiedscan_amd import engine as E
    c, det = occ, occ['det']
    walk = det.open_walk(c['meta'])
    first = _occ_pass(walk, c)
    walk.reset()
    assert walk.t == 0 and walk.logits is None
    E.TAPE.clear()
    det.train(True)
    E.TAPE.enabled = True
    second = []
    for t, rows, d2i in c['frames']:
        if t == 2:                                         # weights moved between two observes: refused, the state stays
            old = E.WEIGHT_VERSION[0]
            E.WEIGHT_VERSION[0] += 1
            try:
                with pytest.raises(ValueError, match='stale'):
                    walk.observe(c['imgs'][0, t], rows, d2i)
            finally:
                E.WEIGHT_VERSION[0] = old
            assert walk.t == 2
        p = walk.observe(c['imgs'][0, t], rows, d2i)
        assert det.training and E.TAPE.enabled and len(E.TAPE.fns) == 0, 'training flag / tape not restored, or something was recorded'
        second.append((p.clone(), walk.logits.clone()))
    torch.cuda.synchronize()
    for t, ((p0, l0), (p1, l1)) in enumerate(zip(first, second)):
        assert torch.equal(p0, p1) and torch.equal(l0, l1), f'prefix {t}: the pass after reset() is not bit-equal to the first'
    with pytest.raises(ValueError, match='walk on'):
        walk.observe(c['imgs'][0, 0].cpu(), c['frames'][0][1], c['frames'][0][2])
    assert walk.t == c['T']


# ------------------------------------------------------------------ detection
@pytest.fixture(scope='module')
def det3d(dev):
    from embodiedscan_amd import pipeline
    T = 3
    det = CD._build(dev)
    CD._randomise_statistics(det, dev, seed=2)
    det.bbox_head.test_cfg = dict(nms_pre=300, iou_thr=0.5, score_thr=0.09)     # top-k selection and NMS really run on random-init scores
    scan = CD._sweep_scan(44, T)
    dscan = pipeline.upload_scan(scan, dev)
    batch = pipeline.make_cont_det_batch(dscan)
    cloud = batch['inputs']['points'][-1]
    data = det.data_preprocessor(batch, False)
    imgs = data['inputs']['imgs'].clone()
    out = det.forward(data['inputs'], data['data_samples'], mode='predict')
    torch.cuda.synchronize()
    return dict(det=det, T=T, imgs=imgs, frames=_frames(dscan, cloud), meta=_const_meta(data['data_samples'][0].metainfo), ref=CD._dets(out))


def _inst(r):
    return r.bboxes_3d.tensor.clone(), r.scores_3d.clone(), r.labels_3d.clone()


def _det_pass(walk, c, upto=None):
    res = [_inst(walk.observe(c['imgs'][0, t], rows, d2i)) for t, rows, d2i in c['frames'][:upto]]
    torch.cuda.synchronize()
    return res


def test_det_walk_equals_predict_per_prefix(det3d):
    c = det3d
    walk = c['det'].open_walk(c['meta'], max_frames=c['T'])
    res = _det_pass(walk, c)
    n_det = 0
    for t, r in enumerate(res):
        got = tuple(a.cpu().numpy() for a in r)
        print(f'prefix {t}: {len(got[1])} detections (walk), {len(c["ref"][t][1])} (predict on the whole walk)')
        CD._same(got, c['ref'][t], f'prefix {t}: the walk session against mode=predict')
        n_det += len(got[1])
    assert n_det > 20
    assert walk.t == c['T'] and walk.state_bytes() > 0


def test_det_walk_protocol(det3d):
    from embodiedscan_amd import engine as E
    c, det = det3d, det3d['det']
    with pytest.raises(ValueError, match='max_frames'):
        det.open_walk(c['meta'], max_frames=65)
    walk = det.open_walk(c['meta'], max_frames=2)
    first = _det_pass(walk, c, upto=2)
    maps = [m.clone() for m, _, _ in walk.maps]
    n_rows = walk.cloud.n
    t, rows, d2i = c['frames'][2]
    with pytest.raises(ValueError, match='max_frames'):    # past max_frames: refused before any launch, frame 2's state intact
        walk.observe(c['imgs'][0, t], rows, d2i)
    assert walk.t == 2 and walk.cloud.n == n_rows and len(walk.meta) == 2
    assert all(torch.equal(a, m) for a, (m, _, _) in zip(maps, walk.maps))
    walk.reset()
    E.TAPE.clear()
    det.train(True)
    E.TAPE.enabled = True
    second = []
    for t, rows, d2i in c['frames'][:2]:
        if t == 1:                                         # weights moved between two observes: refused, the state stays
            old = E.WEIGHT_VERSION[0]
            E.WEIGHT_VERSION[0] += 1
            try:
                with pytest.raises(ValueError, match='stale'):
                    walk.observe(c['imgs'][0, t], rows, d2i)
            finally:
                E.WEIGHT_VERSION[0] = old
            assert walk.t == 1 and len(walk.meta) == 1
        second.append(_inst(walk.observe(c['imgs'][0, t], rows, d2i)))
        assert det.training and E.TAPE.enabled and len(E.TAPE.fns) == 0, 'training flag / tape not restored, or something was recorded'
    torch.cuda.synchronize()
    for t, (a, b) in enumerate(zip(first, second)):
        assert all(torch.equal(x, y) for x, y in zip(a, b)), f'prefix {t}: the pass after reset() is not bit-equal to the first'
    assert sum(len(a[1]) for a in first) > 0
