"""embodiedscan_amd.inference on the MI355X: a demo folder of 4 frames at 60 x 80 (synth.write_demo_scene) through run_scene, walk_scene
and the command line, on the small settings of tests/test_gpu_walk_session.py (cont-det3d: randomised statistics, nms_pre 300 / iou 0.5 /
score 0.09; cont-occ: FPN width 32, 8 x 8 x 4 voxels; 128 x 128 images, 2000 points per frame) and seeded random weights.  The filter's
score threshold is the median score of the run, so that rows fall on both sides of it.  Each detector and each by-hand reference is
made once per module."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_cont_det as CD
import test_gpu_cont_occ as CO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_CFG = dict(nms_pre=300, iou_thr=0.5, score_thr=0.09)
SEED = 5


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def demo(tmp_path_factory):
    from embodiedscan_amd.synth import write_demo_scene
    root = str(tmp_path_factory.mktemp('demo'))
    write_demo_scene(root, 'room', n_frames=4, height=60, width=80, seed=3)
    return root


def _small_pipeline(cfg):
    from embodiedscan_amd import inference as I
    pipe = copy.deepcopy(I.pipeline_of(cfg))
    for t in pipe:
        if t['type'] == 'MultiViewPipeline':
            t['n_images'] = 4
            for u in t['transforms']:
                if u['type'] == 'PointSample':
                    u['num_points'] = 2000
                elif u['type'] == 'Resize':
                    u['scale'] = (128, 128)
        elif t['type'] == 'PointSample':
            t['num_points'] = 6000
    return pipe


def _scan(det, demo, pipe):
    """the folder on the device, by hand: scene_info -> ScanPipeline -> upload_scan"""
    from embodiedscan_amd import inference as I, pipeline
    from embodiedscan_amd.datasets.loading import ScanPipeline
    scan = ScanPipeline.from_cfg(pipe)(I.scene_info(os.path.join(demo, 'room')), np.random.RandomState(SEED))
    return pipeline.upload_scan(scan, det.device)


def _split(scores):
    """a score threshold with rows on both sides"""
    thr = float(scores.float().median())
    assert bool((scores < thr).any()) and bool((scores >= thr).any())
    return thr


def _same_instances(a, b, what):
    assert torch.equal(a.keep, b.keep), f'{what}: kept rows differ'
    assert torch.equal(a.bboxes_3d.tensor, b.bboxes_3d.tensor) and torch.equal(a.scores_3d, b.scores_3d) and torch.equal(a.labels_3d, b.labels_3d), what


# ------------------------------------------------------------------------------------------------------------------ mv-3ddet
def test_run_scene_equals_filter_instances_on_predict(dev, demo):
    from embodiedscan_amd import inference as I, pipeline
    from embodiedscan_amd.config import load_config
    cfg = load_config(os.path.join(ROOT, 'configs', 'mv_3ddet.py'))
    det, _ = I.init_model(cfg, device=dev)
    assert not det.training
    CD._randomise_statistics(det, dev, seed=2)
    det.bbox_head.test_cfg = dict(TEST_CFG)
    pipe = _small_pipeline(cfg)
    data = det.data_preprocessor(pipeline.make_batch([_scan(det, demo, pipe)]), False)
    hand = det.forward(data['inputs'], data['data_samples'], mode='predict')[0].pred_instances_3d
    n = len(hand.scores_3d)
    raw = I.run_scene(det, os.path.join(demo, 'room'), pipe, seed=SEED, filter=None)
    assert len(raw) == 1 and torch.equal(raw[0].bboxes_3d.tensor, hand.bboxes_3d.tensor) and torch.equal(raw[0].scores_3d, hand.scores_3d)
    assert torch.equal(raw[0].labels_3d, hand.labels_3d) and n > 20
    flt = dict(iou_thr=0.15, score_thr=_split(hand.scores_3d), topk_per_class=2)
    got = I.run_scene(det, os.path.join(demo, 'room'), pipe, seed=SEED, filter=flt)
    want = I.filter_instances(hand, n_classes=det.bbox_head.num_classes, **flt)
    _same_instances(got[0], want, 'run_scene against filter_instances(predict)')
    print(f'mv-3ddet: {n} raw detections, {len(want.keep)} after the filter')
    assert 0 < len(want.keep) < n and bool((want.scores_3d >= flt['score_thr']).all())
    assert torch.equal(want.bboxes_3d.tensor, hand.bboxes_3d.tensor[want.keep])
    other = I.run_scene(det, os.path.join(demo, 'room'), pipe, seed=SEED + 1, filter=None)[0]
    assert not (other.scores_3d.shape == hand.scores_3d.shape and torch.equal(other.scores_3d, hand.scores_3d)), 'the seed does not reach the pipeline'
    with pytest.raises(ValueError, match='walk'):
        next(I.walk_scene(det, os.path.join(demo, 'room'), pipe))


# ------------------------------------------------------------------------------------------------------------------ cont-det3d
@pytest.fixture(scope='module')
def cont_det(dev, demo, tmp_path_factory):
    """the detector (through a written config and a saved checkpoint, as the command line gets them), the walk by hand, its median score"""
    from embodiedscan_amd import inference as I, pipeline
    from embodiedscan_amd.checkpoint import save_checkpoint
    from embodiedscan_amd.config import load_config
    work = tmp_path_factory.mktemp('cfg')
    base = load_config(CD.CFG)
    cfg_path = os.path.join(str(work), 'cont_det3d_small.py')
    with open(cfg_path, 'w') as f:
        f.write(f"_base_ = [{CD.CFG!r}]\nmodel = dict(test_cfg=dict({', '.join(f'{k}={v!r}' for k, v in TEST_CFG.items())}))\n"
                f"test_pipeline = {_small_pipeline(base)!r}\nmetainfo = dict(classes=['chair', 'table'])\n")
    seeded = CD._build(dev)
    CD._randomise_statistics(seeded, dev, seed=2)
    ckpt = os.path.join(str(work), 'weights.pth')
    save_checkpoint(seeded, ckpt)
    det, cfg = I.init_model(cfg_path, ckpt, device=dev)
    assert det.bbox_head.test_cfg == TEST_CFG
    pipe = I.pipeline_of(cfg)
    dscan = _scan(det, demo, pipe)
    batch = pipeline.make_cont_det_batch(dscan)
    cloud = batch['inputs']['points'][-1]
    data = det.data_preprocessor(batch, False)
    imgs = data['inputs']['imgs'].clone()
    meta = dict(data['data_samples'][0].metainfo)
    meta['depth2img'] = {k: v for k, v in meta['depth2img'].items() if k not in ('extrinsic', 'intrinsic')}
    walk = det.open_walk(meta, max_frames=4)
    raw = []
    for t, (r0, r1), e, i in pipeline.walk_frames(dscan, cloud.shape[0]):
        r = walk.observe(imgs[0, t], cloud[r0:r1], dict(extrinsic=e, intrinsic=i))
        raw.append(type(r)(bboxes_3d=r.bboxes_3d, scores_3d=r.scores_3d.clone(), labels_3d=r.labels_3d.clone()))
    torch.cuda.synchronize()
    return dict(det=det, cfg_path=cfg_path, ckpt=ckpt, pipe=pipe, raw=raw, thr=_split(torch.cat([r.scores_3d for r in raw])))


def test_walk_scene_yields_the_filtered_observations(cont_det, demo):
    from embodiedscan_amd import inference as I
    c, det = cont_det, cont_det['det']
    flt = dict(score_thr=c['thr'], topk_per_class=2)
    got = list(I.walk_scene(det, os.path.join(demo, 'room'), c['pipe'], seed=SEED, filter=flt))
    assert [t for t, _ in got] == [0, 1, 2, 3]
    kept = 0
    for t, g in got:
        want = I.filter_instances(c['raw'][t], n_classes=det.bbox_head.num_classes, **flt)
        _same_instances(g, want, f'prefix {t}')
        print(f'prefix {t}: {len(c["raw"][t].scores_3d)} raw detections, {len(want.keep)} after the filter')
        kept += len(want.keep)
    assert 0 < kept < sum(len(r.scores_3d) for r in c['raw'])
    raw = list(I.walk_scene(det, os.path.join(demo, 'room'), c['pipe'], seed=SEED, filter=None, max_frames=2))
    assert [t for t, _ in raw] == [0, 1] and all(torch.equal(r.scores_3d, c['raw'][t].scores_3d) for t, r in raw)
    # the batch path on the same folder: one filtered list per prefix, the same detections as the walk (test_gpu_walk_session's tolerances)
    batch = I.run_scene(det, os.path.join(demo, 'room'), c['pipe'], seed=SEED, filter=None)
    assert len(batch) == 4
    for t, b in enumerate(batch):
        CD._same(tuple(a.cpu().numpy() for a in (b.bboxes_3d.tensor, b.scores_3d, b.labels_3d)),
                 tuple(a.cpu().numpy() for a in (c['raw'][t].bboxes_3d.tensor, c['raw'][t].scores_3d, c['raw'][t].labels_3d)), f'prefix {t}')


def test_command_line_writes_the_same_counts(cont_det, demo, tmp_path):
    from embodiedscan_amd import inference as I
    c = cont_det
    out = str(tmp_path / 'objects.json')
    cmd = [sys.executable, '-m', 'embodiedscan_amd.inference', c['cfg_path'], c['ckpt'], '--root-dir', demo, '--scene', 'room', '--walk',
           '--seed', str(SEED), '--score-thr', repr(c['thr']), '--topk-per-class', '2', '--out', out]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    doc = json.load(open(out))
    assert doc['scene'] == 'demo/room' and doc['walk'] is True and doc['model'] == 'Embodied3DDetector' and len(doc['results']) == 4
    flt = dict(score_thr=c['thr'], topk_per_class=2)
    for t, rec in enumerate(doc['results']):
        want = I.filter_instances(c['raw'][t], n_classes=c['det'].bbox_head.num_classes, **flt)
        assert rec['t'] == t and len(rec['boxes']) == len(rec['scores']) == len(rec['labels']) == len(rec['class_names']) == len(want.keep)
        assert rec['labels'] == want.labels_3d.cpu().tolist() and all(len(b) == 9 for b in rec['boxes'])
        assert all(nm == (['chair', 'table'][l] if l < 2 else f'class_{l}') for nm, l in zip(rec['class_names'], rec['labels']))


# ------------------------------------------------------------------------------------------------------------------ cont-occ
def test_walk_scene_yields_the_occupancy_volumes(dev, demo):
    from embodiedscan_amd import inference as I, pipeline
    cfg = CO._small_cfg()
    det, _ = I.init_model(cfg, device=dev)
    pipe = _small_pipeline(cfg)
    dscan = _scan(det, demo, pipe)
    batch = I.make_scene_batch(det, dscan)
    cloud = batch['inputs']['points'][-1]
    data = det.data_preprocessor(batch, False)
    imgs = data['inputs']['imgs'].clone()
    meta = dict(data['data_samples'][0].metainfo)
    meta['depth2img'] = {k: v for k, v in meta['depth2img'].items() if k not in ('extrinsic', 'intrinsic')}
    walk = det.open_walk(meta)
    want = [walk.observe(imgs[0, t], cloud[r0:r1], dict(extrinsic=e, intrinsic=i)).clone()
            for t, (r0, r1), e, i in pipeline.walk_frames(dscan, cloud.shape[0])]
    got = list(I.walk_scene(det, os.path.join(demo, 'room'), pipe, seed=SEED))
    assert [t for t, _ in got] == [0, 1, 2, 3]
    X, Y, Z = cfg['model']['n_voxels']
    for (t, g), w in zip(got, want):
        assert g.shape == (X, Y, Z) and g.dtype == torch.int64 and torch.equal(g, w), f'prefix {t}'
    assert any(not torch.equal(want[0], w) for w in want[1:]), 'every prefix got the same volume'
    vols = I.run_scene(det, os.path.join(demo, 'room'), pipe, seed=SEED)
    assert len(vols) == 4 and all(v.shape == (X, Y, Z) for v in vols)


# ------------------------------------------------------------------------------------------------------------------ nothing else moves
_CHILD = r'''
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join({root!r}, 'tests'))
import test_gpu_cont_det as CD
from embodiedscan_amd import pipeline
dev = torch.device('cuda:0')
det = CD._build(dev)
CD._randomise_statistics(det, dev, seed=2)
det.bbox_head.test_cfg = dict(nms_pre=300, iou_thr=0.5, score_thr=0.09)
dscan = pipeline.upload_scan(CD._sweep_scan(44, 2), dev)
def predict():
    data = det.data_preprocessor(pipeline.make_cont_det_batch(dscan), False)
    out = det.forward(data['inputs'], data['data_samples'], mode='predict')
    torch.cuda.synchronize()
    return [(ds.pred_instances_3d.bboxes_3d.tensor.clone(), ds.pred_instances_3d.scores_3d.clone(), ds.pred_instances_3d.labels_3d.clone()) for ds in out]
assert 'embodiedscan_amd.inference' not in sys.modules
before = predict()
from embodiedscan_amd import inference
from embodiedscan_amd.structures import InstanceData
kept = [len(inference.filter_instances(InstanceData(bboxes_3d=b, scores_3d=s, labels_3d=l), n_classes=284).keep) for b, s, l in before]
after = predict()
same = all(torch.equal(x, y) for a, b in zip(before, after) for x, y in zip(a, b))
print(json.dumps(dict(same=same, n=[len(s) for _, s, _ in before], kept=kept)))
'''


def test_predict_is_unchanged_by_the_module():
    """predict before embodiedscan_amd.inference is imported and after it was imported and used: identical tensors (a child process,
    so that no other test's import comes first)"""
    res = subprocess.run([sys.executable, '-c', _CHILD.format(root=ROOT)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    doc = json.loads(res.stdout.strip().splitlines()[-1])
    assert doc['same'] and sum(doc['n']) > 0 and 0 < sum(doc['kept']) <= sum(doc['n']), doc
