"""Object tracks through embodiedscan_amd.inference on the MI355X: the demo folder of tests/test_gpu_inference.py (4 frames at 60 x 80,
the small cont-det3d settings, seeded random weights) through walk_scene(track=...), --render and the command line.  The reference of
the ids is a tracks.TrackTable updated by hand with filter_instances(walk.observe(...)) -- the table itself is held to its
specification in tests/test_gpu_tracks.py; the pictures are held to tests/render_spec.py with the track colours."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_spec as RS
import test_gpu_inference as TI
from test_gpu_inference import cont_det, demo, dev  # noqa: F401  (module-scoped fixtures: the folder, the detector, the walk by hand)
from test_gpu_render import _frames_of

pytestmark = pytest.mark.gpu
ROOT = TI.ROOT
TOPK = 3


def _by_hand(c, flt, **track):
    """-> per frame (the filtered list, ids, hits, first_seen) of a TrackTable fed by hand, and the table"""
    from embodiedscan_amd import inference as I
    from embodiedscan_amd.tracks import TrackTable
    table = TrackTable(c['det'].device, **track)
    out = []
    for t, raw in enumerate(c['raw']):
        inst = I.filter_instances(raw, n_classes=c['det'].bbox_head.num_classes, **flt)
        ids = table.update(inst, t)
        hits, first = table.lookup(ids)
        out.append((inst, ids, hits, first))
    return out, table


def test_walk_scene_tracks_equal_a_table_fed_by_hand(cont_det, demo):  # noqa: F811
    from embodiedscan_amd import inference as I
    c, det = cont_det, cont_det['det']
    flt = dict(score_thr=c['thr'], topk_per_class=TOPK)
    scene = os.path.join(demo, 'room')
    plain = list(I.walk_scene(det, scene, c['pipe'], seed=TI.SEED, filter=flt))
    for kw in (dict(), dict(iou_thr=0.5, max_age=0, same_class=True, capacity=512)):
        want, table = _by_hand(c, flt, **kw)
        got = list(I.walk_scene(det, scene, c['pipe'], seed=TI.SEED, filter=flt, track=kw))
        assert [t for t, _ in got] == [0, 1, 2, 3]
        for (t, g), (inst, ids, hits, first), (_, p) in zip(got, want, plain):
            TI._same_instances(g, inst, f'prefix {t}: the tracked list against filter_instances(observe)')
            TI._same_instances(g, p, f'prefix {t}: track= changed the list')
            assert g.track_ids.dtype == torch.int64 and g.track_ids.device == inst.scores_3d.device
            assert torch.equal(g.track_ids, ids) and torch.equal(g.track_hits, hits) and torch.equal(g.track_first_seen, first), f'prefix {t}'
            assert not hasattr(p, 'track_ids'), 'a walk without track= carries ids'
            ids_l = ids.cpu().tolist()
            assert len(set(ids_l)) == len(ids_l) and min(ids_l, default=0) >= 0, 'two rows of a frame share a track'
            print(f'{kw or "defaults"} prefix {t}: ids {ids_l} hits {hits.cpu().tolist()}')
        assert int(want[-1][2].max()) >= 3 and int((want[-1][2] == 1).sum()) > 0, 'the walk holds no track that continues over three frames, or no birth at the end'
        inv = table.inventory(alive_only=False)
        assert inv.track_ids.cpu().tolist() == list(range(int(table.counts[0]))) and int(inv.hits.sum()) == sum(len(w[1]) for w in want)
    assert len(want[0][1]) > 0 and want[0][1].cpu().tolist() == list(range(len(want[0][1]))), 'frame 0: every detection is born, in row order'
    with pytest.raises(ValueError, match='capacity'):
        next(I.walk_scene(det, scene, c['pipe'], seed=TI.SEED, filter=flt, track=dict(capacity=0)))


def test_render_colours_by_track(cont_det, demo, tmp_path):  # noqa: F811
    from embodiedscan_amd import inference as I, render as RD
    c, det = cont_det, cont_det['det']
    flt = dict(score_thr=c['thr'], topk_per_class=TOPK)
    scene = os.path.join(demo, 'room')
    out = str(tmp_path / 'tracked')
    got = list(I.walk_scene(det, scene, c['pipe'], seed=TI.SEED, filter=flt, render=out, class_names=['chair', 'table'], track=dict()))
    want, _ = _by_hand(c, flt)
    pal = RD.class_palette(257)[1:]
    dscan = TI._scan(det, demo, c['pipe'])
    E, K = I.frame_matrices(dscan)
    src = dscan['img'].cpu().numpy()
    pngs = _frames_of(out, 4)
    pairs, legend_want = 0, {}
    for (t, g), (inst, ids, _, _) in zip(got, want):
        assert torch.equal(g.track_ids, ids)
        ids_n, lab = ids.cpu().numpy(), g.labels_3d.cpu().numpy()
        colours = pal[ids_n % 256]
        pic = RS.render_boxes(src[t:t + 1], 1, g.bboxes_3d.tensor.cpu().numpy(), E[t:t + 1].astype(np.float32), K[t:t + 1].astype(np.float32), colours, 4, 192)[0]
        assert np.array_equal(pngs[t], pic), f'frame {t}: {int((pngs[t] != pic).any(-1).sum())} pixels differ from the picture in track colours'
        for a in range(len(lab)):
            for b in range(a + 1, len(lab)):
                if lab[a] == lab[b]:
                    assert ids_n[a] != ids_n[b] and colours[a].tolist() != colours[b].tolist(), 'two boxes of one class share a colour'
                    pairs += 1
    assert pairs > 0, 'no frame holds two boxes of one class'
    legend = json.load(open(os.path.join(out, 'legend.json')))
    seen = sorted({i for _, ids, _, _ in want for i in ids.cpu().tolist()})
    assert sorted(legend, key=lambda k: int(k.split('_')[1])) == [f'track_{i}' for i in seen]
    names = ['chair', 'table']
    table_labels = _by_hand(c, flt)[1].i[:, 0].cpu().tolist()
    for i in seen:
        l = table_labels[i]
        assert legend[f'track_{i}'] == dict(color=pal[i % 256].tolist(), class_name=names[l] if l < 2 else f'class_{l}')
    # without track= the class colouring and the legend are what they were
    plain = str(tmp_path / 'plain')
    list(I.walk_scene(det, scene, c['pipe'], seed=TI.SEED, filter=flt, render=plain, class_names=['chair', 'table']))
    cls_legend = json.load(open(os.path.join(plain, 'legend.json')))
    assert list(cls_legend)[:3] == ['chair', 'table', 'class_2'] and list(cls_legend.values()) == I.scene_palette(det).tolist()


def test_command_line_tracks(cont_det, demo, tmp_path):  # noqa: F811
    c = cont_det
    flt = dict(score_thr=c['thr'], topk_per_class=TOPK)
    want, _ = _by_hand(c, flt, iou_thr=0.3, max_age=2)
    out = str(tmp_path / 'objects.json')
    base = [sys.executable, '-m', 'embodiedscan_amd.inference', c['cfg_path'], c['ckpt'], '--root-dir', demo, '--scene', 'room', '--seed', str(TI.SEED),
            '--score-thr', repr(c['thr']), '--topk-per-class', str(TOPK), '--out', out]
    res = subprocess.run(base + ['--walk', '--track', '--track-iou', '0.3', '--track-max-age', '2'], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    doc = json.load(open(out))
    assert doc['walk'] is True and doc['track'] == dict(iou_thr=0.3, max_age=2) and len(doc['results']) == 4
    for t, (rec, (inst, ids, _, _)) in enumerate(zip(doc['results'], want)):
        assert rec['t'] == t and rec['track_ids'] == ids.cpu().tolist() and rec['labels'] == inst.labels_3d.cpu().tolist()
        assert len(rec['boxes']) == len(rec['track_ids'])
    os.remove(out)
    for extra in (['--track'], ['--track-iou', '0.3', '--walk']):
        res = subprocess.run(base + extra, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert res.returncode == 2 and '--track' in res.stderr and '--walk' in res.stderr and not os.path.exists(out), res.stderr[-2000:]
