"""A posed RGB-D recording in, an object list (or an occupancy volume) out -- and, with --render, the prediction drawn onto the frames
the model consumed: the reference's demo (demo/demo.py) without the 3-D viewer.

    python -m embodiedscan_amd.inference CONFIG [CHECKPOINT] --root-dir D --scene S [--walk] [--out F.json] [--render DIR]
                                         [--map DIR [--map-cell M] [--map-z ZMIN ZMAX]] [--track [--track-iou X] [--track-max-age K]]
                                         [--cloud DIR [--cloud-cell M] [--cloud-min-hits N] [--cloud-every K]]

reads D/S/{poses.txt, intrinsic.txt, axis_align_matrix.txt, rgb/<timestamp>.jpg, depth/<timestamp>.png}, runs the model of CONFIG in
`predict` mode (or frame by frame through a walk session with --walk) and writes the filtered boxes, scores, labels and class names
(occupancy models: the volume's shape and class histogram) as JSON.

filter_instances is the demo's nms_filter (demo.py:84-130) on the device: a score threshold, CLASS-AGNOSTIC greedy suppression on the
true 9-DoF IoU and a per-class quota, in one launch of es_box3d_iou_filter behind es_topk_sorted.  It is not the head's NMS
(bbox_head.predict: per class, BEV IoU, hundreds to thousands of boxes per prefix) and changes nothing there: everything here is opt-in.
The IoU of a candidate row i with a kept row j is the [i][j] element of es_box3d_iou -- the candidate is the first argument -- and is
compared in f32, like the score, against the f32 value of the threshold; a NaN IoU (zero-volume pair) does not suppress.

render=DIR (run_scene, walk_scene, --render): frame_0000.png ... = dscan['img'] -- the resized frames the image backbone saw -- under the
prediction, projected with that sample's own depth2img matrices (frame_matrices), so the picture shows the projection the fusion used;
legend.json (class name -> colour) lies next to them.  embodiedscan_amd.render draws on the device; with render=None nothing of it runs.

map=DIR (run_scene, walk_scene, --map [--map-cell M] [--map-z ZMIN ZMAX]): the scene seen from above (embodiedscan_amd.scene_map, DESIGN
3i).  run_scene writes DIR/map.png -- every view's depth pixels in the frames' colours, z-buffered from above under the z cut, under the final
boxes' footprints (or the final volume's top surface) and the trail of the camera centres --, DIR/map.json (the grid, the z cut and
max_depth: a pixel maps back to metres) and DIR/legend.json; walk_scene writes map_0000.png ...: map t holds frames 0 .. t, the prediction of
prefix t and the trail so far.  The grid is fixed before the first frame: the rectangle of all camera centres grown by 8 m (detectors) or the
xy rectangle of point_cloud_range (occupancy).  With map=None nothing of it runs.

cloud=DIR (run_scene, walk_scene, --cloud [--cloud-cell M] [--cloud-min-hits N] [--cloud-every K]): the scene in three dimensions as
binary PLY files that MeshLab, CloudCompare, Blender or open3d open (embodiedscan_amd.scene_cloud): DIR/scene.ply, the
recording's depth pixels fused on the device into one coloured point per voxel of M metres, every point labelled with the class and the
row (--track: the track id) of the detection that contains it; DIR/boxes.ply, the boxes' wireframes, or DIR/occupancy.ply, the exposed
voxel faces of the volume; DIR/cloud.json.  The records of a labelled list gain `support`, the number of points inside each box.  With
cloud=None nothing of it runs.

--track (with --walk, the cont-det3d model; walk_scene(track=dict(...))): a tracks.TrackTable is updated with every frame's filtered list,
the records gain track_ids -- the same object keeps its id from frame to frame -- and --render colours by track (legend.json: track_<id> ->
{color, class_name}).  Without it nothing of the table runs and every output is what it was.

Asking in words (a grounding configuration):

    python -m embodiedscan_amd.inference CONFIG [CHECKPOINT] --root-dir D --scene S --prompt "the chair next to the window" [--prompt ...]
                                         [--prompts-file F] [--topk K] [--iou-thr X] [--score-thr Y] [--walk] [--render DIR]

ground_scene encodes the folder once and grounds every prompt on that encoding; ask_walk feeds a GroundWalk frame by frame and answers
on the prefix seen so far.  select_answers turns the Q boxes and scores ground() returns per prompt into a short list of distinct boxes:
the greedy of filter_instances with one class, for ALL prompts in one launch of es_ground_answers and one host read.  The JSON holds
results = [{t, prompt, boxes, scores, keep}] (t: the last frame of the prefix, null for the whole recording); with --render every
prompt's answers are drawn in the prompt's own colour (legend.json: prompt -> colour)."""
import json
import os

import numpy as np
import torch

from . import hip
from . import pipeline as PL
from . import render as RD
from . import scene_cloud as SC
from . import scene_map as SM
from .structures import EulerDepthInstance3DBoxes, InstanceData

MAX_ROWS, MAX_CLASSES = 16384, 4096          # limits of es_topk_sorted / es_box3d_iou_filter


def filter_instances(instances, iou_thr=0.15, score_thr=0.075, topk_per_class=10, n_classes=None):
    """what bbox_head.predict / DetWalk.observe return -> InstanceData(bboxes_3d, scores_3d, labels_3d, keep) of the demo's object
    list, in selection order (score descending, ties to the lower row); `keep` = int64 rows of the input.  n_classes None: max(label)
    + 1, which costs one read-back (detectors pass bbox_head.num_classes); a row with a label outside [0, n_classes) is never kept.
    The only host synchronisation otherwise is the read of the kept count.  ValueError before any launch: inputs on different
    devices, more than 16384 rows, n_classes outside 1 .. 4096, topk_per_class < 1."""
    boxes = getattr(instances.bboxes_3d, 'tensor', instances.bboxes_3d)
    scores, labels = instances.scores_3d, instances.labels_3d
    if not (boxes.device == scores.device == labels.device):
        raise ValueError(f'filter_instances: boxes on {boxes.device}, scores on {scores.device}, labels on {labels.device}')
    n = int(boxes.shape[0])
    if boxes.dim() != 2 or boxes.shape[1] != 9 or scores.shape != (n,) or labels.shape != (n,):
        raise ValueError(f'filter_instances: boxes (n, 9), scores (n), labels (n); got {tuple(boxes.shape)}, {tuple(scores.shape)}, '
                         f'{tuple(labels.shape)}')
    if n > MAX_ROWS:
        raise ValueError(f'filter_instances: {n} rows, the sorted order covers {MAX_ROWS} (raise the head\'s score_thr or lower nms_pre)')
    if topk_per_class < 1:
        raise ValueError(f'filter_instances: topk_per_class = {topk_per_class}')
    if n_classes is None:
        n_classes = max(int(labels.max()) + 1, 1) if n else 1
    if not 1 <= n_classes <= MAX_CLASSES:
        raise ValueError(f'filter_instances: n_classes = {n_classes}, the class counters cover 1 .. {MAX_CLASSES}')
    dev, P, st = boxes.device, hip.P, hip.stream()
    b, s, l = boxes.float().contiguous(), scores.float().contiguous(), labels.to(torch.int32).contiguous()
    order = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    keep_idx = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    keep_cnt = torch.empty(1, dtype=torch.int32, device=dev)
    if n:
        hip.call('es_topk_sorted', P(s), 1, n, 0, n, P(order), st)
    hip.call('es_box3d_iou_filter', P(b), P(s), P(l), P(order), n, int(n_classes), float(iou_thr), float(score_thr), int(topk_per_class),
             P(keep_idx), P(keep_cnt), st)
    keep = keep_idx[:int(keep_cnt.item())].long()
    return InstanceData(bboxes_3d=EulerDepthInstance3DBoxes(boxes[keep]), scores_3d=scores[keep], labels_3d=labels[keep], keep=keep)


MAX_ANSWER_ROWS, MAX_ANSWER_PROMPTS = 1024, 65535      # limits of es_ground_answers


def select_answers(results, iou_thr=0.25, score_thr=0.0, topk=1):
    """what SparseFeatureFusion3DGrounder.ground returns -- a list of P InstanceData with Q rows each -- or stacked (boxes (P, Q, 9),
    scores (P, Q)) tensors -> a list of P InstanceData(bboxes_3d, scores_3d, keep): per prompt the at most `topk` distinct boxes in
    selection order (score descending, ties to the lower row; a row below score_thr or with a NaN score is never an answer; a row whose
    9-DoF IoU with an already chosen one exceeds iou_thr is skipped), `keep` = int64 rows of the prompt's input.  ONE launch of
    es_ground_answers for all prompts and one host read (the P counts).  The defaults are interface choices: 0.25 is the lower IoU at
    which GroundingMetric calls two boxes the same object, topk = 1 is "the" answer.  ValueError before any launch: inputs on different
    devices, prompts with different numbers of rows, more than 1024 rows or 65535 prompts, topk outside 1 .. max(Q, 1)."""
    if isinstance(results, (tuple, list)) and len(results) == 2 and all(torch.is_tensor(t) for t in results):
        boxes, scores = results
        if boxes.dim() != 3 or boxes.shape[2] != 9 or tuple(scores.shape) != tuple(boxes.shape[:2]):
            raise ValueError(f'select_answers: boxes (P, Q, 9), scores (P, Q); got {tuple(boxes.shape)}, {tuple(scores.shape)}')
        if boxes.device != scores.device:
            raise ValueError(f'select_answers: boxes on {boxes.device}, scores on {scores.device}')
        n_p, n_q = int(boxes.shape[0]), int(boxes.shape[1])
        per_b, per_s = list(boxes), list(scores)
    else:
        results = list(results)
        per_b = [getattr(r.bboxes_3d, 'tensor', r.bboxes_3d) for r in results]
        per_s = [r.scores_3d for r in results]
        n_p = len(results)
        devs = {t.device for t in per_b + per_s}
        if len(devs) > 1:
            raise ValueError(f'select_answers: inputs on different devices: {sorted(str(d) for d in devs)}')
        for b, s in zip(per_b, per_s):
            if b.dim() != 2 or b.shape[1] != 9 or tuple(s.shape) != (b.shape[0],):
                raise ValueError(f'select_answers: per prompt boxes (Q, 9) and scores (Q); got {tuple(b.shape)}, {tuple(s.shape)}')
        qs = {int(b.shape[0]) for b in per_b}
        if len(qs) > 1:
            raise ValueError(f'select_answers: the prompts carry different numbers of rows {sorted(qs)}; one launch takes one Q')
        n_q = qs.pop() if qs else 0
        boxes = torch.stack(per_b) if n_p else None
        scores = torch.stack(per_s) if n_p else None
    if n_q > MAX_ANSWER_ROWS:
        raise ValueError(f'select_answers: {n_q} rows per prompt, the selection covers {MAX_ANSWER_ROWS}')
    if n_p > MAX_ANSWER_PROMPTS:
        raise ValueError(f'select_answers: {n_p} prompts, one launch covers {MAX_ANSWER_PROMPTS}')
    topk = int(topk)
    if not 1 <= topk <= max(n_q, 1):
        raise ValueError(f'select_answers: topk = {topk} outside 1 .. {max(n_q, 1)} (Q = {n_q})')
    if n_p == 0:
        return []
    dev, P = boxes.device, hip.P
    b, s = boxes.float().contiguous(), scores.float().contiguous()
    ans_idx = torch.empty((n_p, topk), dtype=torch.int32, device=dev)
    ans_cnt = torch.empty(n_p, dtype=torch.int32, device=dev)
    hip.call('es_ground_answers', P(b), P(s), n_p, n_q, float(iou_thr), float(score_thr), topk, P(ans_idx), P(ans_cnt), hip.stream())
    counts = ans_cnt.tolist()                                            # the one host read
    idx = ans_idx.long()
    out = []
    for p, c in enumerate(counts):
        keep = idx[p, :c]
        out.append(InstanceData(bboxes_3d=EulerDepthInstance3DBoxes(per_b[p][keep]), scores_3d=per_s[p][keep], keep=keep))
    return out


# ------------------------------------------------------------------------------------------------------------------ the folder
CAM_AXES = np.array([[0., 0., 1.], [-1., 0., 0.], [0., -1., 0.]])       # demo.py:180: the recorder's camera axes -> the model's


def quat_to_matrix(q):
    """(x, y, z, w), scalar last, any non-zero norm -> 3 x 3 rotation (f64), as scipy's Rotation.from_quat(q).as_matrix()"""
    q = np.asarray(q, np.float64)
    nrm = float(np.sqrt((q * q).sum()))
    if q.shape != (4,) or not nrm > 0:
        raise ValueError(f'a quaternion has four components and a non-zero norm, got {q.tolist()}')
    x, y, z, w = q / nrm
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _matrix44(path):
    m = np.loadtxt(path)
    if m.shape != (4, 4):
        raise ValueError(f'{path}: a 4 x 4 matrix, got shape {m.shape}')
    return m


def scene_info(scene_dir, origin=(0, 0, .5), depth_shift=1000., skip_first=True):
    """The folder of the reference's demo (demo.py:143-197) -> the `info` dict ScanPipeline.__call__ consumes (numpy f64 throughout,
    no scipy).  poses.txt: `timestamp x y z qx qy qz qw` per line; cam2global = [R(q) CAM_AXES | t]; extrinsic_i = inv(axis_align @
    cam2global_i) as f32; frames rgb/<timestamp>.jpg and depth/<timestamp>.png; depth_cam2img = cam2img = intrinsic; empty ground
    truth; scan_id = sample_idx = demo/<scene>.

    skip_first: the reference's loop starts at line 1 of poses.txt and never uses line 0 -- kept as the default so that the same
    folder gives the same frames; skip_first=False uses every line.
    ValueError: intrinsic.txt / axis_align_matrix.txt not 4 x 4, a malformed pose line.  FileNotFoundError naming the first missing
    frame file, before anything is decoded."""
    scene_dir = os.path.abspath(scene_dir)
    scene = os.path.basename(scene_dir.rstrip(os.sep))
    axis_align = _matrix44(os.path.join(scene_dir, 'axis_align_matrix.txt'))
    intrinsic = _matrix44(os.path.join(scene_dir, 'intrinsic.txt')).astype(np.float32)
    with open(os.path.join(scene_dir, 'poses.txt')) as f:
        lines = [ln for ln in f.read().splitlines() if ln.strip()]
    images, img_path, depth_path, extrinsic = [], [], [], []
    for k, ln in enumerate(lines[1 if skip_first else 0:], 1 if skip_first else 0):
        tok = ln.split()
        if len(tok) != 8:
            raise ValueError(f'{scene_dir}/poses.txt line {k}: `timestamp x y z qx qy qz qw`, got {len(tok)} fields')
        stamp, vals = tok[0], [float(v) for v in tok[1:]]
        c2g = np.identity(4)
        c2g[:3, :3] = quat_to_matrix(vals[3:]) @ CAM_AXES
        c2g[:3, 3] = vals[:3]                                            # camera -> the recording's (not yet aligned) global frame
        images.append(dict(img_path=os.path.join('demo', scene, 'rgb', stamp + '.jpg'),
                           depth_path=os.path.join('demo', scene, 'depth', stamp + '.png'), cam2global=c2g, cam2img=intrinsic))
        img_path.append(os.path.join(scene_dir, 'rgb', stamp + '.jpg'))
        depth_path.append(os.path.join(scene_dir, 'depth', stamp + '.png'))
        extrinsic.append(np.linalg.inv(axis_align @ c2g).astype(np.float32))
    for p in (q for pair in zip(img_path, depth_path) for q in pair):
        if not os.path.isfile(p):
            raise FileNotFoundError(p)
    V = len(images)
    return dict(scan_id=f'demo/{scene}', sample_idx=f'demo/{scene}', axis_align_matrix=axis_align, images=images, img_path=img_path,
                depth_img_path=depth_path,
                depth2img=dict(extrinsic=extrinsic, intrinsic=intrinsic, origin=np.asarray(origin, np.float32)),
                depth_cam2img=intrinsic, depth_shift=float(depth_shift), cam2img=intrinsic, box_type_3d='euler-depth',
                ann_info=dict(gt_bboxes_3d=np.zeros((0, 9), np.float32), gt_labels_3d=np.zeros((0,), np.int64),
                              visible_instance_masks=[[] for _ in range(V)], gt_occupancy=np.zeros((0, 4), np.int64),
                              visible_occupancy_masks=[[] for _ in range(V)]))


# ------------------------------------------------------------------------------------------------------------------ the model
def init_model(config, checkpoint=None, device='cuda:0'):
    """config: a path or a loaded config dict -> (detector in eval mode on `device`, cfg); checkpoint None: the seeded initialisation"""
    from .checkpoint import load_checkpoint
    from .config import build_detector, load_config
    cfg = load_config(config) if isinstance(config, (str, os.PathLike)) else config
    det = build_detector(cfg, device=device).to(device)
    if checkpoint is not None:
        load_checkpoint(det, checkpoint)
    det.train(False)
    return det, cfg


def pipeline_of(cfg):
    """cfg.test_dataloader.dataset.pipeline; a config that carries no test dataloader: its val dataloader's, else its `test_pipeline`"""
    for key in ('test_dataloader', 'val_dataloader'):
        if cfg.get(key) is not None:
            return cfg[key]['dataset']['pipeline']
    return cfg['test_pipeline']


def _kind(detector):
    """'det3d' / 'occ', 'cont-' in front for the continuous models: from the class attributes `task` and `continuous`"""
    if getattr(detector, 'task', None) in ('det3d', 'occ'):
        return ('cont-' if detector.continuous else '') + detector.task
    raise ValueError(f'{type(detector).__name__}: run_scene / walk_scene serve the detection and occupancy models (a grounder needs a prompt)')


def load_scene(detector, scene_dir, pipeline, seed=0):
    """scene_info -> ScanPipeline.from_cfg(pipeline) with numpy RandomState(seed) -> the scan on the detector's device"""
    from .datasets.loading import ScanPipeline
    scan = ScanPipeline.from_cfg(pipeline)(scene_info(scene_dir), np.random.RandomState(seed))
    return PL.upload_scan(scan, detector.device)


def make_scene_batch(detector, dscan):
    """the batch builder of the detector's kind on a scan without ground truth (the continuous kinds: one cloud per prefix)"""
    kind = _kind(detector)
    if kind == 'cont-det3d':
        return PL.make_cont_det_batch(dscan)
    if kind == 'cont-occ':                                               # (one mask per prefix makes the preprocessor split the sample)
        return PL.make_cont_occ_batch(dscan, dict(gt_occupancy=torch.zeros((0, 4), dtype=torch.int64),
                                                  gt_occupancy_masks=[None] * (len(dscan['points_slice_indices']) - 1)))
    return PL.make_batch([dscan])


# ------------------------------------------------------------------------------------------------------------------ the picture
def _scan_matrices(dscan):
    """-> (extrinsic, intrinsic, (sx, sy)): the scan's depth2img matrices, (V, 4, 4) f64 each, as the meta carries them, and the resize's
    scale_factor.  ValueError for a scan whose pipeline flipped / cropped the image or moved the cloud (a train-time augmentation: its
    predictions do not live in the aligned frame)."""
    meta = dscan['meta']
    pm = meta[PL.projection_key(meta)]
    E = np.stack([np.asarray(e, np.float64) for e in pm['extrinsic']])
    intr = pm['intrinsic']
    K = np.stack([np.asarray(k, np.float64) for k in intr]) if isinstance(intr, (list, tuple)) else np.repeat(np.asarray(intr, np.float64)[None], len(E), 0)
    rot = np.asarray(meta.get('pcd_rotation', np.eye(3)), np.float64)
    moved = (not np.array_equal(rot, np.eye(3)) or float(meta.get('pcd_scale_factor', 1.)) != 1. or bool(np.any(np.asarray(meta.get('pcd_trans', 0.)) != 0))
             or meta.get('pcd_horizontal_flip', False) or meta.get('pcd_vertical_flip', False))
    if moved or meta.get('flip', False) or tuple(meta.get('img_crop_offset', (0., 0.))) != (0., 0.):
        raise ValueError('render: the pipeline augments the scan; draw on a test pipeline')
    sx, sy = (float(s) for s in meta.get('scale_factor', (1., 1.)))
    return E, K.copy(), (sx, sy)


def frame_matrices(dscan):
    """-> (extrinsic, intrinsic), (V, 4, 4) f64 each: the scan's depth2img matrices at the resolution of dscan['img'] -- the fusion projects
    with intrinsic @ extrinsic and then applies the resize's scale_factor (point_fusion.py:79-105); here the factor is folded into the
    intrinsic's first two rows.  ValueError for a scan whose pipeline flipped / cropped the image or moved the cloud (a train-time
    augmentation: its predictions do not live in the aligned frame)."""
    E, K, (sx, sy) = _scan_matrices(dscan)
    K[:, 0, :] *= sx
    K[:, 1, :] *= sy
    return E, K


def depth_matrices(dscan):
    """-> (extrinsic, intrinsic), (V, 4, 4) f64 each, at the resolution of dscan['depth']: frame_matrices without the scale_factor (the
    depth maps are never resized), with the same refusal of an augmenting pipeline"""
    E, K, _ = _scan_matrices(dscan)
    return E, K


def _default_names(detector, kind):
    nc = getattr(detector.bbox_head, 'num_classes', 0)
    return [f'class_{i}' for i in range(nc)] if kind in ('det3d', 'cont-det3d') else ['empty'] + [f'class_{i}' for i in range(max(nc - 1, 0))]


def scene_palette(detector):
    """(n_classes, 3) u8: row l = the colour of label l.  Detectors skip render.class_palette's grey row 0; occupancy keeps it for `empty`"""
    kind, nc = _kind(detector), int(getattr(detector.bbox_head, 'num_classes', 0))
    return RD.class_palette(nc + 1)[1:] if kind in ('det3d', 'cont-det3d') else RD.class_palette(max(nc, 1))


def draw_prediction(detector, frames, extrinsic, intrinsic, res, palette_dev):
    """one prediction (InstanceData or an (X, Y, Z) volume) over frames (V, 3, H, W) u8 -> (V, H, W, 3) u8 on the device"""
    if isinstance(res, InstanceData):
        labels = res.labels_3d.long().clamp(0, palette_dev.shape[0] - 1)
        return RD.render_boxes(frames, extrinsic, intrinsic, res.bboxes_3d, palette_dev[labels], layout='chw')
    return RD.render_occupancy(frames, extrinsic, intrinsic, res, detector.point_cloud_range, palette_dev, layout='chw')


def _class_legend(detector, class_names):
    """-> (the name of every palette row, scene_palette): class_names cut or padded with class_<i> to the palette"""
    pal = scene_palette(detector)
    names = list(class_names) if class_names is not None else _default_names(detector, _kind(detector))
    return names[:len(pal)] + [f'class_{i}' for i in range(len(names), len(pal))], pal


def _painter(dir, names, palette, dscan, device, draw):
    """writes dir/legend.json (names[i] -> palette[i]) now -> paint(res, t=None): draw(frames, extrinsic, intrinsic, res, palette on
    the device) over frame t of the scan saved as frame_<t>.png; t None: over all its frames, numbered from 0"""
    os.makedirs(dir, exist_ok=True)
    with open(os.path.join(dir, 'legend.json'), 'w') as f:
        json.dump({nm: [int(c) for c in palette[i]] for i, nm in enumerate(names)}, f)
    pal = torch.from_numpy(palette).to(device)
    E, K = frame_matrices(dscan)

    def paint(res, t=None):
        v = slice(None) if t is None else slice(t, t + 1)
        RD.save_frames(dir, draw(dscan['img'][v], E[v], K[v], res, pal), start=t or 0)
    return paint


def _prediction_painter(dir, detector, class_names, dscan):
    return _painter(dir, *_class_legend(detector, class_names), dscan, detector.device,
                    lambda *args: draw_prediction(detector, *args))


def _filtered(detector, inst, filter):
    if filter is None:
        return inst
    return filter_instances(inst, **dict(dict(n_classes=detector.bbox_head.num_classes), **filter))


def run_scene(detector, scene_dir, pipeline, seed=0, filter=dict(), render=None, class_names=None, map=None, map_cell=0.02, map_z=(-1.0, 2.0),
              cloud=None, cloud_cell=0.02, cloud_min_hits=1):
    """one `predict` over the folder.  Detectors: the filtered InstanceData per sample (the cont-det3d detector: one per prefix);
    occupancy models: pred_occupancy per sample / prefix.  filter: keyword arguments of filter_instances; None: the raw prediction.
    render: a directory that receives every view of the scan under the final list / volume (the last prefix's for the continuous kinds)
    as frame_0000.png ... and legend.json; None: nothing is drawn.
    map: a directory that receives map.png, map.json and legend.json -- the whole recording seen from above under that same final
    prediction, in cells of map_cell metres, showing z in [map_z[0], map_z[1]); None: nothing of it runs.
    cloud: a directory that receives scene.ply -- every view's depth pixels fused into one voxel of cloud_cell metres each (those that at
    least cloud_min_hits pixels fell into), labelled by that same final prediction --, boxes.ply or occupancy.ply and cloud.json
    (_cloud_writer); the final InstanceData gains cloud_support; None: nothing of it runs."""
    kind = _kind(detector)
    dscan = load_scene(detector, scene_dir, pipeline, seed)
    data = detector.data_preprocessor(make_scene_batch(detector, dscan), False)
    out = detector.forward(data['inputs'], data['data_samples'], mode='predict')
    if kind in ('occ', 'cont-occ'):
        res = [ds.pred_occupancy for ds in out]
    else:
        res = [_filtered(detector, ds.pred_instances_3d, filter) for ds in out]
    if render is not None:
        _prediction_painter(render, detector, class_names, dscan)(res[-1])
    if map is not None:
        _map_painter(map, detector, class_names, dscan, map_cell, map_z)(res[-1])
    if cloud is not None:
        join, write = _cloud_writer(cloud, detector, class_names, dscan, cloud_cell, cloud_min_hits)
        join(None)
        write(res[-1])
    return res


def _scene_walk(detector, dscan, batch, max_frames, capped):
    """opens a walk session on the scan's constant meta (its projection entry without the matrices) -> (walk, n_frames, frames):
    n_frames = min(max_frames, the scan's frames); frames yields (t, (img, rows, matrices)), the arguments of walk.observe for frame
    t < n_frames.  capped: the session keeps per-frame maps and is opened for n_frames of them."""
    cloud = batch['inputs']['points'][-1]
    data = detector.data_preprocessor(batch, False)
    imgs = data['inputs']['imgs'].clone()                                # (the preprocessor's buffers are a ring)
    meta = dict(data['data_samples'][0].metainfo)
    key = PL.projection_key(meta)
    meta[key] = {k: v for k, v in meta[key].items() if k not in ('extrinsic', 'intrinsic')}
    n_frames = imgs.shape[1] if max_frames is None else min(int(max_frames), imgs.shape[1])
    walk = detector.open_walk(meta, max_frames=max(n_frames, 1)) if capped else detector.open_walk(meta)

    def frames():
        for t, (r0, r1), e, i in PL.walk_frames(dscan, cloud.shape[0]):
            if t >= n_frames:
                break
            yield t, (imgs[0, t], cloud[r0:r1], dict(extrinsic=e, intrinsic=i))
    return walk, n_frames, frames()


TRACK_PALETTE = 257                      # a track takes render.class_palette(257)[1:][id % 256]


def _track_legend(dir, names, pal, table):
    """-> update(res): legend.json of a tracked walk, track_<id> -> {color, class_name} for every track drawn so far (the class of the track's
    best detection), rewritten after every frame"""
    legend = {}

    def update(res):
        ids = res.track_ids.cpu().tolist()
        labels = table.i[res.track_ids.clamp(min=0), 0].cpu().tolist()
        for i, l in zip(ids, labels):
            if i >= 0:
                legend[f'track_{i}'] = dict(color=[int(c) for c in pal[i % 256]], class_name=names[l] if 0 <= l < len(names) else f'class_{l}')
        with open(os.path.join(dir, 'legend.json'), 'w') as f:
            json.dump(legend, f)
    return update


def _track_painter(dir, detector, class_names, dscan, table):
    """the painter of a tracked walk: a box takes the colour of its track, render.class_palette(257)[1:][id % 256], so two chairs differ
    and one chair keeps its colour when its arg-max label flickers; legend.json maps track_<id> -> {color, class_name} for every track
    drawn so far (the class of the track's best detection) and is rewritten after every frame"""
    names, _ = _class_legend(detector, class_names)
    pal = RD.class_palette(TRACK_PALETTE)[1:]
    paint = _painter(dir, [], pal, dscan, detector.device,
                     lambda frames, E, K, res, pal_dev: RD.render_boxes(frames, E, K, res.bboxes_3d, pal_dev[res.track_ids.remainder(256)].contiguous(),
                                                                        layout='chw'))
    legend = _track_legend(dir, names, pal, table)

    def paint_tracks(res, t=None):
        paint(res, t)
        legend(res)
    return paint_tracks


def _map_painter(dir, detector, class_names, dscan, cell, z, table=None, max_depth=8.0):
    """fixes the grid from ALL of the scan's poses (occupancy kinds: from point_cloud_range), writes dir/map.json and dir/legend.json now
    -> paint(res, t=None): t None: every view is splatted and map.png holds the prediction `res` and the whole trail; else frame t joins
    the map and map_<t>.png holds the prediction of prefix t and the trail so far.  table: the boxes take their track's colour."""
    os.makedirs(dir, exist_ok=True)
    kind, dev = _kind(detector), detector.device
    E, K = depth_matrices(dscan)
    centres = RD.camera_rays(E, K)[:, 9:]
    z_min, z_max = (float(v) for v in z)
    if kind in ('occ', 'cont-occ'):
        pr = np.asarray(detector.point_cloud_range, np.float64)
        grid = SM.MapGrid.covering(pr[:2], pr[3:5], cell, z_min, z_max)
    else:
        grid = SM.MapGrid.around(centres, cell=cell, z_min=z_min, z_max=z_max)
    smap = SM.SceneMap(grid, dev, max_depth)
    with open(os.path.join(dir, 'map.json'), 'w') as f:
        json.dump(dict(grid=grid.to_json(), max_depth=smap.max_depth, trail_color=list(SM.TRAIL_COLOR)), f)
    names, pal = _class_legend(detector, class_names)
    track_legend = None
    if table is None:
        with open(os.path.join(dir, 'legend.json'), 'w') as f:
            json.dump({nm: [int(c) for c in pal[i]] for i, nm in enumerate(names)}, f)
    else:
        pal = RD.class_palette(TRACK_PALETTE)[1:]
        track_legend = _track_legend(dir, names, pal, table)
    pal_dev = torch.from_numpy(pal).to(dev)

    def paint(res, t=None):
        v = slice(None) if t is None else slice(t, t + 1)
        smap.add(dscan['depth'][v], dscan['img'][v], E[v], K[v], layout='chw')
        img = smap.image()
        if not isinstance(res, InstanceData):
            smap.draw_occupancy(img, res, detector.point_cloud_range, pal_dev)
        elif table is not None:
            smap.draw_boxes(img, res.bboxes_3d, pal_dev[res.track_ids.remainder(256)].contiguous())
        else:
            smap.draw_boxes(img, res.bboxes_3d, pal_dev[res.labels_3d.long().clamp(0, pal_dev.shape[0] - 1)])
        smap.draw_trail(img, centres if t is None else centres[:t + 1])
        path = RD.save_frames(dir, img[None], stem='map', start=t or 0)[0]
        if t is None:
            os.replace(path, os.path.join(dir, 'map.png'))
        if track_legend is not None:
            track_legend(res)
    return paint


def _cloud_writer(dir, detector, class_names, dscan, cell, min_hits, table=None, capacity=1 << 22, max_depth=8.0):
    """the scene in three dimensions as files (scene_cloud) -> (join(t), write(res, t=None)).  join(t) fuses frame t of the scan
    into the cloud (None: every frame).  write(res) writes, under the prediction `res`, dir/scene.ply -- vertex properties x y z red green
    blue hits label instance: detectors: label = the class of the first box of the list that holds the point, instance = that box's row in
    the list (table: its track id), both -1 outside every box; occupancy kinds: both -1 --, dir/boxes.ply (the boxes' wireframes in their
    class colour; table: their track's) or dir/occupancy.ply (the volume's exposed faces in the class palette) and dir/cloud.json (cell,
    capacity, counters, rows, class names and colours, the boxes' support); with t the files are scene_<t>.ply ...; an InstanceData gains
    cloud_support (m,) int32 on the device.  scene_cloud.CloudFull when the table dropped a pixel."""
    os.makedirs(dir, exist_ok=True)
    dev = detector.device
    E, K = depth_matrices(dscan)
    cl = SC.SceneCloud(dev, cell, capacity, max_depth=max_depth)
    names, pal = _class_legend(detector, class_names)
    track_pal = RD.class_palette(TRACK_PALETTE)[1:]

    def join(t):
        v = slice(None) if t is None else slice(t, t + 1)
        cl.add(dscan['depth'][v], dscan['img'][v], E[v], K[v], layout='chw')

    def write(res, t=None):
        sfx = '' if t is None else f'_{t:04d}'
        xyz, rgb, hits = cl.points(min_hits)
        n = int(xyz.shape[0])
        doc = dict(cell=cl.cell, capacity=cl.capacity, min_hits=int(min_hits), counters=list(cl.pixel_counts()), rows=n, class_names=list(names),
                   class_colors=[[int(c) for c in row] for row in pal])
        if isinstance(res, InstanceData):
            row, support = SC.label(xyz, res.bboxes_3d)
            res.cloud_support = support
            hit = row.long().clamp(min=0)
            m = int(support.shape[0])
            lab_of = res.labels_3d.to(torch.int32) if m else torch.zeros(1, dtype=torch.int32, device=dev)
            ins_of = res.track_ids.to(torch.int32) if (table is not None and m) else None
            minus = torch.full_like(row, -1)
            label = torch.where(row >= 0, lab_of[hit if m else torch.zeros_like(hit)], minus)
            instance = row if ins_of is None else torch.where(row >= 0, ins_of[hit], minus)
            labels = res.labels_3d.long().cpu().numpy()
            if table is not None:
                colors = track_pal[res.track_ids.cpu().numpy() % 256]
                doc['track_ids'] = res.track_ids.cpu().tolist()
            else:
                colors = pal[np.clip(labels, 0, len(pal) - 1)]
            bv, be, bc = SC.box_edges(getattr(res.bboxes_3d, 'tensor', res.bboxes_3d), np.ascontiguousarray(colors, np.uint8).reshape(-1, 3))
            SC.write_ply(os.path.join(dir, f'boxes{sfx}.ply'), SC.vertex_columns(bv.astype(np.float32)), edge=(be, bc))
            doc.update(labels=labels.tolist(), support=support.cpu().tolist())
        else:
            label = instance = torch.full((n,), -1, dtype=torch.int32, device=dev)
            verts, quads, face_label, colors = SC.occupancy_mesh(res, detector.point_cloud_range, pal)
            SC.write_ply(os.path.join(dir, f'occupancy{sfx}.ply'), SC.vertex_columns(verts, colors), face=quads)
            doc.update(faces=int(quads.shape[0]))
        SC.write_ply(os.path.join(dir, f'scene{sfx}.ply'), SC.vertex_columns(xyz, rgb, hits=hits, label=label, instance=instance))
        with open(os.path.join(dir, 'cloud.json'), 'w') as f:
            json.dump(doc, f)
    return join, write


def walk_scene(detector, scene_dir, pipeline, seed=0, filter=dict(), max_frames=None, render=None, class_names=None, track=None, map=None,
               map_cell=0.02, map_z=(-1.0, 2.0), cloud=None, cloud_cell=0.02, cloud_min_hits=1, cloud_every=0):
    """generator over the frames of the folder for the two continuous models (the reference's render_continuous_scene): opens a walk
    session, feeds it frame by frame and yields (t, filtered InstanceData) or (t, pred_occupancy).  render: a directory that receives
    frame t under the prediction of prefix t as frame_<t>.png, and legend.json; None: nothing is drawn.
    track (cont-det3d): keyword arguments of tracks.TrackTable (dict(): its defaults).  The table is updated with the filtered list of
    every frame, and the yielded InstanceData gain track_ids (int64; -1: the table was full), track_hits and track_first_seen, all on the
    device; with render the boxes take their track's colour (_track_painter).  None: no table, nothing of it runs.
    map: a directory that receives map_<t>.png -- frames 0 .. t seen from above under the prediction of prefix t and the trail so far, on
    a grid fixed before the first frame from all of the folder's poses --, map.json and legend.json (run_scene); None: nothing of it runs.
    cloud: a directory for the scene in three dimensions (_cloud_writer): frame t joins the cloud after its observe; with cloud_every > 0 the
    frames t % cloud_every == 0 write scene_<t>.ply (+ boxes_<t>.ply / occupancy_<t>.ply) under the prediction of prefix t, and the last
    frame writes the un-numbered files under the last prefix's prediction -- both before the frame is yielded, so that a labelled
    InstanceData carries cloud_support; None: nothing of it runs."""
    kind = _kind(detector)
    if kind not in ('cont-det3d', 'cont-occ'):
        raise ValueError(f'{type(detector).__name__} has no walk session: use run_scene')
    if track is not None and kind != 'cont-det3d':
        raise ValueError(f'{type(detector).__name__} yields no object list: track= goes with the cont-det3d detector')
    dscan = load_scene(detector, scene_dir, pipeline, seed)
    walk, n_frames, frames = _scene_walk(detector, dscan, make_scene_batch(detector, dscan), max_frames, capped=kind == 'cont-det3d')
    table = None
    if track is not None:
        from .tracks import TrackTable
        table = TrackTable(detector.device, **track)
    if render is None:
        paint = None
    elif table is None:
        paint = _prediction_painter(render, detector, class_names, dscan)
    else:
        paint = _track_painter(render, detector, class_names, dscan, table)
    paint_map = None if map is None else _map_painter(map, detector, class_names, dscan, map_cell, map_z, table)
    join, write_cloud = (None, None) if cloud is None else _cloud_writer(cloud, detector, class_names, dscan, cloud_cell, cloud_min_hits, table)
    for t, frame in frames:
        res = walk.observe(*frame)
        res = res if kind == 'cont-occ' else _filtered(detector, res, filter)
        if table is not None:
            res.track_ids = table.update(res, t)
            res.track_hits, res.track_first_seen = table.lookup(res.track_ids)
        if paint is not None:
            paint(res, t)
        if paint_map is not None:
            paint_map(res, t)
        if join is not None:
            join(t)
            if int(cloud_every) > 0 and t % int(cloud_every) == 0:
                write_cloud(res, t)
            if t == n_frames - 1:
                write_cloud(res)
        yield t, res


# ------------------------------------------------------------------------------------------------------------------ asking in words
def _need_grounder(detector, fn):
    if getattr(detector, 'task', None) != 'ground':
        raise ValueError(f'{type(detector).__name__}: {fn} serves the grounding models (run_scene / walk_scene take the others)')


def _prompt_texts(prompts):
    texts = [p if isinstance(p, str) else p.text for p in prompts]
    if not texts:
        raise ValueError('at least one prompt is needed')
    return texts


def sweeps_pipeline(pipeline):
    """the frame-ordered form of a transform list, as the cont-* configurations write it: AggregateMultiViewPoints(save_slices=True), no
    top-level PointSample (it would re-draw the aggregated cloud over all frames, the ones not yet seen included), ConstructMultiSweeps
    before the packing.  The cloud of such a scan is every frame's view sample, in frame order.  A list that already is one: unchanged."""
    from .datasets.loading import ScanPipeline
    if isinstance(pipeline, ScanPipeline) or any(t['type'].split('.')[-1] == 'ConstructMultiSweeps' for t in pipeline):
        return pipeline
    out = []
    for t in pipeline:
        ty = t['type'].split('.')[-1]
        if ty == 'PointSample':
            continue
        if ty == 'Pack3DDetInputs':
            out.append(dict(type='ConstructMultiSweeps'))
        out.append(dict(t, save_slices=True) if ty == 'AggregateMultiViewPoints' else t)
    if not any(t['type'].split('.')[-1] == 'ConstructMultiSweeps' for t in out):
        out.append(dict(type='ConstructMultiSweeps'))
    return out


def prompt_palette(n):
    """(n, 3) u8: row p = the colour of prompt p (render.class_palette without its grey row 0)"""
    return RD.class_palette(n + 1)[1:]


def draw_answers(frames, extrinsic, intrinsic, answers, palette_dev):
    """the answers of every prompt (a list of InstanceData, one per prompt) over frames (V, 3, H, W) u8, each prompt's boxes in its own
    colour -> (V, H, W, 3) u8 on the device"""
    boxes = torch.cat([a.bboxes_3d.tensor.reshape(-1, 9) for a in answers])
    colors = torch.cat([palette_dev[p:p + 1].expand(len(a.scores_3d), 3) for p, a in enumerate(answers)])
    return RD.render_boxes(frames, extrinsic, intrinsic, boxes, colors.contiguous(), layout='chw')


def _answer_painter(dir, detector, texts, dscan):
    return _painter(dir, texts, prompt_palette(len(texts)), dscan, detector.device, draw_answers)


def _selected(res, select):
    return res if select is None else select_answers(res, **select)


def ground_scene(detector, scene_dir, pipeline, prompts, seed=0, select=dict(), render=None):
    """ask a recording in words: the folder is loaded and encoded ONCE (encode_scene), every prompt is grounded on that encoding and
    select_answers makes the answers.  -> one InstanceData(bboxes_3d, scores_3d, keep) per prompt; select: keyword arguments of
    select_answers, None: the raw result of ground() (Q rows per prompt).  render: a directory that receives every view of the scan
    under the answers, one colour per PROMPT, as frame_0000.png ... and legend.json (prompt -> colour); None: nothing is drawn."""
    _need_grounder(detector, 'ground_scene')
    texts = _prompt_texts(prompts)
    dscan = load_scene(detector, scene_dir, pipeline, seed)
    data = detector.data_preprocessor(PL.make_batch([dscan]), False)
    scene = detector.encode_scene(data['inputs'], data['data_samples'])[0]
    res = _selected(detector.ground(scene, prompts), select)
    if render is not None:
        _answer_painter(render, detector, texts, dscan)(res)
    return res


def ask_walk(detector, scene_dir, pipeline, prompts, seed=0, select=dict(), every=1, max_frames=None, render=None):
    """generator over the frames of the folder: opens a GroundWalk, feeds it frame by frame (the frame-ordered form of the pipeline:
    sweeps_pipeline) and, every `every` frames and behind the last one, yields (t, the answers per prompt for frames 0 .. t) -- the
    questions are answered while the walk goes on, and a frame seen once is not paid for again.  select as in ground_scene.  render: a
    directory that receives frame t under the answers of prefix t (the frames that yield) and legend.json; None: nothing is drawn."""
    _need_grounder(detector, 'ask_walk')
    texts = _prompt_texts(prompts)
    every = int(every)
    if every < 1:
        raise ValueError(f'ask_walk: every = {every}')
    dscan = load_scene(detector, scene_dir, sweeps_pipeline(pipeline), seed)
    walk, n_frames, frames = _scene_walk(detector, dscan, PL.make_batch([dscan]), max_frames, capped=True)
    paint = None if render is None else _answer_painter(render, detector, texts, dscan)
    for t, frame in frames:
        walk.observe(*frame)
        if (t + 1) % every and t + 1 != n_frames:
            continue
        res = _selected(walk.ask(prompts), select)
        if paint is not None:
            paint(res, t)
        yield t, res


# ------------------------------------------------------------------------------------------------------------------ the command line
def _class_names(cfg, n):
    mi = cfg.get('metainfo') or {}
    names = list(mi.get('classes', ())) if isinstance(mi, dict) else []
    return names if len(names) >= n else names + [f'class_{i}' for i in range(len(names), n)]


def _record(res, names, **extra):
    if isinstance(res, InstanceData):
        labels = res.labels_3d.cpu().tolist()
        if 'cloud_support' in res:                                       # (a cloud is kept and this list labelled it)
            extra = dict(extra, support=res.cloud_support.cpu().tolist())
        return dict(extra, boxes=res.bboxes_3d.tensor.cpu().tolist(), scores=res.scores_3d.cpu().tolist(), labels=labels,
                    class_names=[names[l] for l in labels])
    hist = torch.bincount(res.reshape(-1)).cpu().tolist()
    return dict(extra, shape=list(res.shape), class_histogram=hist)


def _answer_records(t, texts, answers):
    return [dict(t=t, prompt=tx, boxes=a.bboxes_3d.tensor.cpu().tolist(), scores=a.scores_3d.cpu().tolist(), keep=a.keep.cpu().tolist())
            for tx, a in zip(texts, answers)]


def _emit(a, doc):
    doc = json.dumps(doc)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(doc)
    else:
        print(doc)
    return 0


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m embodiedscan_amd.inference', description=__doc__.split('\n\n')[0])
    ap.add_argument('config')
    ap.add_argument('checkpoint', nargs='?', default=None)
    ap.add_argument('--root-dir', required=True, help='directory that holds the scene folders')
    ap.add_argument('--scene', default='office')
    ap.add_argument('--device', default='cuda:0')
    ap.add_argument('--walk', action='store_true', help='frame by frame through a walk session (continuous models)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--iou-thr', type=float, default=None, help='default: 0.15 (object list), 0.25 (answers of a grounder)')
    ap.add_argument('--score-thr', type=float, default=None, help='default: 0.075 (object list), 0.0 (answers of a grounder)')
    ap.add_argument('--topk-per-class', type=int, default=10)
    ap.add_argument('--prompt', action='append', default=[], metavar='TEXT', help='a question for a grounding model (repeatable)')
    ap.add_argument('--prompts-file', default=None, metavar='F', help='one prompt per line')
    ap.add_argument('--topk', type=int, default=1, help='answers per prompt (grounding models)')
    ap.add_argument('--out', default=None, help='JSON file (default: standard output)')
    ap.add_argument('--render', default=None, metavar='DIR', help='write every frame under its prediction as DIR/frame_0000.png ... and DIR/legend.json')
    ap.add_argument('--map', default=None, metavar='DIR', help='write the scene seen from above as DIR/map.png (--walk: DIR/map_0000.png ...), DIR/map.json and DIR/legend.json')
    ap.add_argument('--map-cell', type=float, default=None, metavar='M', help='side of a map cell in metres (default: 0.02)')
    ap.add_argument('--map-z', type=float, nargs=2, default=None, metavar=('ZMIN', 'ZMAX'), help='the map shows points with ZMIN <= z < ZMAX (default: -1 2)')
    ap.add_argument('--cloud', default=None, metavar='DIR', help='write the scene in three dimensions as DIR/scene.ply (the labelled colour cloud), DIR/boxes.ply or DIR/occupancy.ply and DIR/cloud.json')
    ap.add_argument('--cloud-cell', type=float, default=None, metavar='M', help='side of a cloud voxel in metres (default: 0.02)')
    ap.add_argument('--cloud-min-hits', type=int, default=None, metavar='N', help='keep the voxels that at least N depth pixels fell into (default: 1)')
    ap.add_argument('--cloud-every', type=int, default=None, metavar='K', help='with --walk: also write DIR/scene_<t>.ply ... for every K-th frame (default: only the final files)')
    ap.add_argument('--track', action='store_true', help='with --walk on a cont-det3d configuration: stable object identities over the walk (track_ids)')
    ap.add_argument('--track-iou', type=float, default=None, metavar='X', help='a detection continues a track above this IoU (default: 0.25)')
    ap.add_argument('--track-max-age', type=int, default=None, metavar='K', help='a track unmatched for more than K frames dies (default: never)')
    a = ap.parse_args(argv)
    prompts = list(a.prompt)
    if a.prompts_file is not None:
        with open(a.prompts_file) as f:
            prompts += [ln.strip() for ln in f if ln.strip()]
    from . import models  # noqa: F401  (fills the registry)
    from .config import load_config
    from .registry import MODELS
    cfg = load_config(a.config)
    grounder = getattr(MODELS.get(cfg['model']['type']), 'task', None) == 'ground'   # the class the configuration names: a grounding model?
    if grounder and not prompts:                                         # (both refusals before the model is built)
        ap.error(f"{cfg['model']['type']} grounds prompts: give --prompt TEXT (repeatable) or --prompts-file F")
    if prompts and not grounder:
        ap.error(f"{cfg['model']['type']} takes no prompt: --prompt / --prompts-file go with a grounding configuration")
    if grounder and a.map is not None:
        ap.error('--map goes with the detection and occupancy configurations (a grounding run draws its answers with --render)')
    if a.map is None and (a.map_cell is not None or a.map_z is not None):
        ap.error('--map-cell / --map-z shape the map that --map DIR writes: give --map DIR')
    if grounder and a.cloud is not None:
        ap.error('--cloud goes with the detection and occupancy configurations')
    if a.cloud is None and (a.cloud_cell is not None or a.cloud_min_hits is not None or a.cloud_every is not None):
        ap.error('--cloud-cell / --cloud-min-hits / --cloud-every shape what --cloud DIR writes: give --cloud DIR')
    if a.cloud_every is not None and not a.walk:
        ap.error('--cloud-every numbers the clouds of a walk: it goes with --walk')
    mp = dict(map=a.map, map_cell=0.02 if a.map_cell is None else a.map_cell, map_z=(-1.0, 2.0) if a.map_z is None else tuple(a.map_z),
              cloud=a.cloud, cloud_cell=0.02 if a.cloud_cell is None else a.cloud_cell, cloud_min_hits=1 if a.cloud_min_hits is None else a.cloud_min_hits)
    wk = dict(mp, cloud_every=a.cloud_every or 0)
    tracked = a.track or a.track_iou is not None or a.track_max_age is not None
    if tracked:                                                          # (refused before the model is built as well)
        cls = MODELS.get(cfg['model']['type'])
        if not (a.track and a.walk and getattr(cls, 'task', None) == 'det3d' and getattr(cls, 'continuous', False)):
            ap.error('--track [--track-iou X] [--track-max-age K] follows the objects of a walk: it goes with --walk on a cont-det3d '
                     f"configuration (got {cfg['model']['type']}{', --walk' if a.walk else ', no --walk'}{'' if a.track else ', no --track'})")
    det, cfg = init_model(cfg, a.checkpoint, a.device)
    scene_dir = os.path.join(a.root_dir, a.scene)
    pipe = pipeline_of(cfg)
    if grounder:
        sel = dict(iou_thr=0.25 if a.iou_thr is None else a.iou_thr, score_thr=0.0 if a.score_thr is None else a.score_thr, topk=a.topk)
        if a.walk:
            results = [r for t, ans in ask_walk(det, scene_dir, pipe, prompts, a.seed, sel, render=a.render) for r in _answer_records(t, prompts, ans)]
        else:
            ans = ground_scene(det, scene_dir, pipe, prompts, a.seed, sel, render=a.render)
            results = _answer_records(None, prompts, ans)                 # (t: the last frame of the prefix; null: the whole recording)
        return _emit(a, dict(scene=f'demo/{a.scene}', config=str(a.config), model=type(det).__name__, walk=bool(a.walk), select=sel, results=results))
    flt = dict(iou_thr=0.15 if a.iou_thr is None else a.iou_thr, score_thr=0.075 if a.score_thr is None else a.score_thr,
               topk_per_class=a.topk_per_class)
    kind = _kind(det)
    nc = getattr(det.bbox_head, 'num_classes', 0)
    names = _class_names(cfg, nc) if kind in ('det3d', 'cont-det3d') else ['empty'] + _class_names(cfg, max(nc - 1, 0))
    if a.walk and tracked:
        trk = dict(({} if a.track_iou is None else dict(iou_thr=a.track_iou)), **({} if a.track_max_age is None else dict(max_age=a.track_max_age)))
        results = [_record(r, names, t=t, track_ids=r.track_ids.cpu().tolist())
                   for t, r in walk_scene(det, scene_dir, pipe, a.seed, flt, render=a.render, class_names=names, track=trk, **wk)]
        return _emit(a, dict(scene=f'demo/{a.scene}', config=str(a.config), model=type(det).__name__, walk=True, filter=flt, track=trk, results=results))
    if a.walk:
        results = [_record(r, names, t=t) for t, r in walk_scene(det, scene_dir, pipe, a.seed, flt, render=a.render, class_names=names, **wk)]
    else:
        results = [_record(r, names, t=t) for t, r in enumerate(run_scene(det, scene_dir, pipe, a.seed, flt, render=a.render, class_names=names, **mp))]
    return _emit(a, dict(scene=f'demo/{a.scene}', config=str(a.config), model=type(det).__name__, walk=bool(a.walk), filter=flt, results=results))


if __name__ == '__main__':
    raise SystemExit(main())
