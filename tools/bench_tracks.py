"""Time one update of the track table (embodiedscan_amd.tracks.TrackTable.update: es_box3d_iou into a cached workspace + ONE launch of
es_track_assign, no host synchronisation of its own) against the composition available without it on this project's kernels:
es_box3d_iou on the n x m matrix, a device-to-host copy of it, and the Python greedy of tests/track_spec.py on the host (the table
kept in numpy, as a host tracker would).

    python tools/bench_tracks.py [--sizes 50x200,200x1000,1000x4000 --repeat 7 --warmup 2 --walk-frames 50 --out profiles/tracks.txt]

Populations: m tracks = the objects of tests/scene_filter_spec.clustered (one box per object), n detections = jittered copies of n of
them (4 of 5) and unrelated boxes (1 of 5); thresholds: the table's defaults.  One process, the two forms alternating, --warmup runs
of each first, then --repeat timed runs on the SAME table state (put back outside the timed region): a host clock around the call, a
device synchronise before and after.  Reported per form: median [min, max] in ms; for the update also the device time of its two
launches (events) and the split of the composition.  Both forms must produce the same ids, or the script fails.
Then one frame of a tracked walk: the body of inference.walk_scene -- DetWalk.observe + filter_instances, with and without the table's
update + lookup -- at the last frame of tools/bench_walk.py's synthetic walk (50 frames of 10 000 points at 480 x 640, the table fed
with every earlier frame's filtered list; where the seeded weights give more rows than filter_instances orders, the 16 384 best go
in, on both sides), the session and the table put back outside the timed region.  Needs the GPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def _fmt(v):
    return f'{statistics.median(v):9.3f} [{min(v):.3f}, {max(v):.3f}]'


def population(n, m, seed=7):
    """-> (track boxes (m,9), detections dict(boxes (n,9), scores, labels)): see the module docstring"""
    import scene_filter_spec as F
    rng = np.random.default_rng(seed)
    objs = F.clustered(seed, n_clusters=m, copies=1)['boxes']
    far = F.clustered(seed + 1, n_clusters=n, copies=1)['boxes'] + np.array([100, 0, 0, 0, 0, 0, 0, 0, 0], np.float32)
    src = rng.permutation(m)[:n] if n <= m else rng.integers(0, m, n)
    det = objs[src].copy()
    det[:, :3] += (rng.normal(0, 1, (n, 3)) * 0.07 * det[:, 3:6]).astype(np.float32)
    det[:, 3:6] *= rng.uniform(0.9, 1.1, (n, 3)).astype(np.float32)
    new = rng.random(n) < 0.2
    det[new] = far[new]
    return objs, dict(boxes=det, scores=rng.uniform(0.2, 1, n).astype(np.float32), labels=rng.integers(0, 5, n).astype(np.int32))


def bench_update(n, m, a, dev, lines):
    import track_spec as S
    from embodiedscan_amd import hip
    from embodiedscan_amd.structures import InstanceData
    from embodiedscan_amd.tracks import TrackTable
    cap = min(4096, m + n)
    objs, det = population(n, m)
    table = TrackTable(dev, capacity=cap, iou_thr=2.0)          # (nothing matches while the m tracks are born)
    born = InstanceData(bboxes_3d=torch.from_numpy(objs).to(dev), scores_3d=torch.full((m,), 0.5, device=dev), labels_3d=torch.zeros(m, dtype=torch.long, device=dev))
    for lo in range(0, m, 2048):                               # (an update takes 2048 detections)
        table.update(InstanceData(bboxes_3d=born.bboxes_3d[lo:lo + 2048], scores_3d=born.scores_3d[lo:lo + 2048], labels_3d=born.labels_3d[lo:lo + 2048]))
    assert len(table.inventory().track_ids) == m               # (the read-back makes the host's bound exact: m columns)
    table.iou_thr = S.IOU_THR
    state = [x.clone() for x in (table.boxes, table.f, table.i, table.counts)]
    bound, t_prev = table._bound, table.t
    host0 = dict(boxes=table.boxes.cpu().numpy(), f=table.f.cpu().numpy(), i=table.i.cpu().numpy(), counts=table.counts.cpu().numpy())
    inst = InstanceData(bboxes_3d=torch.from_numpy(det['boxes']).to(dev), scores_3d=torch.from_numpy(det['scores']).to(dev),
                        labels_3d=torch.from_numpy(det['labels']).long().to(dev))
    d_boxes = inst.bboxes_3d.contiguous()
    iou = torch.empty((n, m), dtype=torch.float32, device=dev)

    def restore():
        for x, x0 in zip((table.boxes, table.f, table.i, table.counts), state):
            x.copy_(x0)
        table._bound, table.t = bound, t_prev

    def update():
        restore()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ids = table.update(inst)
        e1.record()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1), ids.cpu().tolist()

    def comp():
        tab = S.copy_table(host0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hip.call('es_box3d_iou', hip.P(d_boxes), n, hip.P(state[0]), m, hip.P(iou), hip.stream())
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host = iou.cpu().numpy()
        t2 = time.perf_counter()
        ids = S.update_spec(tab, cap, t_prev + 1, host, m, det['boxes'], det['scores'], det['labels'])
        t3 = time.perf_counter()
        return (t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, ids.tolist()

    for _ in range(a.warmup):
        update(), comp()
    uw, ue, cw, cm, cc, cg = [], [], [], [], [], []
    for _ in range(a.repeat):
        w, e, k1 = update()
        uw.append(w), ue.append(e)
        w, mt, cp, gr, k2 = comp()
        cw.append(w), cm.append(mt), cc.append(cp), cg.append(gr)
        assert k1 == k2, f'n = {n}, m = {m}: the two forms give different ids'
    matched = sum(1 for i in k1 if 0 <= i < m)
    lines.append(f'{n:6d} {m:6d} {matched:7d} {n - matched:6d} | {_fmt(uw):>30} | {_fmt(ue):>30} | {_fmt(cw):>34} | {statistics.median(cm):9.3f} '
                 f'{statistics.median(cc):9.3f} {statistics.median(cg):9.3f} | {statistics.median(cw) / statistics.median(uw):7.1f} x')
    print(lines[-1], flush=True)


def bench_walk_frame(T, a, dev, lines):
    import bench_walk as BW
    from embodiedscan_amd import inference as I, pipeline
    from embodiedscan_amd.config import build_detector, load_config
    from embodiedscan_amd.structures import Det3DDataSample, InstanceData
    from embodiedscan_amd.tracks import TrackTable
    from embodiedscan_amd import engine as E
    E.PRECISION[0] = 'bf16'                                     # (tools/bench_walk.py's default)
    det = build_detector(load_config(os.path.join(ROOT, 'configs', 'cont_det3d.py')), device=dev, seed=0).to(dev)
    det.train(False)
    scan = BW.sweep_scan(T, (480, 640))
    dscan = pipeline.upload_scan(scan, dev)
    cloud = pipeline.depth_to_points(dscan)
    det.data_preprocessor.batchwise_inputs = False             # (one sample with all T views, as tools/bench_walk.py preprocesses it)
    pre = det.data_preprocessor({'inputs': {'points': [cloud], 'img': dscan['img'][None]}, 'data_samples': [Det3DDataSample(scan['meta'])]}, False)
    imgs = pre['inputs']['imgs'].clone()
    frames = [(t, r, dict(extrinsic=e, intrinsic=i)) for t, r, e, i in pipeline.walk_frames(dscan, cloud.shape[0])]
    walk = det.open_walk(BW._const_meta(pre['data_samples'][0].metainfo), max_frames=T)
    table = TrackTable(dev)
    nc = det.bbox_head.num_classes

    def body(t, tracked):
        _, (r0, r1), m = frames[t]
        raw = walk.observe(imgs[0, t], cloud[r0:r1], m)
        if len(raw.scores_3d) > I.MAX_ROWS:                     # (seeded weights: more rows than filter_instances orders; the best 16384, on both sides)
            top = raw.scores_3d.topk(I.MAX_ROWS).indices
            raw = InstanceData(bboxes_3d=raw.bboxes_3d.tensor[top], scores_3d=raw.scores_3d[top], labels_3d=raw.labels_3d[top])
        res = I.filter_instances(raw, n_classes=nc)
        if tracked:
            res.track_ids = table.update(res, t)
            res.track_hits, res.track_first_seen = table.lookup(res.track_ids)
        return res

    for t in range(T - 1):
        body(t, True)
    torch.cuda.synchronize()
    last = T - 1
    snap = dict(t=walk.t, n=walk.cloud.n)
    state = [x.clone() for x in (table.boxes, table.f, table.i, table.counts)]
    bound, t_prev, nt = table._bound, table.t, int(table.counts[0])

    def timed(tracked):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = body(last, tracked)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        BW._rollback(walk, snap)
        for x, x0 in zip((table.boxes, table.f, table.i, table.counts), state):
            x.copy_(x0)
        table._bound, table.t = bound, t_prev
        return ms, res

    for _ in range(max(a.warmup, 3)):
        timed(True), timed(False)
    with_t, without = [], []
    for _ in range(a.repeat):
        ms, res = timed(True)
        with_t.append(ms)
        without.append(timed(False)[0])
    ids = res.track_ids.cpu().tolist()
    lines.append(f'one frame of a tracked walk at t = {last} (observe + filter_instances; {len(ids)} objects in the list, {nt} tracks in the table, the host bound at '
                 f'{bound} columns, {sum(1 for i in ids if i < nt)} detections continue a track): without the table {_fmt(without)} ms, with update + lookup '
                 f'{_fmt(with_t)} ms, difference of the medians {statistics.median(with_t) - statistics.median(without):+.3f} ms')
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='50x200,200x1000,1000x4000')
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--walk-frames', type=int, default=50, help='0: skip the walk frame')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU: there is no CPU timing'
    dev = torch.device('cuda:0')
    lines = [f'track table update against es_box3d_iou n x m + D2H + host greedy; {a.repeat} runs after {a.warmup} warm-up, alternating, ms median '
             f'[min, max]; device {torch.cuda.get_device_name(0)}',
             f'{"n":>6} {"m":>6} {"matched":>7} {"born":>6} | {"TrackTable.update (wall)":>30} | {"its two launches (events)":>30} | {"composition (wall)":>34} | '
             f'{"matrix":>9} {"copy":>9} {"greedy":>9} | ratio']
    for size in a.sizes.split(','):
        n, m = (int(v) for v in size.split('x'))
        bench_update(n, m, a, dev, lines)
    def write():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
    write()
    if a.walk_frames:
        bench_walk_frame(a.walk_frames, a, dev, lines)
        write()
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
