"""Time the scene inventory filter (embodiedscan_amd.inference.filter_instances: es_topk_sorted + ONE launch of es_box3d_iou_filter + the
read of the kept count) against the reference's own composition (demo/demo.py:102-130) on this project's kernels: es_box3d_iou on
the whole n x n matrix, a device-to-host copy of it, and the Python greedy of tests/scene_filter_spec.py on the host.

    python tools/bench_scene_inventory.py [--sizes 256,2048,6000 --repeat 7 --warmup 2 --observe-ms 58.39 --out FILE.txt]

Populations: tests/scene_filter_spec.clustered with n / 8 objects of 8 jittered detections each (5 classes, the demo's thresholds
0.15 / 0.075 / 10 per class, and a second run without a quota, where rows are kept down to the score threshold).  One process, the
two forms alternating, --warmup runs of each first, then --repeat timed runs: a host clock around the call, a device synchronise
before and after.  Reported per form: median [min, max] in ms; for the filter also the device time of its two launches (events).
Both forms must keep the same rows, or the script fails.  --observe-ms: the time of one DetWalk.observe at t = 49
(profiles/walk_session.txt) of which the filter's time at the largest size is reported as a share.  Needs the GPU."""
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


def _fmt(v):
    return f'{statistics.median(v):9.3f} [{min(v):.3f}, {max(v):.3f}]'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='256,2048,6000')
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--observe-ms', type=float, default=58.39)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'this benchmark needs the GPU: there is no CPU timing'
    import scene_filter_spec as S
    from embodiedscan_amd import hip, inference
    from embodiedscan_amd.structures import EulerDepthInstance3DBoxes, InstanceData
    dev = torch.device('cuda:0')
    lines = [f'scene inventory filter against es_box3d_iou n x n + D2H + host greedy; {a.repeat} runs after {a.warmup} warm-up, alternating, '
             f'ms median [min, max]; device {torch.cuda.get_device_name(0)}',
             f'{"n":>6} {"topk":>5} {"kept":>5} | {"filter_instances (wall)":>30} | {"sort + filter launches (events)":>32} | '
             f'{"composition (wall)":>34} | {"matrix":>9} {"copy":>9} {"greedy":>9} | ratio']
    last = None
    for n in [int(v) for v in a.sizes.split(',')]:
        pop = S.clustered(7, n_clusters=max(n // 8, 1))
        m = len(pop['scores'])
        boxes, scores = torch.from_numpy(pop['boxes']).to(dev), torch.from_numpy(pop['scores']).to(dev)
        labels = torch.from_numpy(pop['labels']).long().to(dev)
        inst = InstanceData(bboxes_3d=EulerDepthInstance3DBoxes(boxes), scores_3d=scores, labels_3d=labels)
        iou = torch.empty((m, m), dtype=torch.float32, device=dev)
        for topk in (10, m):
            kw = dict(iou_thr=S.IOU_THR, score_thr=S.SCORE_THR, topk_per_class=topk, n_classes=pop['n_classes'])

            def filt():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = inference.filter_instances(inst, **kw)
                e1.record()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1), out.keep.cpu().tolist()

            def comp():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hip.call('es_box3d_iou', hip.P(boxes), m, hip.P(boxes), m, hip.P(iou), hip.stream())
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                host = iou.cpu().numpy()
                t2 = time.perf_counter()
                kept = S.greedy(host, pop['scores'], pop['labels'], pop['n_classes'], S.IOU_THR, S.SCORE_THR, topk)
                t3 = time.perf_counter()
                return (t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, kept

            for _ in range(a.warmup):
                filt(), comp()
            fw, fe, cw, cm, cc, cg = [], [], [], [], [], []
            for _ in range(a.repeat):
                w, e, k1 = filt()
                fw.append(w), fe.append(e)
                w, mt, cp, gr, k2 = comp()
                cw.append(w), cm.append(mt), cc.append(cp), cg.append(gr)
                assert k1 == k2, f'n = {m}, topk = {topk}: the two forms keep different rows'
            ratio = statistics.median(cw) / statistics.median(fw)
            lines.append(f'{m:6d} {topk:5d} {len(k1):5d} | {_fmt(fw):>30} | {_fmt(fe):>32} | {_fmt(cw):>34} | {statistics.median(cm):9.3f} '
                         f'{statistics.median(cc):9.3f} {statistics.median(cg):9.3f} | {ratio:7.1f} x')
            print(lines[-1], flush=True)
            if topk == 10:
                last = (m, statistics.median(fw))
    if last is not None:
        lines.append(f'filter_instances at n = {last[0]}, quota 10: {last[1]:.3f} ms = {last[1] / a.observe_ms:.1%} of one DetWalk.observe at t = 49 '
                     f'({a.observe_ms} ms, profiles/walk_session.txt)')
    text = '\n'.join(lines) + '\n'
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
