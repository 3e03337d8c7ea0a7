"""Time the device detection metric (embodiedscan_amd/eval) on a synthetic validation set of realistic size against the
composition that existed before it: es_box3d_iou on every (scene, class) block, a device-to-host copy of each block, and the host
loop of tests/det_metric_spec.py (the reference's marking and curves in numpy).

    python tools/bench_det_metric.py [--scans 200 --preds 1000 --gt 80 --classes 284 --repeat 5 --warmup 2 --out FILE.json]

Predictions are jittered copies of the scan's ground truth (80 % keep the class), so a real share of the IoUs is non-zero.
Reported: wall time of the device evaluator (host clock around the call, ended by a device synchronise; median and spread over
--repeat runs after --warmup), its per-entry-point device time (events around each launch sequence; the rest is the torch
grouping and the final copy), the number of same-scene same-class pairs, and the composition's time (alternating with the device
path in the same process).  Both paths must give the same TP totals and APs within one f32 ulp, or the script fails.
Needs the GPU: there is no CPU timing."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

ENTRY = ('es_det_best_gt', 'es_sort_u64', 'es_det_mark', 'es_det_ap')


def make_set(n_scans, n_pred, n_gt, C, seed=0):
    g = np.random.default_rng(seed)
    scenes = []
    for _ in range(n_scans):
        gb = np.concatenate([g.uniform(-5, 5, (n_gt, 3)), g.uniform(0.3, 2.0, (n_gt, 3)), g.uniform(-3.1, 3.1, (n_gt, 3))], 1).astype(np.float32)
        gl = g.integers(0, C, n_gt)
        src = g.integers(0, n_gt, n_pred)
        pb = gb[src].copy()
        pb[:, :3] += g.normal(0, 0.15, (n_pred, 3)).astype(np.float32)
        pb[:, 3:6] *= g.uniform(0.7, 1.4, (n_pred, 3)).astype(np.float32)
        pb[:, 6:] += g.normal(0, 0.2, (n_pred, 3)).astype(np.float32)
        pl = np.where(g.random(n_pred) < 0.8, gl[src], g.integers(0, C, n_pred))
        scenes.append((pb, g.random(n_pred).astype(np.float32), pl, gb, gl))
    return scenes


def composition(scenes_dev, scenes, C, thr, S):
    """what the repository could do before: the IoU kernel per (scene, class) block, each block copied to the host, first-maximum and
    marking and curves on the host"""
    from embodiedscan_amd import hip
    iou_max, gt_best = [], []
    g0 = 0
    for (pb, pl, gb, gl), sc in zip(scenes_dev, scenes):
        thin = ((pb[:, 3] * pb[:, 4] < 2e-4) | (pb[:, 3] * pb[:, 5] < 2e-4) | (pb[:, 5] * pb[:, 4] < 2e-4))[:, None]
        pb = torch.cat((pb[:, :3], torch.where(thin, pb[:, 3:6].clamp(min=2e-2), pb[:, 3:6]), pb[:, 6:]), 1)
        m = np.full(len(sc[2]), -np.inf, np.float32)
        j = np.full(len(sc[2]), -1, np.int64)
        for c in np.unique(sc[4]):
            rows_p, rows_g = np.nonzero(sc[2] == c)[0], np.nonzero(sc[4] == c)[0]
            if len(rows_p) == 0:
                continue
            a, b = pb[torch.from_numpy(rows_p).to(pb.device)].contiguous(), gb[torch.from_numpy(rows_g).to(pb.device)].contiguous()
            out = torch.empty((len(rows_p), len(rows_g)), dtype=torch.float32, device=pb.device)
            hip.call('es_box3d_iou', hip.P(a), len(rows_p), hip.P(b), len(rows_g), hip.P(out), hip.stream())
            v = out.cpu().numpy()
            k = v.argmax(1)                                   # (numpy's argmax returns the first maximum)
            m[rows_p], j[rows_p] = v[np.arange(len(k)), k], g0 + rows_g[k]
        iou_max.append(m)
        gt_best.append(j)
        g0 += len(sc[4])
    return S.evaluate(scenes, C, thr, best=(np.concatenate(iou_max), np.concatenate(gt_best)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scans', type=int, default=200)
    ap.add_argument('--preds', type=int, default=1000)
    ap.add_argument('--gt', type=int, default=80)
    ap.add_argument('--classes', type=int, default=284)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--composition-repeat', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_det_metric.py measures on the GPU; none found')
    import det_metric_spec as S
    from embodiedscan_amd import hip
    from embodiedscan_amd.eval.indoor_eval import evaluate_device, flatten_annos
    dev = torch.device('cuda:0')
    thr, C = [0.25, 0.5], args.classes
    scenes = make_set(args.scans, args.preds, args.gt, C)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dev)
    gt = [dict(gt_bboxes_3d=t(s[3]), gt_labels_3d=t(s[4])) for s in scenes]
    dt = [dict(bboxes_3d=t(s[0]), scores_3d=t(s[1]), labels_3d=t(s[2])) for s in scenes]
    scenes_dev = [(d['bboxes_3d'], d['labels_3d'], g['gt_bboxes_3d'], g['gt_labels_3d']) for d, g in zip(dt, gt)]
    pairs = int(sum((np.bincount(s[2], minlength=C) * np.bincount(s[4], minlength=C)).sum() for s in scenes))

    def device_path():
        pred, gtt = flatten_annos(gt, dt, dev)
        out = evaluate_device(pred, gtt, C, thr)
        return out['ap'].cpu().numpy(), out['tp_total'].cpu().numpy()         # (the copy ends the work: a synchronise)

    for _ in range(args.warmup):
        device_path()
    torch.cuda.synchronize()
    wall, comp, stage = [], [], {k: [] for k in ENTRY}
    ref = None
    for r in range(args.repeat):
        hip.PROFILE = dict(names=set(ENTRY), records=[], event=lambda: torch.cuda.Event(enable_timing=True))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ap_dev, tot_dev = device_path()
        wall.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        for k in ENTRY:
            stage[k].append(sum(e0.elapsed_time(e1) for name, e0, e1, _ in hip.PROFILE['records'] if name == k))
        hip.PROFILE = None
        if r < args.composition_repeat:                       # alternating with the device path
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = composition(scenes_dev, scenes, C, thr, S)
            comp.append((time.perf_counter() - t0) * 1e3)
    ok = np.array_equal(tot_dev, ref['tp_total'])
    both = ~np.isnan(ref['ap'])
    ulp = np.spacing(np.abs(ref['ap'][both]))
    ok = ok and np.array_equal(np.isnan(ap_dev), ~both) and bool((np.abs(ap_dev[both] - ref['ap'][both]) <= ulp).all())
    med = statistics.median
    res = dict(scans=args.scans, preds_per_scan=args.preds, gt_per_scan=args.gt, classes=C, thresholds=thr, pairs=pairs,
               device_wall_ms=dict(median=med(wall), min=min(wall), max=max(wall), runs=wall),
               device_stage_ms={k: med(v) for k, v in stage.items()},
               device_other_ms=med(wall) - sum(med(v) for v in stage.values()),
               composition_wall_ms=dict(median=med(comp), runs=comp), speedup=med(comp) / med(wall), same_results=bool(ok),
               mAP_0p25=float(np.nanmean(ap_dev[0][both[0]])))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    if not ok:
        raise SystemExit('the device path and the composition disagree')


if __name__ == '__main__':
    main()
