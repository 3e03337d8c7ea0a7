"""Time GroundingMetric and OccupancyMetric (embodiedscan_amd/eval) on synthetic validation sets of realistic size against the
compositions that existed before them, on the same device tensors.

    python tools/bench_eval_metrics.py [--ground-samples 5000 --queries 256 --occ-volumes 1000 --rows 10000 --repeat 3 --warmup 1 --out FILE.json]

Grounding (5 000 samples x 256 queries, batches of --ground-batch): `process` per batch + `evaluate`, against the earlier
composition -- per sample a torch argsort, es_box3d_iou on the top-10 block, a copy of the block to the host and the host loop of
the reference's ground_eval, with every sample's boxes and scores retained until the end.
Occupancy (1 000 volumes of 40 x 40 x 16, 81 labels): `process` per batch + `evaluate`, against the reference's process (dense int64
ground truth by index_put, retained beside the prediction) and its per-class masked loop in torch.
Continuous occupancy (T = 10 prefixes): --rows confusion rows through gather_results on one rank (backend --backend).

Reported per workload: wall time per `process` batch (host clock around the loop over the batches, ended by a device synchronise,
divided by the number of batches; median and spread over --repeat runs after --warmup), wall time of `evaluate`, the device bytes
held between the batches (torch.cuda.memory_allocated after the last batch minus before the first), and whether the dicts are
identical.  The compositions alternate with the new path in the same process.  Needs the GPU: there is no CPU timing."""
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

TYPES = ('Easy', 'Hard', 'View-Dep', 'View-Indep', 'Unique', 'Multi', 'Overall')


def sync_ms(t0):
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def make_ground(n, Q, dev, seed=0):
    """per sample: 1 .. 3 ground-truth boxes, Q predictions jittered around them, distinct random target scores, three flags"""
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, device=dev)
    flags = torch.randint(0, 8, (n,), generator=g, device=dev).tolist()
    n_gt = torch.randint(1, 4, (n,), generator=g, device=dev).tolist()
    out = []
    for i in range(n):
        gt = torch.cat([r(n_gt[i], 3) * 8 - 4, r(n_gt[i], 3) * 1.5 + 0.4, r(n_gt[i], 3) * 6.2 - 3.1], 1)
        boxes = gt[torch.randint(0, n_gt[i], (Q,), generator=g, device=dev)].clone()
        boxes[:, :3] += (r(Q, 3) - 0.5) * 1.2
        boxes[:, 3:6] *= r(Q, 3) * 0.8 + 0.6
        boxes[:, 6:] += (r(Q, 3) - 0.5) * 0.5
        pred = dict(bboxes_3d=boxes, target_scores_3d=r(Q), scores_3d=r(Q))
        ann = dict(gt_bboxes_3d=gt, is_view_dep=bool(flags[i] & 1), is_hard=bool(flags[i] & 2), is_unique=bool(flags[i] & 4))
        out.append(dict(pred_instances_3d=pred, eval_ann_info=ann))
    return out


def ground_composition(samples, thr):
    """what the repository could do before: argsort + es_box3d_iou per sample, the block copied to the host, ground_eval's loop"""
    from embodiedscan_amd import hip
    pred = {f'{ty}@{t}': 0 for t in thr for ty in TYPES}
    gt = {f'{ty}@{t}': 1e-14 for t in thr for ty in TYPES}
    for s in samples:
        p, a = s['pred_instances_3d'], s['eval_ann_info']
        top = p['bboxes_3d'][p['target_scores_3d'].argsort(dim=-1, descending=True)[:10]].contiguous()
        g = a['gt_bboxes_3d'].contiguous()
        iou = torch.empty((top.shape[0], g.shape[0]), dtype=torch.float32, device=top.device)
        hip.call('es_box3d_iou', hip.P(top), top.shape[0], hip.P(g), g.shape[0], hip.P(iou), hip.stream())
        iou = iou.cpu()
        for t in thr:
            found = int((iou > t).any())
            for ty in ('View-Dep' if a['is_view_dep'] else 'View-Indep', 'Hard' if a['is_hard'] else 'Easy',
                       'Unique' if a['is_unique'] else 'Multi', 'Overall'):
                gt[f'{ty}@{t}'] += 1
                pred[f'{ty}@{t}'] += found
    return {f'{ty}@{t}': pred[f'{ty}@{t}'] / max(gt[f'{ty}@{t}'], 1) for t in thr for ty in TYPES}


def make_occ(n, shape, n_labels, dev, seed=1):
    """per volume: 12 % occupied voxels as an (M,4) list, a prediction that agrees on most, an 80 % mask"""
    g = torch.Generator(device=dev).manual_seed(seed)
    X, Y, Z = shape
    nv = X * Y * Z
    out = []
    for _ in range(n):
        flat = torch.randperm(nv, generator=g, device=dev)[:nv // 8]          # no duplicates: index_put on a device leaves their winner open
        lab = torch.randint(1, n_labels, (nv // 8,), generator=g, device=dev)
        lst = torch.stack([flat // (Y * Z), (flat // Z) % Y, flat % Z, lab], 1)
        dense = torch.zeros(nv, dtype=torch.int64, device=dev)
        dense[flat] = lab
        noise = torch.rand(nv, generator=g, device=dev) < 0.2
        pred = torch.where(noise, torch.randint(0, n_labels, (nv,), generator=g, device=dev), dense).reshape(shape)
        out.append(dict(pred_occupancy=pred, gt_occupancy=lst, gt_occupancy_masks=(torch.rand(shape, generator=g, device=dev) < 0.8)))
    return out


def occ_reference_process(samples):
    """OccupancyMetric.process of the reference: one dense int64 ground truth per sample, retained beside the prediction"""
    results = []
    for s in samples:
        pred, gt4 = s['pred_occupancy'], s['gt_occupancy']
        gt = torch.zeros_like(pred)
        gt[gt4[:, 0], gt4[:, 1], gt4[:, 2]] = gt4[:, 3]
        gt[~s['gt_occupancy_masks']] = 255
        results.append((gt, pred))
    return results


def occ_reference_compute(results, classes):
    """compute_metrics of the reference: the per-class masked loop (the running score kept on the device, copied once)"""
    C = len(classes) + 1
    score = torch.zeros((C, 3), dtype=torch.float64, device=results[0][0].device)
    for gt, pred in results:
        mask = gt != 255
        g, p = gt[mask], pred[mask]
        for j in range(C):
            if j == 0:
                score[j, 0] += ((g != 0) * (p != 0)).sum()
                score[j, 1] += (g != 0).sum()
                score[j, 2] += (p != 0).sum()
            else:
                score[j, 0] += ((g == j) * (p == j)).sum()
                score[j, 1] += (g == j).sum()
                score[j, 2] += (p == j).sum()
    score = score.cpu().numpy()
    ret = {}
    with np.errstate(all='ignore'):
        for i in range(C):
            tp, p, g = score[i]
            if not np.isnan(tp / (p + g - tp)):
                ret['empty' if i == 0 else classes[i - 1]] = float(tp / (p + g - tp))
    return ret


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=v)


def run_metric(metric, samples, batch, size):
    """-> (ms per process batch, ms of evaluate, device bytes held between the batches, dict)"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    for i in range(0, len(samples), batch):
        metric.process({}, samples[i:i + batch])
    t_process = sync_ms(t0)
    held = torch.cuda.memory_allocated() - base
    t0 = time.perf_counter()
    ret = metric.evaluate(size)
    return t_process / ((len(samples) + batch - 1) // batch), sync_ms(t0), held, ret


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ground-samples', type=int, default=5000)
    ap.add_argument('--queries', type=int, default=256)
    ap.add_argument('--ground-batch', type=int, default=50)
    ap.add_argument('--occ-volumes', type=int, default=1000)
    ap.add_argument('--occ-batch', type=int, default=4)
    ap.add_argument('--occ-labels', type=int, default=81)
    ap.add_argument('--rows', type=int, default=10000)
    ap.add_argument('--backend', default='nccl')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--composition-repeat', type=int, default=1)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_eval_metrics.py measures on the GPU; none found')
    import embodiedscan_amd  # noqa: F401
    from embodiedscan_amd.eval import gather_results
    from embodiedscan_amd.registry import METRICS
    import embodiedscan_amd.eval.grounding_metric as GM
    import embodiedscan_amd.eval.occupancy_metric as OM
    GM._log = OM._log = lambda text, logger: None                       # the tables are not part of the measurement
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    res = {}

    def dump(key):
        print(json.dumps({key: res[key]}), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                json.dump(res, f, indent=1)

    # ---- grounding
    thr = [0.25, 0.5]
    samples = make_ground(args.ground_samples, args.queries, dev)
    metric = METRICS.build(dict(type='GroundingMetric', iou_thr=thr, device=dev))
    proc, ev, held, comp = [], [], [], []
    for r in range(args.warmup + args.repeat):
        p, e, h, ret = run_metric(metric, samples, args.ground_batch, len(samples))
        if r >= args.warmup:
            proc.append(p), ev.append(e), held.append(h)
            if len(comp) < args.composition_repeat:
                t0 = time.perf_counter()
                ref = ground_composition(samples, thr)
                comp.append(sync_ms(t0))
    retained = sum(s['pred_instances_3d'][k].numel() * s['pred_instances_3d'][k].element_size() for s in samples
                   for k in ('bboxes_3d', 'target_scores_3d', 'scores_3d'))
    n_batches = (len(samples) + args.ground_batch - 1) // args.ground_batch
    res['grounding'] = dict(samples=len(samples), queries=args.queries, batch=args.ground_batch, thresholds=thr,
                            process_ms_per_batch=stats(proc), evaluate_ms=stats(ev), total_ms=statistics.median(proc) * n_batches + statistics.median(ev),
                            held_bytes_between_batches=max(held), row_bytes=5 * len(samples),
                            composition_total_ms=stats(comp), composition_retained_bytes=retained,
                            same_results=bool(ret == ref), overall_0p25=ret['Overall@0.25'])
    dump('grounding')
    del samples

    # ---- occupancy
    shape = (40, 40, 16)
    classes = [f'c{k}' for k in range(1, args.occ_labels)]
    vols = make_occ(args.occ_volumes, shape, args.occ_labels, dev)
    metric = METRICS.build(dict(type='OccupancyMetric', device=dev, dataset_meta=dict(classes=classes)))
    proc, ev, held, comp_p, comp_e, comp_held = [], [], [], [], [], []
    for r in range(args.warmup + args.repeat):
        p, e, h, ret = run_metric(metric, vols, args.occ_batch, len(vols))
        if r >= args.warmup:
            proc.append(p), ev.append(e), held.append(h)
            if len(comp_p) < args.composition_repeat:
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                kept = occ_reference_process(vols)
                comp_p.append(sync_ms(t0) / ((len(vols) + args.occ_batch - 1) // args.occ_batch))
                comp_held.append(torch.cuda.memory_allocated() - base)
                t0 = time.perf_counter()
                ref = occ_reference_compute(kept, classes)
                comp_e.append(sync_ms(t0))
                del kept
    res['occupancy'] = dict(volumes=len(vols), shape=shape, labels=args.occ_labels, batch=args.occ_batch,
                            process_ms_per_batch=stats(proc), evaluate_ms=stats(ev), held_bytes_between_batches=max(held),
                            row_bytes=12 * args.occ_labels * len(vols),
                            composition_process_ms_per_batch=stats(comp_p), composition_evaluate_ms=stats(comp_e),
                            composition_held_bytes=max(comp_held), same_results=bool(ret == ref), kept_classes=len(ret))
    dump('occupancy')
    del vols

    # ---- continuous occupancy: the rows of T = 10 prefixes through the gather on one rank
    import torch.distributed as dist
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', '29637')
    dist.init_process_group(args.backend, rank=0, world_size=1)
    rows = torch.randint(0, 1000, (args.rows, 3 * args.occ_labels), dtype=torch.int32, device=dev)
    results = [(rows[i:i + 1],) for i in range(args.rows)]
    gat = []
    for r in range(args.warmup + args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = gather_results(results, None)
        ms = sync_ms(t0)
        if r >= args.warmup:
            gat.append(ms)
    same = len(got) == args.rows and bool(torch.equal(torch.cat([g[0] for g in got]).to(dev), rows))
    dist.destroy_process_group()
    res['cont_occ_gather'] = dict(rows=args.rows, prefixes=10, backend=args.backend, gather_ms=stats(gat), gathered_bytes=rows.numel() * 4,
                                  dense_volume_bytes_instead=args.rows * 2 * shape[0] * shape[1] * shape[2] * 8, same_rows=same)
    dump('cont_occ_gather')
    if not (res['grounding']['same_results'] and res['occupancy']['same_results'] and same):
        raise SystemExit('the new path and the composition disagree')


if __name__ == '__main__':
    main()
