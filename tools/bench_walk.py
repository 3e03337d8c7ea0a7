"""Per-observation latency of the walk sessions against what a user has without them.

    python tools/bench_walk.py [--reps 20] [--frames 50] [--at 0 9 24 49] [--precision bf16] [--models det occ] [--out profiles/walk_session.txt]

One synthetic walk of T = 50 frames with 10 000 points per frame: cont-det3d at 480 x 640 and cont-occ at its shipped 480 x 480, both at
the shipped widths.  At every t of --at:
  session   walk.observe(frame t, the rows frame t adds, its matrices) on a session that has seen frames 0 .. t-1
  baseline  the parent detector's predict on (cloud t, views 0 .. t) as a batch of one -- SparseFeatureFusionSingleStage3DDetector /
            DenseFusionOccPredictor on the same weights -- in its cheapest form: images preprocessed and on the device, the cloud a
            row-prefix view of one device buffer
Both sides run in this process and alternate inside every repetition; every shape is warmed three times first (eager, capture, replay
of the image backbone's launch graph); the clock is the host's around work that ends in a device synchronise; median of >= 20 with
[min, max].  The session is put back to "has seen 0 .. t-1" outside the timed region.  Also: the baseline's peak device memory at the
last t (a pass of its own, before the session exists), the session's state bytes and the peak device memory of a pass of its own over
the whole walk, and the share of observe(t = last) spent in re-voxelising the cloud so far (sparse.voxelize / voxelize_range on it,
timed alone the same way).  One JSON line per record.
There is no CPU path: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = []


def emit(d):
    line = json.dumps(d)
    LINES.append(line)
    print(line, flush=True)


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(ts):
    ts = sorted(ts)
    return dict(median_ms=round(ts[len(ts) // 2], 3), min_ms=round(ts[0], 3), max_ms=round(ts[-1], 3))


def sweep_scan(T, img_size, seed=5):
    """a synthetic scan as a sweeps pipeline hands it over: all T x 10 000 points in frame order and the slice indices"""
    from embodiedscan_amd.synth import make_scan
    scan = make_scan(seed, n_views=T, height=480, width=640, img_size=img_size, n_points=T * 10000, n_boxes=20, augment=False)
    order = np.argsort(scan['sel_view'], kind='stable')
    scan['sel_view'], scan['sel_pix'] = scan['sel_view'][order], scan['sel_pix'][order]
    scan['points_slice_indices'] = [0] + np.cumsum(np.bincount(scan['sel_view'], minlength=T)).tolist()
    return scan


def _const_meta(metainfo):
    d2i = metainfo['depth2img']
    return dict(metainfo, depth2img={k: v for k, v in d2i.items() if k not in ('extrinsic', 'intrinsic')})


def _rollback(walk, snap):
    """the session as it was before the observe that has just been timed"""
    walk.t, walk.cloud.n = snap['t'], snap['n']
    walk.meta.pop()
    if snap.get('sum') is not None:
        walk.sum.copy_(snap['sum'])
        walk.nvalid.copy_(snap['nvalid'])


def run(model, T, at, reps, dev):
    from embodiedscan_amd import pipeline, sparse
    from embodiedscan_amd.config import build_detector, load_config
    from embodiedscan_amd.structures import Det3DDataSample
    occ = model == 'occ'
    name, parent_name, parent_type = (('cont_occ.py', 'mv_occ.py', 'DenseFusionOccPredictor') if occ else
                                      ('cont_det3d.py', 'cont_det3d.py', 'SparseFeatureFusionSingleStage3DDetector'))
    img_size = (480, 480) if occ else (480, 640)
    det = build_detector(load_config(os.path.join(ROOT, 'configs', name)), device=dev, seed=0).to(dev)
    pcfg = load_config(os.path.join(ROOT, 'configs', parent_name))
    pcfg['model']['type'] = parent_type
    pcfg['model']['data_preprocessor']['batchwise_inputs'] = False
    ref = build_detector(pcfg, device=dev, seed=0).to(dev)
    assert torch.equal(ref.arena.data, det.arena.data), 'the parent detector does not carry the same weights'
    scan = sweep_scan(T, img_size)
    dscan = pipeline.upload_scan(scan, dev)
    cloud = pipeline.depth_to_points(dscan)
    pre = ref.data_preprocessor({'inputs': {'points': [cloud], 'img': dscan['img'][None]}, 'data_samples': [Det3DDataSample(scan['meta'])]}, False)
    imgs = pre['inputs']['imgs'].clone()                                    # (1, T, 3, H, W) preprocessed, on the device
    meta = pre['data_samples'][0].metainfo
    d2i = meta['depth2img']
    frames = [(t, r, dict(extrinsic=e, intrinsic=i)) for t, r, e, i in pipeline.walk_frames(dscan, cloud.shape[0])]

    def observe(walk, t):
        _, (r0, r1), m = frames[t]
        return walk.observe(imgs[0, t], cloud[r0:r1], m)

    def baseline(t):
        m = dict(meta, depth2img=dict(d2i, extrinsic=d2i['extrinsic'][:t + 1], intrinsic=d2i['intrinsic'][:t + 1]))
        return ref.forward({'points': [cloud[:frames[t][1][1]]], 'imgs': imgs[:, :t + 1]}, [Det3DDataSample(m)], mode='predict')

    for _ in range(2):                                                      # the baseline's peak memory at the last t, in a pass of its own
        baseline(at[-1])                                                    # (before the session exists: none of its buffers is live)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base_before = torch.cuda.memory_allocated()
    baseline(at[-1])
    torch.cuda.synchronize()
    emit(dict(bench='walk_baseline_memory', model=model, t=at[-1], peak_device_bytes=torch.cuda.max_memory_allocated(),
              allocated_before=base_before))
    walk = det.open_walk(_const_meta(meta)) if occ else det.open_walk(_const_meta(meta), max_frames=T)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base_mem = torch.cuda.memory_allocated()
    for t in range(T):                                                      # a pass of its own: warm-up and the session's peak memory
        observe(walk, t)
    torch.cuda.synchronize()
    emit(dict(bench='walk_session_memory', model=model, T=T, image=list(img_size), state_bytes=walk.state_bytes(),
              peak_device_bytes_over_the_walk=torch.cuda.max_memory_allocated(), allocated_before_the_walk=base_mem))
    walk.reset()
    for t in range(T):
        if t in at:
            snap = dict(t=walk.t, n=walk.cloud.n, sum=None if not occ or walk.sum is None else walk.sum.clone(),
                        nvalid=None if not occ or walk.nvalid is None else walk.nvalid.clone())
            for _ in range(3):                                              # every shape warmed on both sides
                observe(walk, t)
                _rollback(walk, snap)
                baseline(t)
            ts, tb = [], []
            for _ in range(reps):                                           # alternate inside every repetition
                ts.append(_timed(lambda: observe(walk, t)))
                _rollback(walk, snap)
                tb.append(_timed(lambda: baseline(t)))
            s, b = _stats(ts), _stats(tb)
            rec = dict(bench='walk_observe', model=model, t=t, reps=reps, cloud_rows=frames[t][1][1], session=s, baseline=b,
                       speedup_median=round(b['median_ms'] / s['median_ms'], 3))
            if t == at[-1]:
                pts = [cloud[:frames[t][1][1]]]
                if occ:
                    cmax = [k * det.voxel_stride - 1 for k in det.n_voxels]
                    vox = lambda: sparse.voxelize_range(pts, det.point_cloud_range[:3], det.voxel_size, cmax)      # noqa: E731
                else:
                    vox = lambda: sparse.voxelize(pts, det.voxel_size)                                             # noqa: E731
                for _ in range(3):
                    vox()
                v = _stats([_timed(vox) for _ in range(reps)])
                rec.update(revoxelise=v, revoxelise_share_of_observe=round(v['median_ms'] / s['median_ms'], 3))
            emit(rec)
        observe(walk, t)
    torch.cuda.synchronize()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--frames', type=int, default=50)
    ap.add_argument('--at', type=int, nargs='+', default=[0, 9, 24, 49])
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'f32'])
    ap.add_argument('--models', nargs='+', default=['det', 'occ'], choices=['det', 'occ'])
    ap.add_argument('--out', default=None, help='also write the JSON lines to this file')
    a = ap.parse_args()
    assert a.reps >= 20, 'at least 20 repetitions'
    at = sorted(t for t in a.at if t < a.frames)
    assert at and a.frames <= 64
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_walk.py needs the GPU: there is no CPU path')
    from embodiedscan_amd import engine as _E
    _E.PRECISION[0] = a.precision
    emit(dict(bench='walk', precision=a.precision, frames=a.frames, points_per_frame=10000, device=torch.cuda.get_device_name(0)))
    for model in a.models:
        run(model, a.frames, at, a.reps, torch.device('cuda:0'))
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')
