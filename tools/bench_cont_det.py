"""Time the view-window fusion kernels against the T-launch composition of the kernels they replace, and one continuous train step.

    python tools/bench_cont_det.py [--reps 30] [--warmup 5] [--no-step] [--out profiles/r7_cont_det.txt]

(a) One synthetic walk-through of T = 10 views 480 x 480 with 10 000 points per view: the T cumulative clouds are voxelised as batch
entries 0 .. T-1 and taken through the 3-D backbone's coordinate chain; on each of the four level shapes (rows of that level, image
channels 64 / 128 / 256 / 512 on 120^2 / 60^2 / 30^2 / 15^2 maps)
  forward   es_point_sample_win_fwd (one launch, window table (0, t + 1))
            vs es_point_sample_fwd on the row slice of every prefix with a zeroed batch column and t + 1 views (T launches)
  backward  es_point_sample_win_bwd (one link + one gather)
            vs es_point_sample_bwd per prefix with accumulate = 1 into a zeroed gradient (T links + T gathers over t + 1 images)
Both sides run in this process, alternate inside every repetition, are warmed up first and are timed with device events around the
whole call sequence; median, minimum and maximum over the repetitions go out as one JSON line per (level, direction).  The
composition's zeroed-column coordinates and per-prefix buffers are prepared outside the timed region.
(b) One Embodied3DDetector train step at the shipped widths with T = 10 (the same scan, bf16): milliseconds (median of the timed
steps) and peak device memory.
There is no CPU path: without a GPU the tool fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = []


def emit(d):
    line = json.dumps(d)
    LINES.append(line)
    print(line, flush=True)


def _timed(fn, st):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(ts):
    ts = sorted(ts)
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4))


def sweep_scan(T, seed=5):
    """a synthetic scan as a sweeps pipeline hands it over: all T x 10 000 points in frame order, slice indices, every instance visible"""
    from embodiedscan_amd.synth import make_scan
    scan = make_scan(seed, n_views=T, height=480, width=640, img_size=(480, 480), n_points=T * 10000, n_boxes=20, augment=False)
    order = np.argsort(scan['sel_view'], kind='stable')
    scan['sel_view'], scan['sel_pix'] = scan['sel_view'][order], scan['sel_pix'][order]
    scan['points_slice_indices'] = [0] + np.cumsum(np.bincount(scan['sel_view'], minlength=T)).tolist()
    scan['visible_instance_masks'] = [np.ones(len(scan['gt_labels']), dtype=bool)] * T
    return scan


def kernels(det, dscan, T, reps, warmup, dev):
    from embodiedscan_amd import pipeline, sparse
    from embodiedscan_amd.hip import P, call
    from embodiedscan_amd.models.layers.fusion_layers.point_fusion import build_fusion_meta
    V, H, W = T, 480, 480
    det._bind()                                                 # the backbones build their blocks when they are bound to the arena
    batch = pipeline.make_cont_det_batch(dscan)
    pts = det._points_f32(batch['inputs']['points'])
    cs, _ = sparse.voxelize(pts, det.voxel_size)
    levels = det.backbone_3d.prefetch_coords(cs)
    meta = build_fusion_meta([dscan['meta']] * T, det.coord_type, (H, W), V).to(dev)
    win = torch.tensor([[0, t + 1] for t in range(T)], dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream()
    s = st.cuda_stream
    vs = float(det.voxel_size)
    for lvl, (lc, C, Hf) in enumerate(zip(levels, (64, 128, 256, 512), (120, 60, 30, 15))):
        Wf, n, off = Hf, lc.n, lc.offsets()
        ldo = 2 * C                                             # the detector's [3-D | image] rows: the image half is written
        g = torch.Generator().manual_seed(lvl)
        feats = torch.randn(V * Hf * Wf, C, generator=g).to(dev)
        coords = lc.coords
        zc = coords[:n].clone()
        zc[:, 0] = 0
        out, out2 = torch.zeros(n, ldo, device=dev), torch.zeros(n, ldo, device=dev)
        pix, cnt = torch.empty(n, V, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        pix_t = [torch.empty(max(off[t + 1] - off[t], 1), t + 1, dtype=torch.int32, device=dev) for t in range(T)]
        cnt2 = torch.empty(n, dtype=torch.int32, device=dev)

        def fwd_win():
            call('es_point_sample_win_fwd', P(coords), n, vs, P(meta), meta.shape[1], V, P(win), P(feats), Hf, Wf, C, out.data_ptr() + 4 * C, ldo,
                 P(pix), P(cnt), s)

        def fwd_comp():
            for t in range(T):
                r0, nt = off[t], off[t + 1] - off[t]
                call('es_point_sample_fwd', zc.data_ptr() + 16 * r0, nt, vs, meta.data_ptr() + 4 * t * meta.shape[1], meta.shape[1], t + 1, P(feats),
                     Hf, Wf, C, out2.data_ptr() + 4 * (r0 * ldo + C), ldo, P(pix_t[t]), cnt2.data_ptr() + 4 * r0, s)
        fwd_win()
        fwd_comp()
        torch.cuda.synchronize()
        assert torch.equal(out, out2) and torch.equal(cnt, cnt2), 'the window forward is not bit-equal to the composition'
        dout = torch.randn(n, ldo, generator=g).to(dev)
        df, df2 = torch.empty(V * Hf * Wf, C, device=dev), torch.zeros(V * Hf * Wf, C, device=dev)
        head, nxt = torch.empty(V * Hf * Wf, dtype=torch.int32, device=dev), torch.empty(n * V, dtype=torch.int32, device=dev)

        def bwd_win():
            call('es_point_sample_win_bwd', P(coords), n, V, P(win), dout.data_ptr() + 4 * C, ldo, P(pix), P(cnt), Hf, Wf, C, P(df), V, P(head),
                 P(nxt), 0, s)

        def bwd_comp():
            df2.zero_()
            for t in range(T):
                r0, nt = off[t], off[t + 1] - off[t]
                call('es_point_sample_bwd', zc.data_ptr() + 16 * r0, nt, t + 1, dout.data_ptr() + 4 * (r0 * ldo + C), ldo, P(pix_t[t]),
                     cnt2.data_ptr() + 4 * r0, Hf, Wf, C, P(df2), t + 1, P(head), P(nxt), 1, s)
        res = {}
        for name, a, b in (('forward', fwd_win, fwd_comp), ('backward', bwd_win, bwd_comp)):
            for _ in range(warmup):
                a()
                b()
            torch.cuda.synchronize()
            ta, tb = [], []
            for _ in range(reps):                       # alternate inside every repetition
                ta.append(_timed(a, st))
                tb.append(_timed(b, st))
            res[name] = (ta, tb)
        torch.cuda.synchronize()
        rel = float((df.double() - df2.double()).norm() / df2.double().norm())
        for name, (ta, tb) in res.items():
            emit(dict(bench='window_fusion', direction=name, level=lvl, T=T, rows=n, rows_per_prefix=[off[t + 1] - off[t] for t in range(T)], C=C, Hf=Hf,
                      Wf=Wf, reps=reps, window=_stats(ta), composition=_stats(tb),
                      speedup_median=round(_stats(tb)['median_ms'] / _stats(ta)['median_ms'], 3), valid_rows=round(float((cnt > 0).float().mean()), 3),
                      bwd_rel_l2_vs_composition=rel))


def train_step(det, opt, dscan, T, steps, warmup):
    from embodiedscan_amd import engine as E, pipeline
    E.PRECISION[0] = 'bf16'
    st = torch.cuda.current_stream()
    ts = []
    torch.cuda.reset_peak_memory_stats()
    try:
        for i in range(warmup + steps):
            t = _timed(lambda: det.train_step(pipeline.make_cont_det_batch(dscan), opt), st)
            if i >= warmup:
                ts.append(t)
        torch.cuda.synchronize()
    finally:
        E.PRECISION[0] = 'f32'
    emit(dict(bench='cont_det_train_step', T=T, precision='bf16', steps=steps, warmup=warmup, step=_stats(ts),
              peak_memory_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=None, help='also write the JSON lines to this file')
    a = ap.parse_args()
    assert a.reps >= 20, 'at least 20 repetitions'
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_cont_det.py needs the GPU: there is no CPU path')
    from embodiedscan_amd import pipeline as _pl
    from embodiedscan_amd.config import build_detector, build_optim_wrapper, load_config
    dev = torch.device('cuda:0')
    T = 10
    cfg = load_config(os.path.join(ROOT, 'configs', 'cont_det3d.py'))
    det = build_detector(cfg, device=dev, seed=0).to(dev)
    dscan = _pl.upload_scan(sweep_scan(T), dev)
    kernels(det, dscan, T, a.reps, a.warmup, dev)
    if not a.no_step:
        train_step(det, build_optim_wrapper(cfg), dscan, T, a.steps, 2)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')
