"""Time the prefix-fusion kernels against the V-call composition of the kernels they replace, and one continuous train step.

    python tools/bench_prefix_fusion.py [--reps 30] [--warmup 5] [--no-step]

Shipped shape of the continuous occupancy detector: 40 x 40 x 16 prior voxels, C = 256, 120 x 120 feature maps, V = 10 and 20.
  forward   es_point_sample_prefix_fwd_pts (one launch, V view gathers per voxel)
            vs es_point_sample_fwd_pts called with 1 .. V views (V launches, V (V + 1) / 2 gathers); both write V n C floats
  backward  es_point_sample_prefix_bwd (one link + one gather) vs es_point_sample_bwd called V times with accumulate = 1
Both sides run in this process, alternate inside every repetition, are warmed up first and are timed with device events around the
whole call sequence; the median and the minimum over the repetitions are printed as one JSON line per (V, direction).
Then one EmbodiedOccPredictor train step at the shipped widths with T = 10 (synthetic scan, bf16): milliseconds (median of the timed
steps) and peak device memory."""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _meta(V, H, W, seed):
    """one meta block whose V cameras stand 4 m from the room centre and look at it"""
    from embodiedscan_amd import hip
    c = hip.CONSTS
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(1, c['ES_FUSE_PROJ'] + 16 * V)
    m[0, c['ES_FUSE_SFX']] = m[0, c['ES_FUSE_SFY']] = m[0, c['ES_FUSE_ISCALE']] = 1.0
    m[0, c['ES_FUSE_PADW']] = m[0, c['ES_FUSE_ORIW']] = float(W)
    m[0, c['ES_FUSE_PADH']] = float(H)
    K = torch.tensor([[0.6 * W, 0, W / 2, 0], [0, 0.6 * W, H / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float64)
    for v in range(V):
        a = float(torch.rand(1, generator=g)) * 2 * math.pi
        d = torch.tensor([math.cos(a), math.sin(a), -0.2], dtype=torch.float64)
        d = d / d.norm()
        rx = torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64), d)
        rx = rx / rx.norm()
        R = torch.stack([rx, torch.linalg.cross(d, rx), d])
        E = torch.eye(4, dtype=torch.float64)
        E[:3, :3], E[:3, 3] = R, -R @ (-4.0 * d)
        m[0, c['ES_FUSE_PROJ'] + 16 * v:c['ES_FUSE_PROJ'] + 16 * v + 16] = (K @ E).reshape(-1).float()
    return m


def _timed(fn, st):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    fn()
    e1.record(st)
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(ts):
    ts = sorted(ts)
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4))


def kernels(V, reps, warmup, dev):
    from embodiedscan_amd import hip
    from embodiedscan_amd.hip import P, call
    X, Y, Z, C, Hf, Wf, ldo = 40, 40, 16, 256, 120, 120, 256 + 512
    n = X * Y * Z
    g = torch.Generator().manual_seed(V)
    xs = [torch.linspace(-3.2, 3.2, k + 1)[:-1] + 3.2 / k for k in (X, Y)] + [torch.linspace(-1.28, 1.28, Z + 1)[:-1] + 1.28 / Z]
    prior = torch.stack(torch.meshgrid(*xs, indexing='ij'), -1).reshape(-1, 3).contiguous().to(dev)
    meta = _meta(V, 480, 480, V).to(dev)
    feats = torch.randn(V, Hf * Wf, C, generator=g).to(dev)
    coords = torch.zeros(n, 4, dtype=torch.int32, device=dev)
    out = torch.zeros(V * n, ldo, device=dev)
    out2 = torch.zeros(V * n, ldo, device=dev)
    pix = torch.empty(n, V, dtype=torch.int32, device=dev)
    cnt = torch.empty(V, n, dtype=torch.int32, device=dev)
    pix_t = [torch.empty(n, t + 1, dtype=torch.int32, device=dev) for t in range(V)]
    cnt_t = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(V)]
    st = torch.cuda.current_stream()
    s = st.cuda_stream

    def fwd_prefix():
        call('es_point_sample_prefix_fwd_pts', P(coords), P(prior), n, P(meta), meta.shape[1], V, P(feats), Hf, Wf, C, P(out), ldo, P(pix),
             P(cnt), s)

    def fwd_comp():
        for t in range(V):      # (views 0 .. t are the first t + 1 images of `feats`: no copy needed with one sample)
            call('es_point_sample_fwd_pts', P(coords), P(prior), n, P(meta), meta.shape[1], t + 1, P(feats), Hf, Wf, C,
                 out2.data_ptr() + 4 * t * n * ldo, ldo, P(pix_t[t]), P(cnt_t[t]), s)
    fwd_prefix()
    fwd_comp()
    torch.cuda.synchronize()
    assert torch.equal(out, out2), 'the prefix forward is not bit-equal to the composition'
    dout = torch.randn(V * n, ldo, generator=g).to(dev)
    df, df2 = torch.empty(V * Hf * Wf, C, device=dev), torch.zeros(V * Hf * Wf, C, device=dev)
    head, nxt = torch.empty(V * Hf * Wf, dtype=torch.int32, device=dev), torch.empty(n * V, dtype=torch.int32, device=dev)

    def bwd_prefix():
        call('es_point_sample_prefix_bwd', P(coords), n, V, P(dout), ldo, P(pix), P(cnt), Hf, Wf, C, P(df), V, P(head), P(nxt), 0, s)

    def bwd_comp():
        df2.zero_()
        for t in range(V):
            call('es_point_sample_bwd', P(coords), n, t + 1, dout.data_ptr() + 4 * t * n * ldo, ldo, P(pix_t[t]), P(cnt_t[t]), Hf, Wf, C,
                 P(df2), t + 1, P(head), P(nxt), 1, s)
    res = {}
    for name, a, b in (('forward', fwd_prefix, fwd_comp), ('backward', bwd_prefix, bwd_comp)):
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
    hits = int((pix >= 0).sum())
    for name, (ta, tb) in res.items():
        print(json.dumps(dict(bench='prefix_fusion', direction=name, V=V, n=n, C=C, Hf=Hf, Wf=Wf, reps=reps, prefix=_stats(ta),
                              composition=_stats(tb), speedup_median=round(_stats(tb)['median_ms'] / _stats(ta)['median_ms'], 3),
                              hits_per_voxel=round(hits / n, 2), valid_last_prefix=round(float((cnt[V - 1] > 0).float().mean()), 3),
                              bwd_rel_l2_vs_composition=rel)), flush=True)


def train_step(T, steps, warmup, dev):
    from embodiedscan_amd import engine as E, pipeline
    from embodiedscan_amd.config import build_detector, build_optim_wrapper, load_config
    from embodiedscan_amd.synth import make_occ_gt, make_scan
    import numpy as np
    cfg = load_config(os.path.join(ROOT, 'configs', 'cont_occ.py'))
    det = build_detector(cfg, device=dev, seed=0).to(dev)
    opt = build_optim_wrapper(cfg)
    scan = make_scan(5, n_views=T, height=480, width=640, img_size=(480, 480), n_points=T * 10000, n_boxes=20, augment=False)
    order = np.argsort(scan['sel_view'], kind='stable')
    scan['sel_view'], scan['sel_pix'] = scan['sel_view'][order], scan['sel_pix'][order]
    scan['points_slice_indices'] = [0] + np.cumsum(np.bincount(scan['sel_view'], minlength=T)).tolist()
    occ = make_occ_gt(scan, n_voxels=cfg['model']['n_voxels'], prior_range=cfg['prior_generator']['ranges'][0], seed=5)
    occ['gt_occupancy_masks'] = [occ['gt_occupancy_masks']] * T
    dscan = pipeline.upload_scan(scan, dev)
    E.PRECISION[0] = 'bf16'
    st = torch.cuda.current_stream()
    ts, loss = [], None
    torch.cuda.reset_peak_memory_stats()
    for i in range(warmup + steps):
        t = _timed(lambda: det.train_step(pipeline.make_cont_occ_batch(dscan, occ), opt), st)
        if i >= warmup:
            ts.append(t)
    torch.cuda.synchronize()
    print(json.dumps(dict(bench='cont_occ_train_step', T=T, precision='bf16', steps=steps, warmup=warmup, step=_stats(ts),
                          peak_memory_gib=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--no-step', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    for V in (10, 20):
        kernels(V, a.reps, a.warmup, dev)
    if not a.no_step:
        train_step(10, a.steps, 2, dev)
