"""A8 / A13-A15 kernels against the golden vectors made by the reference's own code and against the oracle."""
import os
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _meta_from(d):
    meta = dict(img_shape=tuple(int(v) for v in d['img_shape']), scale_factor=tuple(float(v) for v in d['scale_factor']),
                img_crop_offset=tuple(float(v) for v in d['crop_offset']), flip=bool(d['flip']))
    flow = [str(x) for x in d['flow']]
    if flow:
        meta.update(pcd_rotation=d['pcd_rotation'], pcd_scale_factor=float(d['pcd_scale_factor']), pcd_trans=d['pcd_trans'],
                    pcd_horizontal_flip=bool(d['hflip']), pcd_vertical_flip=bool(d['vflip']), transformation_3d_flow=flow)
    return meta


def point_sample_golden(dev, golden_dir):
    """The golden points are arbitrary floats, the kernel takes integer voxel coordinates * voxel_size, so the check
    runs on the quantised points through BOTH the kernel and the oracle (itself pinned to the golden file).  pix and cnt pass
    fusion_geom_spec.check_geometry; every row without an undecided (point, view) pair matches the oracle within the sum bound
    (k + 1) u sum |f| / cnt of the kernel plus the same for the oracle's own f32 sum: NO row may differ; rows with an undecided pair are
    at most 1 / 100 of the rows (measured: 0 and 1 of 400).  es_point_sample_fwd on the f32 maps and es_point_sample_fwd_h on the maps
    rounded to bf16 (on both sides)."""
    import fusion_geom_spec as G
    import window_spec as WS
    from embodiedscan_amd.hip import P, call
    from embodiedscan_amd.models.layers.fusion_layers.point_fusion import build_fusion_meta
    from oracle import model as OM
    for name in ('point_sample_plain', 'point_sample_aug'):
        d = np.load(os.path.join(golden_dir, name + '.npz'))
        meta = _meta_from(d)
        V = d['proj'].shape[0]
        # express the projection as intrinsic @ extrinsic with identity intrinsics
        meta['depth2img'] = dict(intrinsic=[np.eye(4, dtype=np.float32)] * V, extrinsic=[d['proj'][v] for v in range(V)])
        vs = 0.01
        ci = np.round(d['points'] / vs).astype(np.int32)
        n = len(ci)
        coords = torch.from_numpy(np.concatenate([np.zeros((n, 1), np.int32), ci], 1))
        pts_q = torch.from_numpy(ci).float() * vs
        md = build_fusion_meta([meta], 'DEPTH', tuple(int(v) for v in d['pad_shape']), V)
        for half in (False, True):
            feats = torch.from_numpy(d['feats'])                   # (V,C,H,W)
            if half:
                feats = feats.to(torch.bfloat16).float()
            ref = OM.batch_point_sample(meta, feats, pts_q, torch.from_numpy(d['proj']), torch.from_numpy(d['scale_factor']),
                                        torch.from_numpy(d['crop_offset']), bool(d['flip']), tuple(d['pad_shape']),
                                        tuple(d['img_shape']))
            Vn, C, H, W = feats.shape
            nhwc = feats.permute(0, 2, 3, 1).contiguous().reshape(Vn * H * W, C).to(dev)
            if half:
                nhwc = nhwc.to(torch.bfloat16)
            mdd, cd = md.to(dev), coords.to(dev)
            out = torch.zeros((n, C), device=dev)
            pix = torch.empty((n, V), dtype=torch.int32, device=dev)
            cnt = torch.empty(n, dtype=torch.int32, device=dev)
            call('es_point_sample_fwd_h' if half else 'es_point_sample_fwd', P(cd), n, vs, P(mdd), mdd.shape[1], V, P(nhwc), H, W,
                 C, P(out), C, P(pix), P(cnt), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            rec = dict(V=V, C=C, n=n, Hf=H, Wf=W, coords=cd, meta=md, feats=nhwc.reshape(1, V, H * W, C), out=out, pix=pix, cnt=cnt,
                       win=G.full_windows(1, V), seed=name)
            geo = G.geometry(rec, dev, vs)
            r = G.check_geometry(rec, dev, vs, caps=False, geo=geo, label=f'{name} half={half}')
            WS.check_win_fwd(rec, dev, WS.Stats(name))
            _, bnd, und = G.spec_out(geo, rec['feats'].float(), cd[:, 0], dev)
            diff = (out.double().cpu() - ref.double()).abs()
            bad = int(((diff > 2 * bnd.cpu()).any(1) & ~und.cpu()).sum())
            print(f'{name} half={half}: decided rows differing from the oracle beyond the sum bounds: {bad}/{n} (allowed: 0); rows with an '
                  f'undecided pair: {r["und_rows"]}/{n} (allowed: 1/100)')
            assert bad == 0
            assert 100 * r['und_rows'] <= n
            assert (ref != 0).any(1).sum() > 20


def test_point_sample_vs_reference_golden(golden_dir):
    point_sample_golden(torch.device('cuda:0'), golden_dir)


def test_losses_vs_oracle(golden_dir):
    from embodiedscan_amd.hip import P, call, farr, iarr, parr
    from oracle import geometry as G
    dev = torch.device('cuda:0')
    d = np.load(os.path.join(golden_dir, 'box_coder_cdloss.npz'))
    n = d['pred'].shape[0]
    g = torch.Generator().manual_seed(3)
    pts, pred, tgt = torch.from_numpy(d['points']), torch.from_numpy(d['pred']), torch.from_numpy(d['target'])
    cls_t = torch.where(torch.rand(n, generator=g) < 0.7, torch.randint(0, 284, (n,), generator=g), torch.tensor(-1)).int()
    center_p, center_t = torch.randn(n, generator=g), torch.rand(n, generator=g)
    npos = int((cls_t >= 0).sum())
    avg = torch.tensor([float(max(npos, 1))])
    w = [0.2, 0.2, 0.2, 0.4]
    # oracle value + autograd gradient
    po = pred.clone().requires_grad_(True)
    co = center_p.clone().requires_grad_(True)
    pos = torch.nonzero(cls_t >= 0).squeeze(1)
    dec = G.bbox_pred_to_bbox(pts[pos], po[pos])
    tb = tgt[pos]
    lb = w[0] * G.bbox_cd_loss(torch.cat((dec[:, :3], tb[:, 3:]), -1), tb) + \
        w[1] * G.bbox_cd_loss(torch.cat((tb[:, :3], dec[:, 3:6], tb[:, 6:]), -1), tb) + \
        w[2] * G.bbox_cd_loss(torch.cat((tb[:, :6], dec[:, 6:]), -1), tb) + w[3] * G.bbox_cd_loss(dec, tb)
    lc = torch.nn.functional.binary_cross_entropy_with_logits(co[pos], center_t[pos], reduction='sum') / (avg[0] + 1.1920929e-07)
    (lb + lc).backward()
    dcen = torch.zeros(n, device=dev)
    dbb = torch.zeros((n, 12), device=dev)
    acc = torch.zeros(2, dtype=torch.float64, device=dev)          # f64 loss sums
    # keep every device tensor alive in a variable: P() only takes the pointer
    d_cls, d_np, d_pts, d_cp = cls_t.to(dev), torch.tensor([npos], dtype=torch.int32, device=dev), pts.to(dev), center_p.to(dev)
    d_pred, d_ct, d_tgt, d_avg = pred.to(dev), center_t.to(dev), tgt.to(dev), avg.to(dev)
    # two "levels" (rows 0..39 and 40..n) to exercise the level table
    n0 = 40
    d_ws = torch.empty(n + 1, dtype=torch.int32, device=dev)     # compacted positives (bound: every row)
    call('es_pos_losses', P(d_cls), n, P(d_np), n, P(d_ws), P(d_pts), 2, iarr([0, n0, n]), parr([d_cp.data_ptr(), d_cp.data_ptr() + 4 * n0]),
         parr([d_pred.data_ptr(), d_pred.data_ptr() + 48 * n0]), parr([dcen.data_ptr(), dcen.data_ptr() + 4 * n0]),
         parr([dbb.data_ptr(), dbb.data_ptr() + 48 * n0]), 1, P(d_ct), P(d_tgt), P(d_avg), 1.0, farr(w), P(acc),
         torch.cuda.current_stream().cuda_stream)
    acc = acc.cpu()
    lb, lc = lb.detach(), lc.detach()
    print(f'bbox loss hip {float(acc[1]):.6f} oracle {float(lb):.6f}; center sum hip {float(acc[0]):.6f}')
    assert abs(float(acc[1]) - float(lb)) / float(lb) < 1e-5
    assert abs(float(acc[0]) / (float(avg[0]) + 1.1920929e-07) - float(lc)) / float(lc) < 1e-5
    e1 = float((dbb.cpu() - po.grad).abs().max() / po.grad.abs().max())
    e2 = float((dcen.cpu() - co.grad).abs().max() / co.grad.abs().max())
    print(f'dual-number box-loss gradient rel err {e1:.2e}, centerness gradient rel err {e2:.2e} (tol 1e-4)')
    assert e1 < 1e-4 and e2 < 1e-4
    # focal
    N, C = 3000, 284
    logits = torch.randn(N, C, generator=g) * 2 - 2
    labels = torch.where(torch.rand(N, generator=g) < 0.1, torch.randint(0, C, (N,), generator=g), torch.tensor(-1))
    lo = logits.clone().requires_grad_(True)
    fl = G.sigmoid_focal_loss_sum(lo, labels) / (avg[0] + 1.1920929e-07)
    fl.backward()
    grad = torch.zeros((N, C), device=dev)
    partial = torch.empty(2048, dtype=torch.float64, device=dev)
    out = torch.zeros(1, device=dev)
    d_log, d_lab = logits.to(dev), labels.int().to(dev)
    call('es_focal_loss', P(d_log), C, P(d_lab), N, C, 2.0, 0.25, P(d_avg), 1.0, P(grad), C,
         P(partial), P(out), torch.cuda.current_stream().cuda_stream)
    e = abs(float(out.cpu()) - float(fl)) / float(fl)
    eg = float((grad.cpu() - lo.grad).abs().max() / lo.grad.abs().max())
    print(f'focal loss rel err {e:.2e} grad rel err {eg:.2e} (tol 1e-5 / 1e-4)')
    assert e < 1e-5 and eg < 1e-4


def test_optimizer_step():
    from embodiedscan_amd.hip import P, call
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(0)
    n = 100003
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3
    pt = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([pt], lr=1e-3, weight_decay=1e-4)
    pd, gd = p.to(dev), gr.to(dev)
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    partial, norm = torch.empty(2048, dtype=torch.float64, device=dev), torch.zeros(1, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    for step in range(1, 4):
        pt.grad = gr.clone()
        torch.nn.utils.clip_grad_norm_([pt], 10.0)
        opt.step()
        call('es_grad_norm', P(gd), n, P(partial), P(norm), s)
        call('es_adamw_step', P(pd), P(gd), P(m), P(v), n, 1e-3, 0.9, 0.999, 1e-8, 1e-4, step, 10.0, P(norm), 1.0, s)
    assert abs(float(norm.cpu()) - float(gr.norm())) / float(gr.norm()) < 1e-6
    err = float((pd.cpu() - pt.detach()).abs().max())
    print(f'AdamW 3 steps max abs err {err:.2e} (tol 1e-6)')
    assert err < 1e-6


def point_sample_bwd_ordered_gather(dev):
    """es_point_sample_bwd (round 3: linked hit lists + one wave per feature-map pixel adding its hits in ascending voxel
    order) against the f64 adjoint, element by element, under the bound of window_spec.check_win_bwd (full windows, one image set
    per sample): a pixel with more than 256 linked hits, pixels with exactly 1, 63, 64, 65, 128 and 129 linked hits (the edges of the 64-at-a-time
    extraction), voxels WITHOUT a valid view whose pix entries are >= 0 all the same (the forward samples unmasked, SURVEY Q3: they
    must not contribute), empty pixels written as zeros, a sample that owns no row, C in {96, 1, 65, 512}, strided dout rows,
    accumulate on / off; two runs bit-identical."""
    import window_spec as WS
    from embodiedscan_amd.hip import P, call
    g = torch.Generator().manual_seed(3)
    B, V, Hf, Wf, n = 3, 3, 6, 5, 4000
    HW = Hf * Wf
    EDGES = (1, 63, 64, 65, 128, 129)
    coords = torch.zeros((n, 4), dtype=torch.int32)
    coords[:, 0] = 2 * (torch.arange(n) >= n // 2).int()     # samples 0 and 2: sample 1 owns no row
    pix = torch.randint(-1, HW, (n, V), generator=g, dtype=torch.int32)
    pix[:600, 0] = 7                                         # 600 hits on one pixel of (sample 0, view 0)
    pix[torch.rand(n, V, generator=g) < 0.3] = -1
    dead = torch.rand(n, generator=g) < 0.1                  # sampled somewhere, but no VALID view
    pix[n // 2:, 2] = -1                                     # (sample 2, view 2): pixel j gets exactly EDGES[j] linked hits
    rows = torch.nonzero(~dead[n // 2:]).squeeze(1) + n // 2
    r0 = 0
    for j, h in enumerate(EDGES):
        pix[rows[r0:r0 + h], 2] = j
        r0 += h
    cnt = (pix >= 0).sum(1).int()
    cnt[dead] = 0
    st = torch.cuda.current_stream().cuda_stream
    stats = WS.Stats('es_point_sample_bwd')
    d = dict(coords=coords.to(dev), pix=pix.to(dev), cnt=cnt.to(dev))
    head = torch.empty(B * V * HW, dtype=torch.int32, device=dev)
    nxt = torch.empty(n * V, dtype=torch.int32, device=dev)
    for C in (96, 1, 65, 512):
        dout = torch.randn(n, C + 8, generator=g).to(dev)    # strided rows (columns 8.. are the image part)
        rec = dict(V=V, C=C, n=n, Hf=Hf, Wf=Wf, B=B, n_sets=B, coords=d['coords'], win=torch.tensor([[b, V] for b in range(B)], dtype=torch.int32),
                   pix=d['pix'], cnt=d['cnt'], dout=dout[:, 8:])
        outs = []
        for _ in range(2):
            f = torch.full((B * V * HW, C), float('nan'), device=dev)        # accumulate = 0 must overwrite everything
            call('es_point_sample_bwd', P(d['coords']), n, V, dout.data_ptr() + 32, C + 8, P(d['pix']), P(d['cnt']), Hf, Wf, C,
                 P(f), B * V, P(head), P(nxt), 0, st)
            torch.cuda.synchronize()
            outs.append(f.clone())
        assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
        brec = dict(rec, acc=0, dfeats=outs[0])
        WS.check_win_bwd(brec, dev, stats)
        H = WS.win_bwd_bound(brec, dev)[3]
        p0 = (2 * V + 2) * HW
        assert H[p0:p0 + len(EDGES)].tolist() == list(EDGES) and int(H.max()) > 256, 'the hit counts the test is about'
        assert not bool(H[V * HW:2 * V * HW].any()) and bool((outs[0][V * HW:2 * V * HW] == 0).all()), 'the sample without rows: zeros'
        base = torch.randn(B * V * HW, C, generator=g)
        f = base.clone().to(dev)
        call('es_point_sample_bwd', P(d['coords']), n, V, dout.data_ptr() + 32, C + 8, P(d['pix']), P(d['cnt']), Hf, Wf, C,
             P(f), B * V, P(head), P(nxt), 1, st)
        torch.cuda.synchronize()
        WS.check_win_bwd(dict(rec, acc=1, dfeats=f, dfeats0=base), dev, stats)
    print(stats.report())
    print(f'point_sample_bwd vs the f64 adjoint per element; busiest pixel {int((pix[:, 0] == 7).sum())} hits')


def test_point_sample_bwd_is_an_ordered_gather():
    point_sample_bwd_ordered_gather(torch.device('cuda:0'))
