"""The head loss, target and prediction kernels (csrc/losses.hip, csrc/targets.hip, csrc/predict.hip, csrc/occ.hip) held to the f64
specifications of tests/head_spec.py at every shape edge: the focal loss over N / C / leading-dimension edges, both gamma branches and
saturated logits; the regression decode at the clamp and past its grid stride; the corner-Chamfer losses over level tables, wave
boundaries, a max_pos below the number of positives and ill-conditioned rotations; target assignment through the TG_CAP re-scan, ties at
the k-th centerness and empty levels; scores, box decode and NMS up to NMS_CAP; the occupancy supervision and the three occupancy losses
over C / n edges and the distributions at which a precision or a recall goes to zero.  Every output buffer is wider or longer than
the kernel should write and pre-filled with a sentinel that must survive; accumulating outputs start from a non-zero prior.

Every body is a function of `dev`: tests/test_emu_head_kernels.py runs the same bodies on the CPU emulator (dev.type == 'cpu' selects
the reduced grid there).  Each body prints the worst bound ratio per class."""
import math

import numpy as np
import pytest
import torch

import head_spec as S
from test_gpu_ground_kernels import SENT, Cols, _flat, _hip, _rc, _small, _st, _tail_ok

pytestmark = pytest.mark.gpu

ISENT = -77
W4 = [0.2, 0.2, 0.2, 0.4]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ibuf(dev, n, pad=8, fill=ISENT):
    buf = torch.full((n + pad,), fill, dtype=torch.int32, device=dev)
    return buf[:n], buf


# ------------------------------------------------------------------------------------------------------------------ focal
def focal_case(dev, stats, x, labels, gamma, with_grad, gs, avg, alpha=0.25):
    hip = _hip()
    P = hip.P
    N, C = x.shape
    L = Cols(dev, N, C, C + 3, 2, x)
    Gd = Cols(dev, N, C, C + 5, 1)
    lab = labels.to(torch.int32).to(dev)
    avg_d = torch.tensor([avg], dtype=torch.float32, device=dev)
    part = torch.full((2048 + 8,), float(SENT), dtype=torch.float64, device=dev)
    out = torch.tensor([0.375, SENT], dtype=torch.float32, device=dev)
    hip.call('es_focal_loss', L.ptr(), L.ld, P(lab), N, C, gamma, alpha, P(avg_d), gs, Gd.ptr() if with_grad else 0, Gd.ld, P(part), P(out), _st())
    torch.cuda.synchronize()
    label = f'focal N={N} C={C}'
    Gd.untouched_outside(label)
    L.untouched_outside(label)
    blocks = max(min((N + 3) // 4, 2048), 1)
    assert bool((part[blocks:] == SENT).all()) and float(out[1]) == SENT, f'{label}: partial / loss_out written past their ends'
    if not with_grad:
        assert bool((Gd.buf == SENT).all()), f'{label}: grad = NULL, yet the gradient buffer was written'
    rec = dict(logits=L.v, labels=lab, gamma=gamma, alpha=alpha, avg=float(avg_d[0]), grad_scale=gs, grad=Gd.v if with_grad else None, loss0=0.375,
               loss1=float(out[0]))
    S.check_focal_head(rec, dev, stats)
    return rec


def focal_inputs(N, C, seed):
    g = _gen(seed)
    x = torch.rand(N, C, generator=g) * 20 - 10
    labels = torch.randint(0, C, (N,), generator=g)
    edge = torch.tensor([-1, 0, C - 1, C])
    labels[:min(N, 4)] = edge.roll(seed % 4)[:min(N, 4)]
    return x, labels


def test_focal_loss_on_the_shape_grid(dev):
    stats = S.Stats('focal grid')
    strided, i = 0, 0
    for N in (1, 3, 4, 5):
        for C in (1, 63, 64, 65, 284):
            x, labels = focal_inputs(N, C, 100 + i)
            focal_case(dev, stats, x, labels, (2.0, 1.5)[i % 2], i % 5 != 4, 0.5, 3.7)
            i += 1
    N = 8197
    strided += (N + 3) // 4 > 2048
    x, labels = focal_inputs(N, 3, 7)
    focal_case(dev, stats, x, labels, 2.0, True, 0.5, 811.0)
    focal_case(dev, stats, x, labels, 1.5, False, 0.5, 811.0)
    assert strided == 1, 'the grid-stride case did not occur'
    print(stats.report())


def test_focal_loss_on_saturated_logits(dev):
    """x in {+-17, +-30, +-100} on a label column and on a background column, both gamma branches"""
    stats = S.Stats('focal saturated')
    vals = torch.tensor([17.0, -17.0, 30.0, -30.0, 100.0, -100.0])
    x = vals[:, None].repeat(2, 2)
    labels = torch.tensor([0] * 6 + [-1] * 6)
    for gamma in (2.0, 1.5):
        focal_case(dev, stats, x, labels, gamma, True, 0.5, 2.0)
    print(stats.report())


# ------------------------------------------------------------------------------------------------------------------ regression decode
def _clamp_rows(scale):
    """f32 arguments whose product with `scale` sits 2 ulps below / exactly at / 2 ulps above the f32 nearest log(1e-3)"""
    t0 = np.float32(math.log(S.LO3))
    lo = np.nextafter(np.nextafter(t0, np.float32(-100)), np.float32(-100))
    hi = np.nextafter(np.nextafter(t0, np.float32(100)), np.float32(100))
    return [float(np.float32(v) / np.float32(scale)) for v in (lo, t0, hi)]


def reg_decode_case(dev, stats, n, scale, seed):
    hip = _hip()
    P = hip.P
    g = _gen(seed)
    reg = torch.randn(n, 12, generator=g) * 2
    reg[:, :6] -= 2                                             # a good share below the floor
    rows = _clamp_rows(scale)
    for k in range(min(n, 3)):
        reg[k, :6] = rows[k]
    R = Cols(dev, n, 12, 14, 1, reg)
    sc = torch.tensor([scale], dtype=torch.float32, device=dev)
    bbox, bbox_buf = _flat(dev, torch.zeros(n, 12))
    bbox_buf.fill_(SENT)
    hip.call('es_reg_decode_fwd', R.ptr(), R.ld, n, P(sc), P(bbox), _st())
    torch.cuda.synchronize()
    label = f'reg_decode n={n} scale={scale}'
    _tail_ok(bbox_buf, n * 12, label)
    S.check_reg_decode_fwd(label, R.v, sc, bbox, stats)
    dbbox = torch.randn(n, 12, generator=g).to(dev)
    runs = []
    for _ in range(2):
        D = Cols(dev, n, 12, 14, 2)
        ds = torch.tensor([0.75, SENT], dtype=torch.float32, device=dev)
        part = torch.full((512 + 8,), SENT, dtype=torch.float32, device=dev)
        hip.call('es_reg_decode_bwd', R.ptr(), R.ld, P(bbox), P(dbbox), n, P(sc), D.ptr(), D.ld, P(ds), P(part), _st())
        torch.cuda.synchronize()
        D.untouched_outside(label)
        blocks = min((n * 12 + 255) // 256, 512)
        assert bool((part[blocks:] == SENT).all()) and float(ds[1]) == SENT, f'{label}: partial / dscale written past their ends'
        runs.append((D.v.clone(), ds[:1].clone()))
    assert S._bits_equal(runs[0][0], runs[1][0]) and S._bits_equal(runs[0][1], runs[1][1]), f'{label}: two launches differ (the reduction order is not fixed)'
    S.check_reg_decode_bwd(label, R.v, bbox, dbbox, sc, runs[0][0], 0.75, float(runs[0][1]), stats)
    return dict(reg=R.v.cpu(), bbox=bbox.cpu(), dbbox=dbbox.cpu(), scale=sc.cpu(), dreg=runs[0][0].cpu(), dscale=float(runs[0][1]))


def test_reg_decode_at_the_clamp_and_past_the_grid_stride(dev):
    stats = S.Stats('reg_decode')
    strided = 0
    for i, n in enumerate((1, 21, 22, 10923, 11000)):
        strided += n * 12 > 512 * 256
        for scale in (0.7, 1.0):
            reg_decode_case(dev, stats, n, scale, 200 + i)
    assert strided == 2
    hip = _hip()
    buf = torch.full((64,), SENT, dtype=torch.float32, device=dev)
    sc = torch.ones(1, device=dev)
    assert _rc('es_reg_decode_fwd', hip.P(buf), 12, 0, hip.P(sc), hip.P(buf), _st()) == 0
    assert _rc('es_reg_decode_bwd', hip.P(buf), 12, hip.P(buf), hip.P(buf), 0, hip.P(sc), hip.P(buf), 12, hip.P(buf), hip.P(buf), _st()) == 0
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()), 'n = 0 wrote something'
    print(stats.report())


# ------------------------------------------------------------------------------------------------------------------ corner Chamfer
def edge_rows():
    """(bbox (5, 12), target (5, 9), point (5, 3)): a coincident box with identity rotation, a cube target whose corners tie, |y_raw| = 1e-3,
    y_raw within 1e-2 of +z, x_raw within 1e-4 relative of y_raw"""
    b = torch.zeros(5, 12)
    b[:, :6] = torch.tensor([0.5, 0.5, 0.25, 0.75, 1.0, 0.5])
    b[:, 6:9] = torch.tensor([1.0, 0.0, 0.0])
    b[:, 9:12] = torch.tensor([0.0, 1.0, 0.0])
    t = torch.zeros(5, 9)
    t[:, :3] = torch.tensor([0.25, -0.5, 1.0])
    t[:, 3:6] = torch.tensor([1.5, 0.75, 2.0])
    t[:, 6:9] = torch.tensor([0.3, -0.2, 0.5])
    p = torch.tensor([[0.5, 0.25, -1.0]]).repeat(5, 1)
    b[0, :6] = 0.5                                               # size (1, 1, 1) at the point itself, identity rotation
    t[0] = torch.tensor([0.5, 0.25, -1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0])
    b[1, :6] = 0.0                                               # a point-sized prediction at the centre of a cube: all 8 corners tie
    t[1] = torch.tensor([0.5, 0.25, -1.0, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0])
    b[2, 9:12] = torch.tensor([0.0, 1e-3, 0.0])
    b[2, 6:9] = torch.tensor([0.7, 0.1, -0.3])
    b[3, 9:12] = torch.tensor([0.006, -0.005, 1.0])
    b[3, 6:9] = torch.tensor([0.9, 0.2, 0.1])
    b[4, 9:12] = torch.tensor([0.3, 0.8, -0.5])
    b[4, 6:9] = b[4, 9:12] * 1.25 + torch.tensor([1e-4, 0.0, 0.0])
    return b, t, p


def pos_losses_case(dev, stats, sizes, npos, max_pos_kind, ldh, seed, edges=False):
    hip = _hip()
    P = hip.P
    g = _gen(seed)
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    n = off[-1]
    bbox = torch.cat([torch.rand(n, 6, generator=g) + 0.2, torch.randn(n, 6, generator=g)], 1)
    tgt = torch.cat([torch.randn(n, 3, generator=g), torch.rand(n, 3, generator=g) + 0.5, torch.rand(n, 3, generator=g) * 6 - 3], 1)
    pts = tgt[:, :3] + torch.randn(n, 3, generator=g) * 0.3
    cls_t = torch.full((n,), -1, dtype=torch.int32)
    rows = torch.randperm(n, generator=g)[:npos].sort().values
    cls_t[rows] = torch.randint(0, 284, (npos,), generator=g).int()
    ctr = torch.randn(n, generator=g) * 2
    if npos >= 2:
        ctr[rows[0]], ctr[rows[1]] = 60.0, -60.0
    if edges:
        eb, et, ep = edge_rows()
        bbox[rows[2:7]], tgt[rows[2:7]], pts[rows[2:7]] = eb, et, ep
    center_t = torch.rand(n, generator=g)
    max_pos = {'count': npos, 'n': n, 'below': max(npos - 13, 1)}[max_pos_kind]
    HO = Cols(dev, n, 1, ldh, 0, ctr[:, None])
    DHO = Cols(dev, n, 1, ldh, 0)
    bb, bb_buf = _flat(dev, bbox)
    dbb, dbb_buf = _flat(dev, torch.full((n, 12), SENT))
    ws, ws_buf = _ibuf(dev, max(max_pos, 1) + 1)
    d_cls, d_pts, d_ct, d_tgt = cls_t.to(dev), pts.to(dev).contiguous(), center_t.to(dev), tgt.to(dev).contiguous()
    d_np = torch.tensor([npos + 3], dtype=torch.int32, device=dev)
    d_avg = torch.tensor([5.3], dtype=torch.float32, device=dev)
    acc = torch.tensor([1.5, -0.25, SENT], dtype=torch.float64, device=dev)
    acc0 = acc[:2].clone()
    lv = len(sizes)
    args = lambda nl, wsp: (P(d_cls), n, P(d_np), max_pos, wsp, P(d_pts), nl, hip.iarr(off + [n] * (nl - lv)),
                            hip.parr([HO.ptr() + 4 * ldh * off[min(l, lv)] for l in range(nl)]), hip.parr([bb.data_ptr() + 48 * off[min(l, lv)] for l in range(nl)]),
                            hip.parr([DHO.ptr() + 4 * ldh * off[min(l, lv)] for l in range(nl)]), hip.parr([dbb.data_ptr() + 48 * off[min(l, lv)] for l in range(nl)]),
                            ldh, P(d_ct), P(d_tgt), P(d_avg), 0.5, hip.farr(W4), P(acc), _st())
    label = f'es_pos_losses levels={sizes} npos={npos} max_pos={max_pos}'
    if max_pos > 0 and n > 0:
        assert _rc('es_pos_losses', *args(9, P(ws))) == -3 and _rc('es_pos_losses', *args(lv, 0)) == -2
        torch.cuda.synchronize()
        assert bool((dbb_buf == SENT).all()) and bool((DHO.buf == SENT).all()) and bool((ws_buf == ISENT).all()) and torch.equal(acc[:2], acc0), \
            f'{label}: a refused call wrote something'
    hip.call('es_pos_losses', *args(lv, P(ws)))
    torch.cuda.synchronize()
    DHO.untouched_outside(label)
    _tail_ok(dbb_buf, n * 12, label)
    assert float(acc[2]) == SENT and bool((ws_buf[max_pos + 1:] == ISENT).all()), f'{label}: loss_acc / pos_ws written past their ends'
    rec = dict(pts=d_pts, bbox=bb, ctr=HO.v[:, 0], cls_t=d_cls, center_t=d_ct, bbox_t=d_tgt, P=npos + 3, avg=float(d_avg[0]), grad_scale=0.5, w=W4,
               max_pos=max_pos, dctr=DHO.v[:, 0], dbbox=dbb, sent=SENT, acc0=acc0, acc1=acc[:2], count=int(ws[0]))
    S.check_pos_losses(rec, dev, stats)
    return rec


POS_CASES = [([1], 1, 'count', 1, False), ([40, 0, 1], 0, 'n', 297, False), ([40, 0, 1], 1, 'n', 1, False), ([40, 0, 1], 16, 'count', 297, True),
             ([40, 0, 1], 17, 'n', 1, True), ([10, 1, 0, 9, 5, 20, 3, 2], 33, 'count', 297, True), ([10, 1, 0, 9, 5, 20, 3, 2], 33, 'below', 1, True)]


def test_pos_losses_over_levels_wave_edges_and_ill_conditioned_rotations(dev):
    stats = S.Stats('pos_losses')
    for i, (sizes, npos, kind, ldh, edges) in enumerate(POS_CASES):
        rec = pos_losses_case(dev, stats, sizes, npos, kind, ldh, 300 + i, edges)
        if edges:                                               # the coincident row: an all-zero gradient, written
            rows = torch.nonzero(rec['cls_t'] >= 0).squeeze(1)
            if bool((rec['dbbox'][rows[2]] != SENT).all()):
                assert bool((rec['dbbox'][rows[2]] == 0).all()), 'the coincident box has a gradient'
    print(stats.report())


def box_cd_case(dev, stats, B, Q, Gs, seed, n_pairs=None, with_grad=True):
    hip = _hip()
    P = hip.P
    g = _gen(seed)

    def boxes(n):
        return torch.cat([torch.randn(n, 3, generator=g), torch.rand(n, 3, generator=g) + 0.3, torch.rand(n, 3, generator=g) * 6 - 3], 1)
    pred, gt = boxes(B * Q), boxes(max(sum(Gs), 1))
    q2g = torch.full((B, Q), -1, dtype=torch.int32)
    for b in range(B):
        q2g[b, torch.randperm(Q, generator=g)[:Gs[b]]] = torch.arange(Gs[b], dtype=torch.int32)
    if B * Q >= 3 and Gs[0] >= 1:                                # one coincident pair: a zero gradient row
        q = int(torch.nonzero(q2g[0] >= 0)[0])
        pred[q] = gt[int(q2g[0, q])]
    gt_off = [0]
    for v in Gs:
        gt_off.append(gt_off[-1] + v)
    n_pairs = sum(Gs) if n_pairs is None else n_pairs
    d_pred, d_gt, d_q = pred.to(dev), gt.to(dev), q2g.reshape(-1).to(dev)
    d_off = torch.tensor(gt_off, dtype=torch.int32, device=dev)
    dp, dp_buf = _flat(dev, torch.full((B * Q, 9), SENT))
    acc = torch.tensor([1.5, SENT], dtype=torch.float64, device=dev)
    hip.call('es_box_cd_pairs', P(d_pred), P(d_q), B, Q, P(d_gt), P(d_off), n_pairs, 0.5, hip.farr(W4), P(dp) if with_grad else 0, P(acc), _st())
    torch.cuda.synchronize()
    label = f'es_box_cd_pairs B={B} Q={Q}'
    _tail_ok(dp_buf, B * Q * 9, label)
    assert float(acc[1]) == SENT
    if not with_grad:
        assert bool((dp_buf == SENT).all())
    S.check_box_cd_pairs(dict(pred=d_pred, q2g=d_q, B=B, Q=Q, gt=d_gt, gt_off=gt_off, n_pairs=n_pairs, grad_scale=0.5, w=W4, dpred=dp if with_grad else None,
                              sent=SENT, acc0=torch.tensor([1.5], dtype=torch.float64), acc1=acc[:1]), dev, stats)


def test_box_cd_pairs_over_batches_and_unmatched_rows(dev):
    stats = S.Stats('box_cd_pairs')
    for i, (B, Q, Gs) in enumerate(((1, 1, [1]), (2, 16, [5, 0]), (2, 17, [0, 17]), (3, 50, [7, 0, 20]))):
        box_cd_case(dev, stats, B, Q, Gs, 400 + i)
    box_cd_case(dev, stats, 2, 17, [4, 3], 410, n_pairs=0)
    box_cd_case(dev, stats, 2, 17, [4, 3], 411, with_grad=False)
    print(stats.report())


# ------------------------------------------------------------------------------------------------------------------ targets
def targets_call(dev, levels, boxes, labels, assign_thr=27, center_thr=18, n_levels=None):
    """es_get_targets on host inputs; returns (status, center_t, bbox_t, cls_t, box_idx, n_pos, best_level, buffers)"""
    from embodiedscan_amd.geometry import euler_to_matrix_zxy
    hip = _hip()
    P = hip.P
    pts = torch.cat(levels) if levels else torch.zeros(0, 3)
    off = [0]
    for p in levels:
        off.append(off[-1] + p.shape[0])
    N, Gn = pts.shape[0], boxes.shape[0]
    nl = len(levels) if n_levels is None else n_levels
    off = off + [N] * (nl - len(levels))
    rot = euler_to_matrix_zxy(-boxes[:, 6:9]).reshape(Gn, 9) if Gn else torch.zeros(0, 9)
    d_pts, d_box, d_rot, d_lab = (t.contiguous().to(dev) for t in (pts, boxes, rot, labels.to(torch.int32)))
    scratch = torch.empty(max(Gn, 1) * max(N, 1) + (nl + 2) * max(Gn, 1) + 8, dtype=torch.float32, device=dev)
    ct, ct_buf = _flat(dev, torch.full((N,), SENT))
    bt, bt_buf = _flat(dev, torch.full((N, 9), SENT))
    kt, kt_buf = _ibuf(dev, N)
    bi, bi_buf = _ibuf(dev, N)
    npos, np_buf = _ibuf(dev, 1)
    rc = _rc('es_get_targets', P(d_pts), N, hip.iarr(off), nl, P(d_box), P(d_rot), P(d_lab), Gn, assign_thr, center_thr, P(scratch), P(ct), P(bt), P(kt),
             P(bi), P(npos), _st())
    torch.cuda.synchronize()
    best = scratch[Gn * N:].view(torch.int32)[nl * Gn:nl * Gn + Gn].cpu() if (Gn and N and rc == 0) else None
    return rc, ct, bt, kt, bi, npos, best, (ct_buf, bt_buf, kt_buf, bi_buf, np_buf)


def targets_case(dev, label, levels, boxes, labels, **kw):
    rc, ct, bt, kt, bi, npos, best, bufs = targets_call(dev, levels, boxes, labels, **kw)
    assert rc == 0, (label, rc)
    N = sum(p.shape[0] for p in levels)
    _tail_ok(bufs[0], N, label)
    _tail_ok(bufs[1], N * 9, label)
    assert all(bool((b[n:] == ISENT).all()) for b, n in ((bufs[2], N), (bufs[3], N), (bufs[4], 1))), f'{label}: an integer output was written past its end'
    S.check_targets(label, levels, boxes, labels, kw.get('assign_thr', 27), kw.get('center_thr', 18), ct.cpu(), bt.cpu(), kt.cpu(), bi.cpu(), int(npos[0]))
    return kt.cpu(), bi.cpu(), best


def _box(c, s, e=(0, 0, 0)):
    return torch.tensor([list(c) + list(s) + list(e)], dtype=torch.float32)


def test_get_targets_bit_exact_through_every_branch(dev):
    from oracle import geometry as OG
    g = _gen(5)
    # random scenes at the block edges: 3 levels, 5 rotated boxes
    for N in (1, 255, 257, 1025):
        n0 = N - N // 3 - N // 5
        levels = [torch.rand(k, 3, generator=g) * 4 - 2 for k in (n0, N // 3, N // 5)]
        boxes = torch.cat([torch.rand(5, 3, generator=g) * 2 - 1, torch.rand(5, 3, generator=g) * 2 + 0.8, torch.rand(5, 3, generator=g) * 6 - 3], 1)
        targets_case(dev, f'random N={N}', levels, boxes, torch.arange(5) + 3, assign_thr=9, center_thr=4)
    # more than TG_CAP points inside one box at its best level (the next level holds fewer than assign_thr inside points)
    big = _box((0, 0, 0), (4, 4, 4), (0.3, 0.1, -0.2))
    levels = [torch.cat([torch.rand(12000, 3, generator=g) * 2 - 1, torch.rand(300, 3, generator=g) * 2 + 5]), torch.rand(10, 3, generator=g) - 0.5]
    inside = OG.face_distances(torch.cat(levels), big).min(-1).values[:, 0] > 0
    assert int(inside[:12300].sum()) > 8192 and int(inside[12300:].sum()) < 27
    kt, bi, best = targets_case(dev, 'TG_CAP', levels, big, torch.tensor([7]))
    assert int(best[0]) == 0 and int((kt >= 0).sum()) == 18
    # the symmetric lattice: ties at the 19th centerness
    ax = torch.tensor([-0.75, -0.5, -0.25, 0.25, 0.5, 0.75])
    lat = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)
    cube = _box((0, 0, 0), (2, 2, 2))
    cen = OG.centerness_from_faces(OG.face_distances(lat, cube))[:, 0].sort(descending=True).values
    assert float(cen[18]) == float(cen[17]) == float(cen[19]), 'no tie at the 19th centerness'
    kt, _, _ = targets_case(dev, 'lattice', [lat], cube, torch.tensor([2]))
    assert int((kt >= 0).sum()) == 8                             # the 8 innermost points are strictly above the tied threshold
    # a box with fewer than 19 inside points, one containing nothing, one whose every level passes the threshold, an empty level
    pts0 = torch.rand(600, 3, generator=g) * 2 - 1
    few = torch.rand(7, 3, generator=g) * 0.2 + 3
    levels = [torch.cat([pts0, few]), torch.zeros(0, 3), torch.rand(400, 3, generator=g) * 2 - 1]
    boxes = torch.cat([_box((3.1, 3.1, 3.1), (0.4, 0.4, 0.4)), _box((-9, 0, 0), (1, 1, 1)), _box((0, 0, 0), (1.6, 1.7, 1.8), (0.4, 0, 0))])
    kt, bi, best = targets_case(dev, 'few / none / every level', levels, boxes, torch.tensor([4, 5, 6]), assign_thr=5)
    assert best.tolist()[1] == 0 and int((bi == 0).sum()) == 7 and int((bi == 1).sum()) == 0
    levels2 = [pts0, torch.rand(400, 3, generator=g) * 2 - 1]
    _, _, best = targets_case(dev, 'every level passes', levels2, boxes[2:], torch.tensor([6]), assign_thr=5)
    assert best.tolist() == [1]
    # nested boxes of equal volume: the first wins
    nested = torch.cat([_box((0, 0, 0), (2, 1, 1)), _box((0, 0, 0), (1, 2, 1))])
    pin = torch.cat([pts0[:15] * 0.4, pts0[15:25] + 5])          # fewer than 19 inside points, inside both: every one passes, the volumes tie
    kt, bi, _ = targets_case(dev, 'equal volumes', [pin], nested, torch.tensor([1, 2]), assign_thr=5)
    assert bool((OG.face_distances(pin[:15], nested).min(-1).values > 0).all()) and bool((bi[:15] == 0).all())
    # 8 levels accepted, 9 refused; G = 0; N = 0
    lv8 = [torch.rand(30, 3, generator=g) * 2 - 1 for _ in range(8)]
    targets_case(dev, '8 levels', lv8, boxes[2:], torch.tensor([6]), assign_thr=3, center_thr=4)
    rc, ct, bt, kt, bi, npos, _, bufs = targets_call(dev, lv8, boxes[2:], torch.tensor([6]), n_levels=9)
    assert rc == -3 and all(bool((b == (SENT if b.dtype == torch.float32 else ISENT)).all()) for b in bufs), '9 levels: not refused, or something was written'
    targets_case(dev, 'G = 0', [pts0], torch.zeros(0, 9), torch.zeros(0, dtype=torch.long))
    rc, _, _, _, _, npos, _, bufs = targets_call(dev, [], boxes, torch.tensor([4, 5, 6]))
    assert rc == 0 and int(npos[0]) == 0 and all(bool((b == (SENT if b.dtype == torch.float32 else ISENT)).all()) for b in bufs[:4])


# ------------------------------------------------------------------------------------------------------------------ predict
def test_predict_scores_on_the_shape_grid(dev):
    hip = _hip()
    stats = S.Stats('predict_scores')
    g = _gen(6)
    for n in (1, 3, 5):
        for C in (1, 64, 65, 284):
            ldh = 13 + C + 3
            HO = Cols(dev, n, ldh - 1, ldh, 0, torch.randn(n, ldh - 1, generator=g) * 3)
            sc, sc_buf = _flat(dev, torch.full((n, C), SENT))
            mx, mx_buf = _flat(dev, torch.full((n,), SENT))
            hip.call('es_predict_scores', HO.ptr(), ldh, n, C, hip.P(sc), hip.P(mx), _st())
            torch.cuda.synchronize()
            label = f'scores n={n} C={C}'
            _tail_ok(sc_buf, n * C, label)
            _tail_ok(mx_buf, n, label)
            S.check_scores(label, HO.v, C, sc, mx, stats)
    print(stats.report())


def test_decode_boxes_with_and_without_an_index_list(dev):
    hip = _hip()
    stats = S.Stats('decode_boxes')
    g = _gen(8)
    eb, _, ep = edge_rows()
    for m in (1, 128, 129):
        n = m + 5
        bbox = torch.cat([torch.rand(n, 6, generator=g) + 0.2, torch.randn(n, 6, generator=g)], 1)
        pts = torch.randn(n, 3, generator=g) * 3
        bbox[-5:], pts[-5:] = eb, ep
        for idx in (None, torch.cat([torch.arange(n - 1, n - 6, -1), torch.randint(0, n, (m,), generator=g)])[:max(m, 5)].int()):
            mm = m if idx is None else idx.numel()
            d_b, d_p = bbox.to(dev), pts.to(dev)
            d_i = None if idx is None else idx.to(dev)
            out, out_buf = _flat(dev, torch.full((mm, 9), SENT))
            hip.call('es_decode_boxes', hip.P(d_p), hip.P(d_b), hip.P(d_i), mm, hip.P(out), _st())
            torch.cuda.synchronize()
            label = f'decode m={mm} idx={"none" if idx is None else "list"}'
            _tail_ok(out_buf, mm * 9, label)
            S.check_decode_boxes(label, d_p, d_b, d_i, out, stats)
    print(stats.report())


def nms_boxes(M, g, aligned=False):
    """clustered boxes; the first rows are the special ones: exact duplicates, nested, touching, quarter turns"""
    nc = max(M // 12, 1)
    centers = torch.rand(nc, 3, generator=g) * math.sqrt(nc) * 2.5
    boxes = torch.cat([centers[torch.randint(0, nc, (M,), generator=g)] + torch.randn(M, 3, generator=g) * 0.2, torch.rand(M, 3, generator=g) * 1.2 + 0.4,
                       torch.rand(M, 3, generator=g) * 6.2 - 3.1], 1)
    if M >= 16:
        boxes[1] = boxes[0]
        boxes[2] = boxes[0]                                     # exact duplicates
        boxes[3] = torch.tensor([50.0, 50, 0, 2, 2, 1, 0, 0, 0])
        boxes[4] = torch.tensor([50.0, 50, 0, 1, 1, 1, 0, 0, 0])   # nested: IoU 1 / 4 .. exactly the usual threshold: moved off it below
        boxes[4, 3] = 1.5
        boxes[5] = torch.tensor([52.0, 50, 0, 2, 2, 1, 0, 0, 0])   # touches box 3 along an edge
        boxes[6] = torch.tensor([60.0, 60, 0, 2, 1, 1, 0, 0, 0])
        boxes[7] = torch.tensor([60.0, 60, 0, 1, 2, 1, math.pi / 2, 0, 0])   # the same footprint after a quarter turn
        boxes[8] = torch.tensor([60.0, 60, 0, 2, 1, 1, math.pi, 0, 0])
    if aligned:
        boxes[:, 6:] = 0
    return boxes


def nms_case(dev, M, C, scores, boxes, score_thr, iou_thr, aligned=False):
    hip = _hip()
    d_b, d_s = boxes.to(dev), scores.to(dev).contiguous()
    ki, ki_buf = _ibuf(dev, C * M)
    kc, kc_buf = _ibuf(dev, C)
    rc = _rc('es_nms3d_multiclass', hip.P(d_b), hip.P(d_s), M, C, score_thr, iou_thr, hip.P(ki), hip.P(kc), _st())
    torch.cuda.synchronize()
    assert bool((ki_buf[C * M:] == ISENT).all()) and bool((kc_buf[C:] == ISENT).all())
    return rc, ki.view(C, M).cpu(), kc.cpu(), (ki_buf, kc_buf)


def test_nms_over_candidate_counts_ties_and_special_pairs(dev):
    g = _gen(9)
    past_block = 0
    for M in (1, 256, 257, 1000):
        C = 3
        boxes = nms_boxes(M, g)
        scores = torch.rand(M, C, generator=g)
        scores[:, 0] = scores[:, 0] * 0.6 + 0.35 if M <= 257 else scores[:, 0]          # every row a candidate of class 0 (M <= 257)
        scores[:, 1] = 0.0                                                            # a class without candidates
        scores[:, 2] = torch.where(torch.rand(M, generator=g) < 0.4, torch.tensor(0.5), torch.tensor(0.1))   # all-equal scores: index order
        past_block += int((scores[:, 0] > 0.3).sum()) > 256
        rc, ki, kc, _ = nms_case(dev, M, C, scores, boxes, 0.3, 0.25)
        assert rc == 0
        total, margin = S.check_nms(f'nms M={M}', boxes, scores, 0.3, 0.25, ki, kc, ISENT)
        print(f'nms M={M}: kept {kc.tolist()}, smallest |IoU - thr| {margin:.3e}')
        assert margin > 1e-9 and int(kc[1]) == 0, 'a pair of the grid lies on the threshold'
    assert past_block >= 1, 'no class had more than 256 candidates'
    if not _small(dev):
        M = 4096                                                 # every score above the threshold in one class: np2 == NMS_CAP
        # 256 far-apart clusters of 16 concentric axis-aligned boxes whose sizes are multiples of 0.1: two footprints are equal along
        # an axis or differ by >= 0.05 per side, so the 1e-2 corner margin of the overlap routine never adds a corner the closed form
        # does not know, and no IoU (a ratio of integers below 400) comes near the threshold 0.2718
        cl = torch.arange(M) // 16
        boxes = torch.zeros(M, 9)
        boxes[:, 0], boxes[:, 1] = (cl % 16).float() * 5, (cl // 16).float() * 5
        boxes[:, 3:6] = torch.randint(4, 20, (M, 3), generator=g).float() / 10
        scores = torch.rand(M, 1, generator=g) * 0.5 + 0.4
        assert int((scores[:, 0] > 0.3).sum()) == 4096           # NMS_CAP candidates in one class
        rc, ki, kc, _ = nms_case(dev, M, 1, scores, boxes, 0.3, 0.2718)
        assert rc == 0
        total, margin = S.check_nms('nms M=4096', boxes, scores, 0.3, 0.2718, ki, kc, ISENT, aligned=True)
        from oracle import predict as PR
        b = boxes.double().numpy()
        for i in torch.randint(0, M, (300,), generator=g).tolist():
            j = i // 16 * 16 + (i * 7 + 3) % 16                  # a box of the same cluster
            assert abs(PR.iou_bev(b[i], b[j]) - float(S.aligned_iou_bev(b[i], b[j]))) < 1e-9
        print(f'nms M=4096: kept {int(kc[0])}, smallest |IoU - thr| {margin:.3e}')
        assert margin > 1e-9 and 256 <= total < M
    boxes = nms_boxes(4097, g, aligned=True)
    rc, ki, kc, (ki_buf, kc_buf) = nms_case(dev, 4097, 1, torch.ones(4097, 1), boxes, 0.3, 0.25)
    assert rc == -10 and bool((ki_buf == ISENT).all()) and bool((kc_buf == ISENT).all()), 'M = 4097: not refused, or something was written'


# ------------------------------------------------------------------------------------------------------------------ occupancy
OCC_KINDS = ('normal', 'absent', 'no0', 'peaked', 'ignored', 'only0', 'only0_small', 'two8', 'two15')


def occ_inputs(n, C, kind, seed):
    g = _gen(seed)
    x = torch.randn(n, C, generator=g)
    t = torch.randint(0, C, (n,), generator=g)
    ign = torch.rand(n, generator=g) < 0.2
    if kind == 'absent' and C > 2:
        t[t == C - 1] = 1
    elif kind == 'no0' and C > 1:
        t[t == 0] = 1
    elif kind == 'peaked':
        x = (torch.randint(0, 2, (n, C), generator=g) * 60 - 30).float()
    elif kind == 'ignored':
        ign[:] = True
    elif kind in ('only0', 'only0_small'):
        t[:] = 0
    elif kind in ('two8', 'two15'):
        t[:] = 0
        ign[:] = False
        t[[n // 3, n // 2]] = min(3, C - 1)
        x[:, 0] += 8.0 if kind == 'two8' else 15.0
    t[ign] = 255
    return x, t.int()


def occ_loss_case(dev, stats, n, C, ld, kind, seed, weight=0.5, with_total=True, with_grad=True):
    hip = _hip()
    P = hip.P
    x, t = occ_inputs(n, C, kind, seed)
    L = Cols(dev, n, C, ld, 0, x)
    D = Cols(dev, n, C, ld + 2, 1)
    gt = t.to(dev)
    st = torch.full((3 * C + 2 + 4,), float(SENT), dtype=torch.float64, device=dev)
    co = torch.full((2 * C + 1 + 8,), SENT, dtype=torch.float32, device=dev)
    out = torch.full((4 + 8,), SENT, dtype=torch.float32, device=dev)
    tot = torch.tensor([2.5, SENT], dtype=torch.float32, device=dev)
    hip.call('es_occ_loss', L.ptr(), ld, P(gt), n, C, weight, P(st), P(co), D.ptr() if with_grad else 0, D.ld, P(out), P(tot) if with_total else 0, _st())
    torch.cuda.synchronize()
    label = f'{stats.label}: occ_loss n={n} C={C} ld={ld} {kind}'
    D.untouched_outside(label)
    L.untouched_outside(label)
    assert bool((st[3 * C + 2:] == SENT).all()) and bool((co[2 * C + 1:] == SENT).all()) and bool((out[4:] == SENT).all()) and float(tot[1]) == SENT, \
        f'{label}: stats / coeff / out / total_acc written past their ends'
    if not with_grad:
        assert bool((D.buf == SENT).all())
    if not with_total:
        assert float(tot[0]) == 2.5
    S.check_occ_stats(label, L.v, gt, C, st[:3 * C + 2], dev, stats)
    return S.check_occ_stage2(label, L.v, gt, C, weight, st[:3 * C + 2], out[:4], 2.5 if with_total else None, float(tot[0]) if with_total else None,
                              D.v if with_grad else None, dev, stats)


def test_occ_loss_on_the_shape_grid(dev):
    hip = _hip()
    stats = S.Stats('occ_loss grid')
    for i, (n, C, ld) in enumerate(((1, 2, 2), (7, 64, 70), (1030, 65, 65), (4099, 81, 81), (300, 256, 256))):
        occ_loss_case(dev, stats, n, C, ld, 'normal', 500 + i, with_total=i % 2 == 0, with_grad=i != 1)
    buf = torch.full((2048,), SENT, dtype=torch.float32, device=dev)
    st = torch.full((1024,), float(SENT), dtype=torch.float64, device=dev)
    gt = torch.zeros(8, dtype=torch.int32, device=dev)
    assert _rc('es_occ_loss', hip.P(buf), 257, hip.P(gt), 4, 257, 1.0, hip.P(st), hip.P(buf), hip.P(buf), 257, hip.P(buf), 0, _st()) != 0
    assert _rc('es_occ_loss', hip.P(buf), 8, hip.P(gt), 0, 8, 1.0, hip.P(st), hip.P(buf), hip.P(buf), 8, hip.P(buf), 0, _st()) != 0
    torch.cuda.synchronize()
    assert bool((buf == SENT).all()) and bool((st == SENT).all()), 'a refused es_occ_loss wrote something'
    print(stats.report())


@pytest.mark.parametrize('kind', OCC_KINDS)
def test_occ_loss_on_the_distributions_where_a_precision_or_recall_vanishes(dev, kind):
    """two8 / two15: two non-empty voxels among 2000 under a logit-0 offset; only0: every unmasked target is class 0 (n = 2000, C = 81 and
    n = 50, C = 5: the two cases whose gradient the split alpha + beta coefficients lost)"""
    stats = S.Stats(f'occ_loss {kind}')
    for n, C in {'only0': ((2000, 81),), 'only0_small': ((50, 5),)}.get(kind, ((2000, 12),)):
        k = occ_loss_case(dev, stats, n, C, C + (kind == 'normal'), kind, 600, weight=1.0)
        if kind in ('only0', 'only0_small', 'two15'):
            print(f'{kind} n={n} C={C}: alpha_0 {k["alpha"][0]:.3e}, beta_0 {k["beta"][0]:.3e}, gamma_0 {k["gamma"][0]:.3e}')
            assert abs(k['alpha'][0]) > (100 if kind == 'two15' else 1e4) * abs(k['gamma'][0]), 'the case does not reach the cancelling regime'
        if kind == 'ignored':
            assert math.isnan(k['out'][0]) and k['out'][2] == 300.0
    print(stats.report())


def occ_targets_case(dev, base, ratio, occ, mask):
    hip = _hip()
    X, Y, Z = (b // ratio for b in base)
    nv = X * Y * Z
    gt, gt_buf = _ibuf(dev, nv)
    scratch, sc_buf = _ibuf(dev, nv)
    d_occ = occ.to(torch.int32).to(dev).contiguous()
    d_m = None if mask is None else mask.to(torch.uint8).to(dev).contiguous()
    rc = _rc('es_occ_targets', hip.P(d_occ) if occ.shape[0] else 0, occ.shape[0], ratio, X, Y, Z, hip.P(d_m), hip.P(scratch), hip.P(gt), _st())
    torch.cuda.synchronize()
    assert rc == 0 and bool((gt_buf[nv:] == ISENT).all()) and bool((sc_buf[nv:] == ISENT).all())
    S.check_occ_targets(f'occ_targets ratio={ratio} n={occ.shape[0]} mask={mask is not None}', occ.cpu(), ratio, (X, Y, Z), mask, gt.cpu())
    return gt.cpu()


def test_occ_targets_duplicates_outside_rows_and_hidden_windows(dev):
    hip = _hip()
    g = _gen(12)
    base = (12, 20, 8)                                           # 1920 voxels: no multiple of 256
    n = 900
    occ = torch.cat([torch.stack([torch.randint(-3, b + 3, (n,), generator=g) for b in base], 1), torch.randint(1, 81, (n, 1), generator=g)], 1)
    occ[:50, :3] = occ[50:100, :3]                               # duplicates with other labels: the last wins
    occ[100] = torch.tensor([-1, 0, 0, 9])                       # -1 / ratio truncates to 0 for ratio > 1
    mask = torch.rand(*base, generator=g) < 0.7
    mask[4:8, 8:12, 0:4] = False                                 # an all-hidden window at every ratio
    for ratio in (1, 2, 4):
        for m in (None, mask):
            gt = occ_targets_case(dev, base, ratio, occ, m)
            if m is not None:
                assert int((gt == 255).sum()) >= (4 // ratio) ** 3
        occ_targets_case(dev, base, ratio, occ[:0], mask)
    dup = torch.tensor([[1, 1, 1, 5], [1, 1, 1, 6]])
    assert int(occ_targets_case(dev, base, 1, dup, None)[(1 * 20 + 1) * 8 + 1]) == 6
    assert int(occ_targets_case(dev, base, 2, torch.tensor([[-1, 0, 0, 9]]), None)[0]) == 9
    buf = torch.full((64,), ISENT, dtype=torch.int32, device=dev)
    assert _rc('es_occ_targets', hip.P(buf), 1, 0, 2, 2, 2, 0, hip.P(buf), hip.P(buf), _st()) != 0
    torch.cuda.synchronize()
    assert bool((buf == ISENT).all()), 'ratio = 0 wrote something'
