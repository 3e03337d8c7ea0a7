"""tests/test_gpu_head_kernels.py on the CPU emulator (tests/emu): the same bodies on their reduced grid (no M = 4096 NMS; the TG_CAP,
grid-stride and wave-boundary cases kept), under the `emulated` fixture of tests/test_emu_product.py (random thread schedule);
es_pos_losses and the NMS also under schedules 0 and 1.  Then the checker itself: for every specification class a correct output with
ONE thing wrong must be rejected, and the f32 torch evaluation of each formula -- no kernel -- must pass the same checker on the same
inputs (the bounds are attainable, and not vacuous).
TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes
import math

import numpy as np
import pytest
import torch

import head_spec as S
import test_gpu_head_kernels as T
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)

CPU = torch.device('cpu')


def _schedule(order):
    import build as emu_build
    lib = ctypes.CDLL(emu_build.build())
    lib.es_emu_set_schedule.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
    lib.es_emu_set_schedule(order, 4242)


def test_focal_loss_on_the_shape_grid(emulated):  # noqa: F811
    T.test_focal_loss_on_the_shape_grid(emulated)
    T.test_focal_loss_on_saturated_logits(emulated)


def test_reg_decode_at_the_clamp_and_past_the_grid_stride(emulated):  # noqa: F811
    T.test_reg_decode_at_the_clamp_and_past_the_grid_stride(emulated)


def test_pos_losses_and_box_cd_pairs(emulated):  # noqa: F811
    T.test_pos_losses_over_levels_wave_edges_and_ill_conditioned_rotations(emulated)
    T.test_box_cd_pairs_over_batches_and_unmatched_rows(emulated)


@pytest.mark.parametrize('order', [0, 1])
def test_pos_losses_and_nms_under_other_schedules(emulated, order):  # noqa: F811
    _schedule(order)
    stats = S.Stats(f'schedule {order}')
    sizes, npos, kind, ldh, edges = T.POS_CASES[-1]
    T.pos_losses_case(emulated, stats, sizes, npos, kind, ldh, 333, edges)
    g = T._gen(90 + order)
    M, C = 257, 2
    boxes, scores = T.nms_boxes(M, g), torch.rand(M, C, generator=g) * 0.6 + 0.35
    rc, ki, kc, _ = T.nms_case(emulated, M, C, scores, boxes, 0.3, 0.25)
    total, margin = S.check_nms(f'nms schedule {order}', boxes, scores, 0.3, 0.25, ki, kc, T.ISENT)
    assert rc == 0 and margin > 1e-9
    print(stats.report())


def test_get_targets_bit_exact_through_every_branch(emulated):  # noqa: F811
    T.test_get_targets_bit_exact_through_every_branch(emulated)


def test_predict_scores_decode_and_nms(emulated):  # noqa: F811
    T.test_predict_scores_on_the_shape_grid(emulated)
    T.test_decode_boxes_with_and_without_an_index_list(emulated)
    T.test_nms_over_candidate_counts_ties_and_special_pairs(emulated)


def test_occ_loss_on_the_shape_grid(emulated):  # noqa: F811
    T.test_occ_loss_on_the_shape_grid(emulated)


@pytest.mark.parametrize('kind', T.OCC_KINDS)
def test_occ_loss_on_the_distributions_where_a_precision_or_recall_vanishes(emulated, kind):  # noqa: F811
    T.test_occ_loss_on_the_distributions_where_a_precision_or_recall_vanishes(emulated, kind)


def test_occ_targets_duplicates_outside_rows_and_hidden_windows(emulated):  # noqa: F811
    T.test_occ_targets_duplicates_outside_rows_and_hidden_windows(emulated)


# ------------------------------------------------------------------------------------------------------------ the formulas alone, and the checker rejects
def _rejected(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError(f'the checker accepted {what}')


def _focal_rec(x, labels, ga, grad, loss1, avg=3.7, gs=0.5):
    return dict(logits=x, labels=labels, gamma=ga, alpha=0.25, avg=float(torch.tensor(avg, dtype=torch.float32)), grad_scale=gs, grad=grad, loss0=0.0,
                loss1=float(loss1))


@pytest.mark.parametrize('ga', [2.0, 1.5])
def test_focal_reference_alone_meets_the_bounds(ga):
    stats = S.Stats('focal reference')
    for N, C, seed in ((5, 65, 1), (300, 7, 2)):
        x, labels = T.focal_inputs(N, C, seed)
        g, l = S.focal_ref_f32(x, labels, ga, 0.25, 3.7, 0.5)
        S.check_focal_head(_focal_rec(x, labels, ga, g, l), CPU, stats)
    vals = torch.tensor([17.0, -17.0, 30.0, -30.0, 100.0, -100.0])
    x, labels = vals[:, None].repeat(2, 2), torch.tensor([0] * 6 + [-1] * 6)
    g, l = S.focal_ref_f32(x, labels, ga, 0.25, 3.7, 0.5)
    S.check_focal_head(_focal_rec(x, labels, ga, g, l), CPU, stats)
    print(stats.report())


def test_checker_rejects_wrong_focal_outputs():
    """one gradient 4 ulp off; a label C treated as class C - 1"""
    x, labels = T.focal_inputs(300, 65, 1)
    labels[0], x[0, 64] = 65, 2.0
    g, l = S.focal_ref_f32(x, labels, 2.0, 0.25, 3.7, 0.5)
    rec = _focal_rec(x, labels, 2.0, g, l)
    S.check_focal_head(rec, CPU, S.Stats('good'))
    # 4 ulp away from the specification, at the element where that uses the largest share of the bound
    spec, bound_u, _ = S.focal_grad_spec(rec, CPU)
    e0 = g.double() - spec
    ulp = torch.from_numpy(np.spacing(g.abs().numpy())).double()
    i = int(((e0.abs() + 4 * ulp) / (S.U * bound_u)).argmax())
    bad = g.clone()
    step = np.float32(9) if float(e0.view(-1)[i]) >= 0 else np.float32(-9)
    v = np.float32(bad.view(-1)[i])
    for _ in range(4):
        v = np.nextafter(v, step)
    bad.view(-1)[i] = float(v)
    _rejected(lambda: S.check_focal_head(_focal_rec(x, labels, 2.0, bad, l), CPU, S.Stats('4 ulp')), 'a focal gradient 4 ulp off')
    wrong = labels.clone()
    wrong[0] = 64
    g2, l2 = S.focal_ref_f32(x, wrong, 2.0, 0.25, 3.7, 0.5)
    _rejected(lambda: S.check_focal_head(_focal_rec(x, labels, 2.0, g2, l), CPU, S.Stats('label')), 'a label C treated as class C - 1 (gradient)')
    # the loss VALUE sees it where the f32 `1 - p` leaves it an interval narrower than one term: |x| <= 4
    x4 = x * 0.4
    _, l4 = S.focal_ref_f32(x4, labels, 2.0, 0.25, 3.7, 0.5)
    S.check_focal_head(_focal_rec(x4, labels, 2.0, None, l4), CPU, S.Stats('good'))
    _, l4 = S.focal_ref_f32(x4, wrong, 2.0, 0.25, 3.7, 0.5)
    _rejected(lambda: S.check_focal_head(_focal_rec(x4, labels, 2.0, None, l4), CPU, S.Stats('label')), 'a label C treated as class C - 1 (loss)')


def _reg_case(n=50, scale=0.7, seed=3):
    g = T._gen(seed)
    reg = torch.randn(n, 12, generator=g) * 2
    reg[:, :6] -= 2
    rows = T._clamp_rows(scale)
    for k in range(3):
        reg[k, :6] = rows[k]
    reg[5, 0] = -12.0
    sc = torch.tensor([scale])
    bbox = S.reg_decode_ref_f32(reg, sc)
    dbbox = torch.randn(n, 12, generator=g)
    dbbox[5, 0] = 0.75
    return reg, sc, bbox, dbbox


def test_reg_decode_reference_alone_meets_the_bounds():
    stats = S.Stats('reg_decode reference')
    for scale in (0.7, 1.0):
        reg, sc, bbox, dbbox = _reg_case(scale=scale)
        S.check_reg_decode_fwd('ref', reg, sc, bbox, stats)
        dreg, ds = S.reg_decode_bwd_ref_f32(reg, bbox, dbbox, sc)
        S.check_reg_decode_bwd('ref', reg, bbox, dbbox, sc, dreg, 0.75, float(torch.tensor(0.75) + ds), stats)
    print(stats.report())


def test_checker_rejects_wrong_reg_decode_gradients():
    """one dreg on the wrong side of the clamp, away from the ambiguous band; dscale missing one row"""
    reg, sc, bbox, dbbox = _reg_case()
    dreg, ds = S.reg_decode_bwd_ref_f32(reg, bbox, dbbox, sc)
    live = (bbox[:, :6] > 2 * S.LO3) & (dbbox[:, :6].abs() > 0.1)
    r, c = torch.nonzero(live)[0].tolist()
    bad = dreg.clone()
    bad[r, c] = 0.0
    _rejected(lambda: S.check_reg_decode_bwd('side', reg, bbox, dbbox, sc, bad, 0.0, float(ds), S.Stats('side')), 'a live dreg clamped to zero')
    # (a clamped element stores b == lo exactly: on the stored bbox it is inside the band where either side is accepted)
    row = int((torch.where(bbox[:, :6] > S.LO3, dbbox[:, :6] * bbox[:, :6] * reg[:, :6], torch.zeros(1)).sum(1)).abs().argmax())
    _, ds_bad = S.reg_decode_bwd_ref_f32(reg, bbox, dbbox, sc, skip_row=row)
    _rejected(lambda: S.check_reg_decode_bwd('row', reg, bbox, dbbox, sc, dreg, 0.0, float(ds_bad), S.Stats('row')), 'dscale missing one row')


def _cd_rec(seed=4, B=2, Q=9, Gs=(4, 3)):
    g = T._gen(seed)

    def boxes(n):
        return torch.cat([torch.randn(n, 3, generator=g), torch.rand(n, 3, generator=g) + 0.3, torch.rand(n, 3, generator=g) * 6 - 3], 1)
    pred, gt = boxes(B * Q), boxes(sum(Gs))
    q2g = torch.full((B, Q), -1, dtype=torch.int32)
    q2g[0, :Gs[0]] = torch.arange(Gs[0], dtype=torch.int32)
    q2g[1, :Gs[1]] = torch.arange(Gs[1], dtype=torch.int32)
    return dict(pred=pred, q2g=q2g.reshape(-1), B=B, Q=Q, gt=gt, gt_off=[0, Gs[0], sum(Gs)], n_pairs=sum(Gs), grad_scale=0.5, w=T.W4, sent=T.SENT,
                acc0=torch.zeros(1, dtype=torch.float64))


def _cd_outputs(rec, w=None, choice='first'):
    """dpred and the loss sum from the f64 formula, rounded to f32 once (what a correct kernel writes)"""
    sel = torch.nonzero(rec['q2g'] >= 0).squeeze(1)
    off = torch.tensor(rec['gt_off'][:-1])
    tgt = rec['gt'].double()[off[sel // rec['Q']] + rec['q2g'][sel].long()]
    x = rec['pred'].double()[sel].clone().requires_grad_(True)
    tot, _ = S.cd_rows(x, tgt, [float(torch.tensor(v, dtype=torch.float32)) for v in (w or rec['w'])], choice)
    (gr,) = torch.autograd.grad(tot.sum(), x)
    inv = float(torch.tensor(1.0) / (torch.tensor(float(rec['n_pairs'])) * 8.0))
    dp = torch.full((rec['B'] * rec['Q'], 9), rec['sent'])
    dp[sel] = (gr * inv * 0.5).float()
    return dp, (tot.detach() * inv).float().double().sum().reshape(1)


def test_checker_rejects_wrong_corner_chamfer_gradients():
    """the second-nearest corner used in one row; one decouple group's weight swapped"""
    rec = _cd_rec()
    dp, acc = _cd_outputs(rec)
    S.check_box_cd_pairs(dict(rec, dpred=dp, acc1=acc), CPU, S.Stats('good'))
    dp2, acc2 = _cd_outputs(rec, choice='second')
    assert float(acc2) > float(acc)                              # (the L1 gradient is a sign vector: it may not change, the distance does)
    _rejected(lambda: S.check_box_cd_pairs(dict(rec, dpred=dp2, acc1=acc2), CPU, S.Stats('second')), 'the second-nearest corner in one row')
    dp3, acc3 = _cd_outputs(rec, w=[0.2, 0.4, 0.2, 0.2])
    _rejected(lambda: S.check_box_cd_pairs(dict(rec, dpred=dp3, acc1=acc), CPU, S.Stats('weights')), 'a swapped group weight (gradient)')
    _rejected(lambda: S.check_box_cd_pairs(dict(rec, dpred=dp, acc1=acc3), CPU, S.Stats('weights')), 'a swapped group weight (loss)')


def test_checker_rejects_wrong_targets():
    """a target taken from the equal-volume second box; the k-th threshold taken inclusively"""
    from oracle import geometry as OG
    g = T._gen(5)
    pin = torch.cat([(torch.rand(15, 3, generator=g) * 2 - 1) * 0.4, torch.rand(10, 3, generator=g) + 5])
    nested = torch.cat([T._box((0, 0, 0), (2, 1, 1)), T._box((0, 0, 0), (1, 2, 1))])
    labels = torch.tensor([1, 2])
    ct, bt, kt = OG.get_targets([pin], nested, labels, 5, 18)
    bi = torch.where(kt >= 0, 0, -1).int()
    assert int((kt >= 0).sum()) == 15
    S.check_targets('good', [pin], nested, labels, 5, 18, ct, bt, kt.int(), bi, 15)
    bt2, kt2, bi2 = bt.clone(), kt.clone(), bi.clone()
    bt2[3], kt2[3], bi2[3] = nested[1], 2, 1
    _rejected(lambda: S.check_targets('second', [pin], nested, labels, 5, 18, ct, bt2, kt2.int(), bi2, 15), 'a target from the equal-volume second box')
    ax = torch.tensor([-0.75, -0.5, -0.25, 0.25, 0.5, 0.75])
    lat = torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1).reshape(-1, 3)
    cube, lab1 = T._box((0, 0, 0), (2, 2, 2)), torch.tensor([2])
    ct, bt, kt = OG.get_targets([lat], cube, lab1)
    S.check_targets('good', [lat], cube, lab1, 27, 18, ct, bt, kt.int(), torch.where(kt >= 0, 0, -1).int(), 8)
    cen = OG.centerness_from_faces(OG.face_distances(lat, cube))[:, 0]
    kt_inc = torch.where(cen >= cen.sort(descending=True).values[18], 2, -1)
    assert int((kt_inc >= 0).sum()) == 32
    _rejected(lambda: S.check_targets('inclusive', [lat], cube, lab1, 27, 18, ct, bt, kt_inc.int(), torch.where(kt_inc >= 0, 0, -1).int(), 32),
              'the k-th threshold taken inclusively')


def test_checker_rejects_wrong_nms_and_scores():
    """two kept NMS indices swapped; one kept duplicate; max_scores from another row"""
    g = T._gen(6)
    M = 40
    boxes, scores = T.nms_boxes(M, g), torch.rand(M, 1, generator=g) * 0.6 + 0.35
    scores[:3, 0] = torch.tensor([0.99, 0.98, 0.97])             # rows 0, 1, 2 are exact duplicates: the first is kept
    keep, _ = S.nms_margin(boxes, scores[:, 0], float(torch.tensor(0.25, dtype=torch.float32)))
    from oracle import predict as PR
    assert keep == PR.nms3d(boxes[:, :7], scores[:, 0], float(torch.tensor(0.25, dtype=torch.float32))).tolist()
    ki = torch.full((1, M), T.ISENT, dtype=torch.int32)
    ki[0, :len(keep)] = torch.tensor(keep, dtype=torch.int32)
    kc = torch.tensor([len(keep)], dtype=torch.int32)
    S.check_nms('good', boxes, scores, 0.3, 0.25, ki, kc, T.ISENT)
    sw = ki.clone()
    sw[0, [2, 3]] = sw[0, [3, 2]]
    _rejected(lambda: S.check_nms('swapped', boxes, scores, 0.3, 0.25, sw, kc, T.ISENT), 'two kept indices swapped')
    assert keep[0] == 0 and 1 not in keep and 2 not in keep
    first, other = 0, 1
    dup = ki.clone()
    pos = keep.index(first)
    dup[0, pos + 2:len(keep) + 1] = ki[0, pos + 1:len(keep)]
    dup[0, pos + 1] = other
    _rejected(lambda: S.check_nms('duplicate', boxes, scores, 0.3, 0.25, dup, kc + 1, T.ISENT), 'a kept duplicate')
    ho = torch.randn(4, 13 + 65, generator=g) * 3
    sc = (torch.sigmoid(ho[:, 13:].double()) * torch.sigmoid(ho[:, :1].double())).float()
    mx = sc.max(1).values
    stats = S.Stats('scores')
    S.check_scores('good', ho, 65, sc, mx, stats)
    _rejected(lambda: S.check_scores('max', ho, 65, sc, mx.roll(1), stats), 'max_scores from another row')
    bad = sc.clone()
    bad[2, 7] *= 1 + 2.0 ** -19
    _rejected(lambda: S.check_scores('score', ho, 65, bad, bad.max(1).values, stats), 'a score 32 u off')


@pytest.mark.parametrize('kind', T.OCC_KINDS)
def test_occ_reference_alone_meets_the_bounds(kind):
    stats = S.Stats(f'occ reference {kind}')
    for n, C in {'only0': ((2000, 81),), 'only0_small': ((50, 5),)}.get(kind, ((400, 12), (7, 64))):
        x, t = T.occ_inputs(n, C, kind, 600)
        st, out, d = S.occ_ref_f32(x, t, C, 0.5)
        S.check_occ_stats('ref', x, t, C, st, CPU, stats)
        S.check_occ_stage2('ref', x, t, C, 0.5, st, out, 2.5, float(torch.tensor(2.5) + out[3]), d, CPU, stats)
    print(stats.report())


@pytest.mark.parametrize('kind', T.OCC_KINDS)
def test_occ_specification_is_the_f64_autograd_of_the_oracle(kind):
    """the closed-form alpha / gamma coefficients of head_spec.occ_coeffs against autograd through oracle.occ (ce + sem + geo) in f64"""
    from oracle import occ as OO
    if kind == 'ignored':
        return                                                   # NaN cross-entropy: nothing to differentiate
    for n, C in ((300, 12), (1, 2), (50, 5)):
        x, t = T.occ_inputs(n, C, kind, 600)
        if not bool((t != 255).any()):
            continue
        xd = x.double().requires_grad_(True)
        pred, gt = xd.t()[None, :, :, None, None], t.long()[None, :, None, None]
        loss = torch.nn.functional.cross_entropy(pred, gt, ignore_index=255) + OO.sem_scal_loss(pred, gt) + OO.geo_scal_loss(pred, gt)
        (ref,) = torch.autograd.grad(loss, xd)
        st, _, _ = S.occ_ref_f32(x, t, C, 1.0)
        p = torch.softmax(x.double(), 1) * (t != 255)[:, None]
        oh = (t.long()[:, None] == torch.arange(C)[None]) & (t != 255)[:, None]
        st64 = torch.cat([p.sum(0), (p * oh).sum(0), oh.double().sum(0), torch.tensor([float((t != 255).sum()), 0.0], dtype=torch.float64)])
        k = S.occ_coeffs(st64.numpy(), C, 1.0)
        g = torch.where(oh, torch.from_numpy(k['gamma'])[None], torch.from_numpy(k['alpha'])[None])
        pp = torch.softmax(x.double(), 1)
        d = pp * (g - (pp * g).sum(1, keepdim=True)) + k['ce_scale'] * (pp - oh.double())
        d = d * (t != 255)[:, None]
        err = float((d - ref).abs().max())
        print(f'{kind} n={n} C={C}: closed form vs f64 autograd {err:.2e} of {float(ref.abs().max()):.2e}')
        assert err <= 1e-8 * float(ref.abs().max()) + 1e-13        # (the autograd side cancels in f64 where alpha_0 reaches 1e5)


def test_checker_rejects_the_split_occupancy_coefficients_and_first_wins_targets():
    """the occupancy gradient built from f32(alpha) + f32(beta) -- what k_occ_grad did before gamma was formed analytically -- on the two
    cases where it lost the gradient: every unmasked target class 0 (n = 2000, C = 81) and two non-empty voxels under a logit-0 offset of
    15; a first-wins duplicate in the occupancy targets"""
    for n, C, kind in ((2000, 81, 'only0'), (2000, 12, 'two15')):
        x, t = T.occ_inputs(n, C, kind, 600)
        st, out, d = S.occ_ref_f32(x, t, C, 1.0)
        S.check_occ_stage2('good', x, t, C, 1.0, st, out, None, None, d, CPU, S.Stats('good'))
        _, _, bad = S.occ_ref_f32(x, t, C, 1.0, split=True)
        print(f'{kind}: split coefficients move the gradient by up to {float((bad - d).abs().max()):.3e} of {float(d.abs().max()):.3e}')
        _rejected(lambda: S.check_occ_stage2('split', x, t, C, 1.0, st, out, None, None, bad, CPU, S.Stats('split')), f'the split coefficients ({kind})')
    occ = torch.tensor([[1, 1, 1, 5], [1, 1, 1, 6], [0, 1, 0, 3]])
    gt = torch.zeros(2 * 3 * 2, dtype=torch.int32)
    gt[(1 * 3 + 1) * 2 + 1], gt[2] = 6, 3
    S.check_occ_targets('good', occ, 1, (2, 3, 2), None, gt)
    gt[(1 * 3 + 1) * 2 + 1] = 5
    _rejected(lambda: S.check_occ_targets('first', occ, 1, (2, 3, 2), None, gt), 'a first-wins duplicate')
