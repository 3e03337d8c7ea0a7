"""Many prompts per scan on one shared scene encoding, training side: SparseFeatureFusion3DGrounder.loss_shared / loss_shared_from_tokens /
train_step_shared, engine.gather_rows_shared and the taped engine.attention_kv, decoder.forward_shared_train, and the kernel under the
gather's backward, es_rows_scatter_sum.

Kernel level: es_rows_scatter_sum against tests/shared_train_spec.py BIT FOR BIT on the issue's grid (L x P x Q x C, accumulate 0 / 1, dy and
dx column slices of wider buffers), over four kinds of index sets (every prompt the same rows; disjoint rows; one row shared by everybody and
the rest nobody else's; independent draws), with -0.0 among the values and a planted (1e8, 1, -1e8) triple on one shared row whose f32 sum
depends on the order; nothing written outside, two calls identical, refusals with the outputs untouched.
Decoder level (f32, from tokens): loss_shared_from_tokens against the oracle on the REPLICATED tokens under teacher-forced queries, at the
bounds tests/test_gpu_grounding.py holds the batched path to (assignments identical, losses 1e-3, gradients of parameters and of the token
features median 2e-3 / worst 1e-1), after HIP `loss` on the replicated tokens -- the code that existed before -- met the same bounds on the
same inputs; without forcing the selected queries and the assignments equal those of `loss` on the replicated batch exactly.
In situ (f32 and bf16): every 'attn' record of the shared path is held to ground_spec.check_attn_bwd and every 'scatter_sum' record to the
spec bit for bit.
Model level (GPU only): train_step_shared against train_step on the replicated batch and against the oracle.

Every body is a function of `dev`; tests/test_emu_shared_train.py runs them on the CPU emulator on a reduced grid."""
import types

import numpy as np
import pytest
import torch

import fwd_spec as F
import ground_spec as S
import shared_train_spec as SP
import test_gpu_ground_kernels as K

pytestmark = pytest.mark.gpu

SENT = K.SENT


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------ scatter-sum
KINDS = ('same', 'disjoint', 'common', 'random')


def scatter_indices(kind, P_, Q, L, g):
    """(idx (P_, Q) int32 with distinct entries per row, the kind actually built): a kind the shape has no room for falls back to 'random'"""
    perm = lambda n: torch.randperm(n, generator=g)
    if kind == 'disjoint' and P_ * Q <= L:
        return perm(L)[:P_ * Q].view(P_, Q).int(), kind
    if kind == 'common' and 1 + P_ * (Q - 1) <= L:
        rows = perm(L)
        idx = torch.empty(P_, Q, dtype=torch.int64)
        for p in range(P_):
            own = torch.cat([rows[:1], rows[1 + p * (Q - 1):1 + (p + 1) * (Q - 1)]])
            idx[p] = own[perm(Q)]                              # the shared row sits at a different position in every prompt
        return idx.int(), kind
    if kind == 'same':
        rows = perm(L)[:Q]
        return torch.stack([rows[perm(Q)] for _ in range(P_)]).int(), kind
    return torch.stack([perm(L)[:Q] for _ in range(P_)]).int(), 'random'


def scatter_case(dev, L, P_, Q, C, acc, kind, seed):
    hip = K._hip()
    P = hip.P
    g = torch.Generator().manual_seed(seed)
    idx, kind = scatter_indices(kind, P_, Q, L, g)
    dy = torch.randn(P_ * Q, C, generator=g)
    dy[torch.rand(P_ * Q, C, generator=g) < 0.1] = -0.0
    planted = False
    if P_ >= 3:                                               # a row three prompts share: 1e8 + 1 - 1e8 in ascending p is 0, in any other order it is not
        cnt = torch.bincount(idx.reshape(-1).long(), minlength=L)
        rows = torch.nonzero(cnt >= 3).reshape(-1)
        if rows.numel():
            ps = torch.nonzero((idx == int(rows[0])).any(1)).reshape(-1)[:3].tolist()
            for p, val in zip(ps, (1e8, 1.0, -1e8)):
                q = int(torch.nonzero(idx[p] == int(rows[0]))[0])
                dy[p * Q + q, 0] = val
            planted = True
    dx0 = torch.randn(L, C, generator=g)
    dx0[torch.rand(L, C, generator=g) < 0.1] = -0.0
    ldy, offy, ldx, offx = C + 8, 4, C + 12, 8
    DY = K.Cols(dev, P_ * Q, C, ldy, offy, dy)
    nws = int(hip.raw('es_rows_scatter_sum_workspace_ints')(P_, L))
    assert nws == P_ * L
    idx_d = idx.to(dev).contiguous()
    label = f'scatter-sum L={L} P={P_} Q={Q} C={C} acc={acc} {kind}'
    want = SP.scatter_sum_ref(dy.numpy(), idx.numpy(), L, acc, dx0.numpy())
    outs = []
    for rep in range(2):
        DX = K.Cols(dev, L, C, ldx, offx, dx0)
        ws = torch.full((nws + 8,), -77, dtype=torch.int32, device=dev)
        hip.call('es_rows_scatter_sum', DY.ptr(), ldy, P(idx_d), P_, Q, L, C, DX.ptr(), ldx, acc, P(ws), nws, K._st())
        if dev.type == 'cuda':
            torch.cuda.synchronize()
        DX.untouched_outside(label)
        DY.untouched_outside(label + ' (dy)')
        assert bool((ws[nws:] == -77).all()), f'{label}: the position table was written past P*L ints'
        assert torch.equal(DY.v.cpu(), dy) and torch.equal(idx_d.cpu(), idx), f'{label}: an input changed'
        got = DX.v.cpu().contiguous().numpy()
        bad = np.nonzero(SP.bits(got) != SP.bits(want))
        assert bad[0].size == 0, (f'{label}: {bad[0].size} elements differ from the ascending-p f32 sum, first at row {bad[0][0]} col {bad[1][0]}: '
                                  f'{got[bad[0][0], bad[1][0]]!r} vs {want[bad[0][0], bad[1][0]]!r}')
        outs.append(got)
    assert np.array_equal(SP.bits(outs[0]), SP.bits(outs[1])), f'{label}: two calls differ'
    nobody = bool((torch.bincount(idx.reshape(-1).long(), minlength=L) == 0).any())
    return kind, planted, nobody


def scatter_grid(dev):
    """the issue's grid; emulator: C = 256 only at L in {5, 1029} with the largest Q"""
    cases, i = [], 0
    for L in (1, 5, 33, 1029):
        for P_ in (1, 2, 5):
            for Q in sorted({1, min(L, 4), min(L, 33)}):
                for C in (4, 256):
                    if K._small(dev) and C == 256 and not (L in (5, 1029) and Q == min(L, 33)):
                        continue
                    for acc in (0, 1):
                        cases.append((L, P_, Q, C, acc, KINDS[i % 4]))
                        i += 1
    return cases


def test_scatter_sum_on_the_shape_grid(dev):
    seen, planted, nobody = set(), 0, 0
    for n, (L, P_, Q, C, acc, kind) in enumerate(scatter_grid(dev)):
        k, pl, nb = scatter_case(dev, L, P_, Q, C, acc, kind, 900 + n)
        seen.add(k)
        planted += pl
        nobody += nb
    print(f'scatter-sum: kinds {sorted(seen)}, {planted} cases with the order-sensitive triple, {nobody} with a row nobody selected')
    assert seen == set(KINDS) and planted >= 4 and nobody >= 4


def test_scatter_sum_order_sensitive_triple_is_order_sensitive():
    """the planted values do tell an ascending sum from another order (CPU only: the spec against a permuted spec)"""
    dy = np.array([[1e8], [1.0], [-1e8]], np.float32)
    idx = np.zeros((3, 1), np.int64)
    assert float(SP.scatter_sum_ref(dy, idx, 1)[0, 0]) == 0.0
    assert float(SP.scatter_sum_ref(dy[[0, 2, 1]], idx, 1)[0, 0]) == 1.0


def test_scatter_sum_refusals_leave_the_outputs_untouched(dev):
    hip = K._hip()
    P = hip.P
    L, P_, Q, C = 9, 2, 3, 8
    g = torch.Generator().manual_seed(5)
    idx = torch.stack([torch.randperm(L, generator=g)[:Q] for _ in range(P_)]).int().to(dev)
    dy = torch.full((P_ * Q, 16), 1.0, device=dev)
    dx = torch.full((L, 16), SENT, device=dev)
    ws = torch.full((P_ * L,), -77, dtype=torch.int32, device=dev)
    st = K._st()
    f = lambda *a: K._rc('es_rows_scatter_sum', *a)
    assert f(P(dy), 14, P(idx), P_, Q, L, C, P(dx), 16, 0, P(ws), P_ * L, st) == -3           # float4 rows, ld % 4 != 0
    assert f(P(dy), 16, P(idx), P_, Q, L, C, P(dx), 10, 0, P(ws), P_ * L, st) == -3
    assert f(P(dy), 4, P(idx), P_, Q, L, C, P(dx), 16, 0, P(ws), P_ * L, st) == -3            # ld below C
    assert f(P(dy), 16, P(idx), P_, L + 1, L, C, P(dx), 16, 0, P(ws), P_ * L, st) == -4       # Q > L
    assert f(P(dy), 16, P(idx), P_, Q, L, C, P(dx), 16, 0, P(ws), P_ * L - 1, st) == -5       # workspace one int short
    assert f(P(dy), 16, P(idx), P_, Q, L, C, P(dx), 16, 0, 0, 0, st) == -5
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    assert bool((dx == SENT).all()) and bool((ws == -77).all())
    # scalar rows (C % 4 != 0) take any leading dimension
    dx3 = torch.full((L, 7), SENT, device=dev)
    hip.call('es_rows_scatter_sum', P(dy), 16, P(idx), P_, Q, L, 3, P(dx3), 7, 0, P(ws), P_ * L, st)
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    want = SP.scatter_sum_ref(np.ones((P_ * Q, 3), np.float32), idx.cpu().numpy(), L)
    assert np.array_equal(SP.bits(dx3[:, :3].cpu().numpy()), SP.bits(want)) and bool((dx3[:, 3:] == SENT).all())


# ------------------------------------------------------------------------------------------------------------ attention backward, prepared
def attn_kv_bwd_case(dev, stats, bf, regime, H, Lq, Lk, acc, seed):
    """es_attn_kv_prepare + es_attn_kv_fwd + es_attn_kv_bwd on column slices, held to ground_spec.check_attn_bwd with B = 1; twice: the
    two calls must agree bit for bit; nothing is written outside the views, past the workspace or past delta"""
    hip = K._hip()
    P = hip.P
    E = H * 32
    q, k, v, do = K.attn_inputs(regime, 1, H, Lq, Lk, seed)
    lds = [E + 4 * (i + 1) for i in range(8)]
    Q, Kc, Vc, DO = (K.Cols(dev, r, E, ld, off, t) for (r, ld, off, t) in
                     ((Lq, lds[0], 4, q), (Lk, lds[1], 0, k), (Lk, lds[2], 8, v), (Lq, lds[3], 4, do)))
    O = K.Cols(dev, Lq, E, lds[4], 8)
    lse, _ = K._flat(dev, torch.zeros(H * Lq))
    kv = torch.empty(int(hip.raw('es_attn_kv_bytes')(H, Lk, bf)), dtype=torch.uint8, device=dev)
    st = K._st()
    hip.call('es_attn_kv_prepare', Kc.ptr(), Kc.ld, Vc.ptr(), Vc.ld, H, Lk, bf, P(kv), st)
    hip.call('es_attn_kv_fwd', Q.ptr(), Q.ld, P(kv), H, Lq, Lk, O.ptr(), O.ld, P(lse), bf, st)
    nws = int(hip.raw('es_attn_kv_bwd_workspace_bytes')(H, Lq, bf))
    QS = 64 if bf else 32
    assert nws == H * ((Lq + QS - 1) // QS) * 4 * QS * 32 * (2 if bf else 4)
    g = torch.Generator().manual_seed(seed + 1)
    pri = [torch.randn(n, E, generator=g) for n in (Lq, Lk, Lk)]
    label = f'attention kv bwd {regime} bf16={bf} H={H} Lq={Lq} Lk={Lk} acc={acc}'
    outs = []
    for poison in (0xFF, 0x4B):                                # the workspace holds NaN patterns / large finite values before the call
        DQ, DK, DV = (K.Cols(dev, r, E, ld, off, t) for (r, ld, off, t) in ((Lq, lds[5], 0, pri[0]), (Lk, lds[6], 12, pri[1]), (Lk, lds[7], 4, pri[2])))
        ws = torch.full((nws + 16,), poison, dtype=torch.uint8, device=dev)
        delta, delta_buf = K._flat(dev, torch.zeros(H * Lq))
        hip.call('es_attn_kv_bwd', Q.ptr(), Q.ld, Kc.ptr(), Kc.ld, Vc.ptr(), Vc.ld, O.ptr(), O.ld, DO.ptr(), DO.ld, P(lse), H, Lq, Lk, P(delta),
                 P(ws), nws, DQ.ptr(), DQ.ld, DK.ptr(), DK.ld, DV.ptr(), DV.ld, acc, bf, st)
        if dev.type == 'cuda':
            torch.cuda.synchronize()
        for c in (DQ, DK, DV, O):
            c.untouched_outside(label)
        K._tail_ok(delta_buf, H * Lq, label + ' delta')
        assert bool((ws[nws:] == poison).all()), f'{label}: the workspace was written past its size'
        rec = dict(B=1, H=H, Lq=Lq, Lk=Lk, bf=bf, q=Q.v, k=Kc.v, v=Vc.v, klen=None, o=O.v, lse=lse, do=DO.v, acc=acc, dq=DQ.v, dk=DK.v, dv=DV.v,
                   dq0=pri[0], dk0=pri[1], dv0=pri[2])
        S.check_attn_bwd(rec, dev, stats)
        outs.append((DQ.v.clone(), DK.v.clone(), DV.v.clone(), delta.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b), f'{label}: two calls differ (or the result depends on what the workspace held)'


# the issue's grid + this kernel's own edges: the query step is 64 rows in bf16 mode and 32 in f32 mode (31 / 32 / 33 join Lq), a workgroup
# owns 64 keys (63 / 64 / 65 / 130 are in the issue's Lk already)
KVB_LQ = (1, 31, 32, 33, 63, 64, 65, 99, 127, 128, 129, 257)
KVB_LK = (1, 31, 33, 63, 64, 65, 130)


def attn_kv_bwd_grid(dev, bf):
    """(regime, H, Lq, Lk, acc).  GPU: every (H, Lq, Lk) at H in {1, 8}, regimes and accumulate rotating.  Emulator: every Lq and every Lk
    at least once, H in {1, 2}"""
    cases, i = [], 0
    if not K._small(dev):
        for H in (1, 8):
            for Lq in KVB_LQ:
                for Lk in KVB_LK:
                    cases.append((K.REGIMES[i % 3], H, Lq, Lk, (i // 3) % 2))
                    i += 1
        return cases
    for n, Lq in enumerate(KVB_LQ):
        cases.append((K.REGIMES[(n + bf) % 3], 1 + (n + bf) % 2, Lq, KVB_LK[(n + 3 * bf) % len(KVB_LK)], (n + bf) % 2))
    return cases


@pytest.mark.parametrize('bf', [0, 1])
def test_attention_kv_bwd_on_the_tile_edge_grid(dev, bf):
    stats = F.Stats(f'attention kv bwd grid bf16={bf}')
    grid = attn_kv_bwd_grid(dev, bf)
    assert {c[2] for c in grid} == set(KVB_LQ) and {c[3] for c in grid} == set(KVB_LK) and {c[4] for c in grid} == {0, 1}
    for n, (regime, H, Lq, Lk, acc) in enumerate(grid):
        attn_kv_bwd_case(dev, stats, bf, regime, H, Lq, Lk, acc, 1200 + 2 * n + bf)
    print(stats.report())
    assert {c.split()[1] for c in stats.ratio if c.startswith('attn_bwd')} == {'dq', 'dk', 'dv'}


def test_attention_kv_bwd_reference_alone_meets_the_bounds():
    """the f32 torch evaluation of the formula (ground_spec.attn_ref, B = 1, no key mask) passes check_attn_bwd at the shapes of this file
    in all regimes and both modes: the bound is one the reference itself meets (CPU only: no kernel is looked at)"""
    dev = torch.device('cpu')
    stats = F.Stats('attention kv bwd reference')
    for n, regime in enumerate(K.REGIMES):
        for bf in (0, 1):
            for (H, Lq, Lk) in ((2, 99, 130), (1, 65, 33), (8, 1, 31), (1, 257, 65), (1, 129, 1)):
                q, k, v, do = K.attn_inputs(regime, 1, H, Lq, Lk, 27 + n)
                r = S.attn_ref(q, k, v, do, None, 1, H, Lq, Lk, bf)
                S.check_attn_bwd(dict(B=1, H=H, Lq=Lq, Lk=Lk, bf=bf, q=q, k=k, v=v, klen=None, o=r['o'], lse=r['lse'].reshape(-1), do=do, acc=0,
                                      dq=r['dq'], dk=r['dk'], dv=r['dv']), dev, stats)
    print(stats.report())


def test_attention_kv_bwd_refusals_leave_the_outputs_untouched(dev):
    """a leading dimension that is not a multiple of 4 returns -3, a missing / short / unaligned workspace -5; nothing is written"""
    hip = K._hip()
    P = hip.P
    H, Lq, Lk = 1, 5, 7
    t = lambda n: torch.full((n, 40), SENT, device=dev)
    q, k, v, o, do, dq, dk, dv = t(Lq), t(Lk), t(Lk), t(Lq), t(Lq), t(Lq), t(Lk), t(Lk)
    lse, delta = torch.full((Lq,), SENT, device=dev), torch.full((Lq,), SENT, device=dev)
    nws = int(hip.raw('es_attn_kv_bwd_workspace_bytes')(H, Lq, 1))
    ws = torch.full((nws + 16,), 0x5A, dtype=torch.uint8, device=dev)

    def rc(ld, wsp, n):
        return K._rc('es_attn_kv_bwd', P(q), ld[0], P(k), ld[1], P(v), ld[2], P(o), ld[3], P(do), ld[4], P(lse), H, Lq, Lk, P(delta), wsp, n,
                     P(dq), ld[5], P(dk), ld[6], P(dv), ld[7], 0, 1, K._st())
    for bad in range(8):
        ld = [36] * 8
        ld[bad] = 37 + bad % 2
        assert rc(ld, P(ws), nws) == -3
    assert rc([36] * 8, 0, nws) == -5 and rc([36] * 8, P(ws), nws - 1) == -5 and rc([36] * 8, P(ws) + 4, nws) == -5
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    for x in (o, dq, dk, dv, lse, delta):
        assert bool((x == SENT).all())
    assert bool((ws == 0x5A).all())


# ------------------------------------------------------------------------------------------------------------ decoder level, from tokens
# (text, target phrases): short and long prompts, one with two targets
PROMPTS = (('find the chair', ('chair',)),
           ('the lamp next to the window on the left side of the door', ('lamp',)),
           ('where is the other chair and the small shelf', ('other chair', 'small shelf')),
           ('a table', ('table',)))
TOKEN_SEED = 3


def _prompt(i, g):
    from embodiedscan_amd.pipeline import GroundingPrompt
    text, targets = PROMPTS[i % len(PROMPTS)]
    spans = [[(text.find(t), text.find(t) + len(t))] for t in targets]
    G = len(targets)
    boxes = torch.cat([torch.rand(G, 3, generator=g) * 3.0 - 1.5, torch.rand(G, 3, generator=g) * 0.9 + 0.3,
                       (torch.rand(G, 3, generator=g) - 0.5) * 0.6], 1)
    return GroundingPrompt(text, spans, boxes.numpy().astype(np.float32), np.zeros(G, np.int64))


def token_inputs(S_, P_, lens, seed=TOKEN_SEED):
    """(feats (S*Lmax, 256) with zero rows behind each scene's tokens, points likewise, S*P prompt records scan-major)"""
    g = torch.Generator().manual_seed(seed * 1000 + sum(lens) + 7 * P_)
    Lmax = max(lens)
    feats, points = torch.zeros(S_ * Lmax, 256), torch.zeros(S_ * Lmax, 3)
    for s, n in enumerate(lens):
        feats[s * Lmax:s * Lmax + n] = torch.randn(n, 256, generator=g)
        points[s * Lmax:s * Lmax + n] = torch.rand(n, 3, generator=g) * 4.0 - 2.0
    prompts = [_prompt(s * P_ + p + s, g) for s in range(S_) for p in range(P_)]
    return feats, points, prompts


def _begin(det):
    from embodiedscan_amd import engine as E
    E.WEIGHT_VERSION[0] += 1
    E.TAPE.clear()
    det._bind()
    det.arena.grad.zero_()
    E.new_grad_epoch()


def _sync(dev):
    if dev.type == 'cuda':
        torch.cuda.synchronize()


def hip_shared_from_tokens(det, dev, feats, points, lens, prompts, force=None):
    """one forward + backward of loss_shared_from_tokens -> dict(losses, grads, fgrad, q2g per layer, idx (free selection))"""
    from embodiedscan_amd import engine as E
    det.force_queries = force
    try:
        _begin(det)
        fv = E.Var(feats.to(dev).clone())
        losses = det.loss_shared_from_tokens(fv, points.to(dev), lens, prompts)
        out = dict(losses={k: float(v) for k, v in losses.items()}, q2g=[l['q2g'].cpu() for l in det.bbox_head.last],
                   idx=(det.free_queries if force is not None else det.last_queries['idx']).cpu())
        E.TAPE.backward()
        _sync(dev)
        out['grads'] = {k: v.cpu().clone() for k, v in det.arena.grad_dict().items()}
        out['fgrad'] = fv.g.cpu().clone()
    finally:
        det.force_queries = None
    return out


def hip_replicated_from_tokens(det, dev, feats, points, lens, prompts, S_, P_, force=None):
    """the code that existed before: forward_transformer + head loss on the REPLICATED padded tokens (scene s's rows P times) ->
    the same dict; fgrad = the P copies' gradients added per scene"""
    from embodiedscan_amd import engine as E
    Lmax = max(lens)
    rep = lambda t: t.view(S_, 1, Lmax, -1).expand(S_, P_, Lmax, t.shape[1]).reshape(S_ * P_ * Lmax, -1).contiguous()
    det.force_queries = force
    try:
        _begin(det)
        fv = E.Var(rep(feats).to(dev))
        det.neck_3d.last = dict(feats=fv, points=rep(points).to(dev), lens=[n for n in lens for _ in range(P_)], Lmax=Lmax)
        text, mask, tlen, T = det.encode_text(prompts)
        hidden, boxes = det.forward_transformer(text, tlen, T, prompts)
        losses = det.bbox_head.loss(hidden, boxes, text, mask, prompts, tlen=tlen)
        out = dict(losses={k: float(v) for k, v in losses.items()}, q2g=[l['q2g'].cpu() for l in det.bbox_head.last],
                   idx=(det.free_queries if force is not None else det.last_queries['idx']).cpu())
        E.TAPE.backward()
        _sync(dev)
        out['grads'] = {k: v.cpu().clone() for k, v in det.arena.grad_dict().items()}
        out['fgrad'] = fv.g.cpu().view(S_, P_, Lmax, -1).sum(1).reshape(S_ * Lmax, -1)
    finally:
        det.force_queries = None
    return out


def oracle_replicated(det, sd, feats, points, lens, prompts, S_, P_, coder):
    """oracle/grounding.py on the replicated token lists with the text hidden states the device produced (det.last_text of the last run)"""
    import torch.nn.functional as TF
    from oracle import grounding as OG
    names = set(det.arena.grad_dict().keys())
    osd = {k: v.clone().requires_grad_(k in names) for k, v in sd.items()}
    th, tmask = det.last_text['hidden'].float().cpu(), det.last_text['mask'].cpu()
    text = TF.linear(th, osd['text_feat_map.weight'], osd['text_feat_map.bias'])
    Lmax = max(lens)
    leaf = feats.clone().requires_grad_(True)
    fl = [leaf[s * Lmax:s * Lmax + lens[s]] for s in range(S_) for _ in range(P_)]
    pl = [points[s * Lmax:s * Lmax + lens[s]] for s in range(S_) for _ in range(P_)]
    gtb = [getattr(p.gt_instances_3d.bboxes_3d, 'tensor', p.gt_instances_3d.bboxes_3d).cpu() for p in prompts]
    pms = [p.gt_instances_3d.positive_maps.cpu() for p in prompts]
    hidden, boxes, aux = OG.forward_transformer(fl, pl, text, tmask, osd, num_queries=32, num_layers=2, coder=coder)
    losses, haux = OG.head_loss(hidden, boxes, text, tmask, osd, gtb, pms, return_aux=True)
    sum(losses.values()).backward()
    return dict(losses={k: float(v.detach()) for k, v in losses.items()}, grads={k: v.grad for k, v in osd.items() if v.grad is not None},
                fgrad=leaf.grad, idx=aux['idx'], assign=[torch.stack(list(h['assign'])) for h in haux])


SKIP_NORM = 1e-6
SKIP_CAP = 0.05


def held_to_oracle(label, h, o):
    """assignments identical, losses 1e-3, gradients of parameters and of the token features median 2e-3 / worst 1e-1"""
    import test_gpu_grounding as TG
    for l, a in enumerate(o['assign']):
        assert torch.equal((h['q2g'][l] + 1).long(), a.long()), f'{label}: Hungarian assignment of layer {l} differs from the oracle\'s'
    for k, w in o['losses'].items():
        e = abs(h['losses'][k] - w) / max(abs(w), 1e-6)
        print(f'{label} {k}: hip {h["losses"][k]:.6f} oracle {w:.6f} rel err {e:.2e} (tol 1e-3)')
        assert e < 1e-3
    skipped = [k for k, g in o['grads'].items() if float(g.norm()) <= SKIP_NORM]
    print(f'{label}: left out of the gradient comparison (oracle gradient norm <= {SKIP_NORM:g}): {skipped}')
    assert len(skipped) <= SKIP_CAP * len(o['grads']), f'{label}: {len(skipped)} of {len(o["grads"])} tensors skipped (cap 5 %)'
    rel = {k: TG._rel(h['grads'][k], g) for k, g in o['grads'].items() if k not in skipped}
    rel['<token features>'] = TG._rel(h['fgrad'], o['fgrad'])
    worst = max(rel, key=rel.get)
    med = float(np.median(list(rel.values())))
    print(f'{label}: {len(rel)} gradient tensors, median rel-L2 {med:.2e} (tol 2e-3), token features {rel["<token features>"]:.2e}, worst '
          f'{rel[worst]:.2e} at {worst} (tol 1e-1)')
    assert len(rel) > 50 and med < 2e-3 and rel[worst] < 1e-1
    assert all(np.isfinite(v) for v in h['losses'].values())


def shared_from_tokens_vs_oracle(dev, config, S_, P_, lens):
    import test_gpu_grounding as TG
    from embodiedscan_amd import engine as E
    cfg, det, sd = TG._small_grounder(dev, config=config)
    coder = det.bbox_head.box_coder
    assert E.PRECISION[0] == 'f32' and len(lens) == S_
    feats, points, prompts = token_inputs(S_, P_, lens)
    label = f'{coder} S={S_} P={P_} lens={lens}'
    # free runs: the shared path selects and assigns exactly what `loss` on the replicated batch does
    free_s = hip_shared_from_tokens(det, dev, feats, points, lens, prompts)
    free_r = hip_replicated_from_tokens(det, dev, feats, points, lens, prompts, S_, P_)
    assert torch.equal(free_s['idx'], free_r['idx']), f'{label}: the selected queries differ from those of `loss` on the replicated batch'
    assert all(torch.equal(a, b) for a, b in zip(free_s['q2g'], free_r['q2g'])), f'{label}: assignments differ from the replicated batch\'s'
    o = oracle_replicated(det, sd, feats, points, lens, prompts, S_, P_, coder)
    force = o['idx'].int()
    print(f'{label}: free selection equal to the oracle\'s: {torch.equal(free_s["idx"].long(), o["idx"])}')
    held_to_oracle(label + ' replicated `loss`', hip_replicated_from_tokens(det, dev, feats, points, lens, prompts, S_, P_, force=force), o)
    h = hip_shared_from_tokens(det, dev, feats, points, lens, prompts, force=force)
    held_to_oracle(label + ' loss_shared', h, o)
    Lmax = max(lens)
    for s, n in enumerate(lens):                               # padded rows carry no gradient
        assert not bool(h['fgrad'][s * Lmax + n:(s + 1) * Lmax].any()), f'{label}: a padded token row received a gradient'
    return det


@pytest.mark.parametrize('config', ['mv_grounding.py', 'mv_grounding_fcaf.py'])
def test_loss_shared_from_tokens_one_scene_three_prompts(dev, config):
    shared_from_tokens_vs_oracle(dev, config, 1, 3, [57])


@pytest.mark.parametrize('config', ['mv_grounding.py', 'mv_grounding_fcaf.py'])
def test_loss_shared_from_tokens_two_scenes_of_different_length(dev, config):
    shared_from_tokens_vs_oracle(dev, config, 2, 2, [43, 68])


def test_oracle_skips_few_gradient_tensors_on_these_inputs():
    """CPU only, the oracle alone: on the inputs above it puts at most 5 % of its gradient tensors below the 1e-6 norm threshold (the
    text hidden states are random here: they only scale the text side)"""
    import torch.nn.functional as TF
    from oracle import grounding as OG
    from embodiedscan_amd.params import ParamArena, grounder_specs
    from embodiedscan_amd.text import HashTokenizer, create_positive_map
    g = torch.Generator().manual_seed(0)
    arena = ParamArena(grounder_specs(text_dim=64, E=256, num_layers=2, ffn=128, in_channels=(64, 128, 256, 512)), seed=0)
    sd = {k: v.clone() for k, v in arena.state_dict().items() if k.startswith(('decoder.', 'bbox_head.', 'text_feat_map.'))}
    for k in sd:
        if 'reg_branches' in k and k.endswith('.4.weight'):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.05
        if 'reg_branches' in k and k.endswith('.4.bias'):
            sd[k] = torch.randn(sd[k].shape, generator=g) * 0.1
    for k in list(sd):
        if 'reg_branches.' in k and not k.startswith('bbox_head.reg_branches.0.'):
            sd[k] = sd['bbox_head.reg_branches.0.' + k.split('.', 3)[3]]
    tok = HashTokenizer()
    for S_, P_, lens in ((1, 3, [57]), (2, 2, [43, 68])):
        feats, points, prompts = token_inputs(S_, P_, lens)
        enc = tok.batch_encode_plus([p.text for p in prompts], padding='longest', return_tensors='pt')
        tmask = enc.attention_mask.bool()
        pms = [create_positive_map(enc, p.tokens_positive, i, 256).bool().float() for i, p in enumerate(prompts)]
        th = torch.randn(S_ * P_, tmask.shape[1], 64, generator=g)
        osd = {k: v.clone().requires_grad_(v.is_floating_point() and 'running' not in k) for k, v in sd.items()}
        text = TF.linear(th, osd['text_feat_map.weight'], osd['text_feat_map.bias'])
        Lmax = max(lens)
        fl = [feats[s * Lmax:s * Lmax + lens[s]] for s in range(S_) for _ in range(P_)]
        pl = [points[s * Lmax:s * Lmax + lens[s]] for s in range(S_) for _ in range(P_)]
        gtb = [p.gt_instances_3d.bboxes_3d.tensor for p in prompts]
        hidden, boxes, aux = OG.forward_transformer(fl, pl, text, tmask, osd, num_queries=32, num_layers=2)
        sum(OG.head_loss(hidden, boxes, text, tmask, osd, gtb, pms).values()).backward()
        grads = {k: v.grad for k, v in osd.items() if v.grad is not None}
        small = [k for k, v in grads.items() if float(v.norm()) <= SKIP_NORM]
        print(f'S={S_} P={P_} lens={lens}: {len(grads)} gradient tensors, below the threshold: {small}')
        assert len(grads) > 50 and len(small) <= SKIP_CAP * len(grads)


# ------------------------------------------------------------------------------------------------------------ in situ
def shared_records_in_situ(dev, mode, S_=2, P_=2, lens=(43, 68)):
    """loss_shared_from_tokens under engine.DEBUG_OPS: every 'attn' record the shared path made passes check_attn_bwd (B = 1), every
    'scatter_sum' record equals the spec bit for bit"""
    import test_gpu_grounding as TG
    from embodiedscan_amd import engine as E
    cfg, det, sd = TG._small_grounder(dev)
    lens = list(lens)
    feats, points, prompts = token_inputs(S_, P_, lens)
    stats = F.Stats(f'shared train {mode}')
    E.PRECISION[0] = mode
    E.DEBUG_OPS = ops = []
    try:
        _begin(det)
        fv = E.Var(feats.to(dev).clone())
        det.loss_shared_from_tokens(fv, points.to(dev), lens, prompts)
        E.TAPE.backward()
        _sync(dev)
    finally:
        E.DEBUG_OPS = None
        E.PRECISION[0] = 'f32'
    n_attn = n_sc = 0
    for r in ops:
        if r['kind'] == 'attn' and r.get('shared'):
            assert r['B'] == 1 and r['klen'] is None and r['bf'] == int(mode == 'bf16') and r['Lq'] == P_ * 32 and r['Lk'] in lens
            assert r['entry'] == 'es_attn_kv_bwd'                   # the decision of DESIGN section 3c
            S.check_attn_bwd(r, dev, stats)
            n_attn += 1
        elif r['kind'] == 'scatter_sum':
            want = SP.scatter_sum_ref(r['dy'].cpu().numpy(), r['idx'].cpu().numpy().reshape(r['P'], r['Q']), r['L'], r['acc'],
                                      r['dx0'].cpu().numpy() if r['acc'] else None)
            assert np.array_equal(SP.bits(r['dx1'].cpu().numpy()), SP.bits(want)), f'{mode}: a scatter_sum record differs from the spec'
            n_sc += 1
    print(stats.report())
    assert n_attn == 2 * S_ and n_sc == S_, (n_attn, n_sc)       # per decoder layer one point cross-attention per scene; one gather per scene
    assert bool(torch.isfinite(fv.g).all())


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_shared_records_in_situ(dev, mode):
    shared_records_in_situ(dev, mode)


# ------------------------------------------------------------------------------------------------------------ model level
def _model_inputs(dev, P_=3):
    from embodiedscan_amd import pipeline
    from embodiedscan_amd.synth import make_grounding_sample, make_scan
    scan = make_scan(41, n_views=2, height=120, width=160, img_size=(128, 128), n_points=6000, n_boxes=8)
    anns = [make_grounding_sample(scan, seed=20 + i) for i in range(P_)]
    assert len({a['text'] for a in anns}) == P_
    return scan, anns, pipeline.upload_scan(scan, dev)


def _step(det, data_fn, shared, force=None):
    """preprocess + loss forward + backward (no optimiser) -> dict(losses, grads, idx, q2g, data)"""
    from embodiedscan_amd import engine as E
    det.force_queries = force
    try:
        _begin(det)
        batch = data_fn()
        points_host = [p.cpu() for p in batch['inputs']['points']]
        data = det.data_preprocessor(batch, True)
        from embodiedscan_amd import hip
        hip.refresh_stream()
        losses = (det.loss_shared if shared else det.loss)(data['inputs'], data['data_samples'])
        out = dict(losses={k: float(v) for k, v in losses.items()}, q2g=[l['q2g'].cpu() for l in det.bbox_head.last],
                   idx=(det.free_queries if force is not None else det.last_queries['idx']).cpu(), data=data, points=points_host)
        det._backward(None)
        torch.cuda.synchronize()
        out['grads'] = {k: v.cpu().clone() for k, v in det.arena.grad_dict().items()}
    finally:
        det.force_queries = None
    return out


def test_train_step_shared_vs_replicated_and_oracle(dev):
    """one synthetic scan (2 views at 120x160, 6 000 points), P = 3, f32: loss_shared against loss on the replicated batch and both against
    the oracle on the replicated batch (teacher-forced queries): losses 1e-3, parameter gradients of backbones, neck, decoder and head
    median 2e-3 / worst 1e-1; two shared runs from the same state are bit-identical; a SceneEncoding built before an optimiser step is
    refused as stale afterwards; unequal P raises ValueError before anything is launched"""
    import test_gpu_grounding as TG
    from embodiedscan_amd import engine as E, hip, pipeline
    from embodiedscan_amd.config import build_optim_wrapper
    from oracle import grounding as OG, model as OM
    P_ = 3
    cfg, det, sd = TG._small_grounder(dev, thr=300)
    scan, anns, dscan = _model_inputs(dev, P_)
    shared_fn = lambda: pipeline.make_shared_grounding_batch([dscan], [anns])
    rep_fn = lambda: pipeline.make_grounding_batch([dscan] * P_, anns)
    free_s, free_r = _step(det, shared_fn, True), _step(det, rep_fn, False)
    print(f'free runs: selected queries of loss_shared equal to the replicated batch\'s: {torch.equal(free_s["idx"], free_r["idx"])} '
          f'(reported: the two batch shapes give tokens that differ by rounding)')
    # oracle on the replicated batch
    names = set(det.arena.grad_dict().keys())
    osd = {k: v.clone().requires_grad_(k in names) for k, v in sd.items()}
    th, tmask = det.last_text['hidden'].float().cpu(), det.last_text['mask'].cpu()
    img = OM.preprocess_img(torch.from_numpy(scan['img']), TG.MEAN, TG.STD)
    gtb = [torch.from_numpy(a['gt_boxes']) for a in anns]
    pms = [ds.gt_instances_3d.positive_maps.cpu() for ds in free_r['data']['data_samples']]
    ol, aux = OG.grounder_loss(osd, free_r['points'], torch.stack([img] * P_), [scan['meta']] * P_, th, tmask, gtb, pms, num_queries=32,
                               num_layers=2, thr=300, return_aux=True)
    sum(ol.values()).backward()
    o = dict(losses={k: float(v.detach()) for k, v in ol.items()}, grads={k: v.grad for k, v in osd.items() if v.grad is not None},
             assign=[torch.stack(list(h['assign'])) for h in aux['head']])
    assert list(det.neck_3d.last['lens']) == [int(f.shape[0]) for f in aux['feats_list']]
    force = aux['idx'].int()
    hs, hr = _step(det, shared_fn, True, force=force), _step(det, rep_fn, False, force=force)
    assert list(det.neck_3d.last['lens']) == [int(aux['feats_list'][0].shape[0])] * P_
    for label, h in (('replicated `loss`', hr), ('loss_shared', hs)):
        for l, a in enumerate(o['assign']):
            assert torch.equal((h['q2g'][l] + 1).long(), a.long()), f'{label}: assignment of layer {l} differs from the oracle\'s'
        for k, w in o['losses'].items():
            e = abs(h['losses'][k] - w) / max(abs(w), 1e-6)
            print(f'{label} {k}: hip {h["losses"][k]:.6f} oracle {w:.6f} rel err {e:.2e} (tol 1e-3)')
            assert e < 1e-3
        skipped = [k for k, g in o['grads'].items() if float(g.norm()) <= SKIP_NORM]
        print(f'{label}: left out (oracle gradient norm <= {SKIP_NORM:g}): {skipped}')
        assert len(skipped) <= SKIP_CAP * len(o['grads'])
        rel = {k: TG._rel(h['grads'][k], g) for k, g in o['grads'].items() if k not in skipped}
        worst = max(rel, key=rel.get)
        med = float(np.median(list(rel.values())))
        print(f'{label} vs oracle: {len(rel)} tensors, median rel-L2 {med:.2e} (tol 2e-3), worst {rel[worst]:.2e} at {worst} (tol 1e-1)')
        assert len(rel) > 100 and med < 2e-3 and rel[worst] < 1e-1
    for k, w in hr['losses'].items():
        assert abs(hs['losses'][k] - w) <= 1e-3 * max(abs(w), 1e-6), (k, hs['losses'][k], w)
    rel = {k: TG._rel(hs['grads'][k], g) for k, g in hr['grads'].items() if float(g.norm()) > SKIP_NORM}
    worst = max(rel, key=rel.get)
    print(f'loss_shared vs replicated `loss`: {len(rel)} tensors, median rel-L2 {float(np.median(list(rel.values()))):.2e} (tol 2e-3), worst '
          f'{rel[worst]:.2e} at {worst} (tol 1e-1)')
    assert float(np.median(list(rel.values()))) < 2e-3 and rel[worst] < 1e-1
    for pre in ('backbone.', 'backbone_3d.', 'neck_3d.', 'decoder.', 'bbox_head.'):
        assert any(k.startswith(pre) for k in rel), pre
    again = _step(det, shared_fn, True, force=force)
    assert all(torch.equal(again['grads'][k], v) for k, v in hs['grads'].items()), 'two loss_shared runs from one state differ'
    # unequal P: refused before anything is launched
    data = pipeline.make_shared_grounding_batch([dscan, dscan], [anns, anns[:2]])
    launches = []
    orig = hip._launch
    hip._launch = lambda name, args: (launches.append(name), orig(name, args))[1]
    try:
        with pytest.raises(ValueError, match='unequal'):
            det.train_step_shared(data, build_optim_wrapper(cfg))
        with pytest.raises(ValueError, match='unequal'):
            det.loss_shared(data['inputs'], data['data_samples'])
    finally:
        hip._launch = orig
    assert launches == [], launches
    # a SceneEncoding built before an optimiser step is stale after it
    data = det.data_preprocessor(pipeline.make_grounding_batch([dscan], anns[:1]), False)
    scene = det.encode_scene(data['inputs'], data['data_samples'])[0]
    assert len(det.ground(scene, [anns[0]['text']])) == 1
    losses = det.train_step_shared(shared_fn(), build_optim_wrapper(cfg))
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in losses.values())
    with pytest.raises(ValueError, match='stale'):
        det.ground(scene, [anns[0]['text']])
