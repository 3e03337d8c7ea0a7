"""One scene, many prompts (SparseFeatureFusion3DGrounder.encode_scene / scene_from_tokens / ground) and the kernels under it.

Kernel level: es_contrastive_shared_fwd is held to fwd_spec.check_contrastive on the replicated record (B = P, the rows repeated) and,
on top of that, must equal es_contrastive_fwd on v.repeat(P, 1) bit for bit; es_attn_kv_prepare + es_attn_kv_fwd are held to
fwd_spec.check_attention with B = 1 on column slices of wider buffers, in both matrix-core modes, with the operand image poisoned
before `prepare` (the result must not depend on what the padding held).  The issue's shape grid is kept as stated; the kernels' own
tile edges are added to it (the contrastive kernel has no grid-stride loop: a workgroup owns 32 consecutive rows, so L = 1029 =
32 * 32 + 5 ends on a partial workgroup and a partial wave; the attention kernel works on 128 query rows x 64 keys, so Lq in
{128, 129, 257} and Lk in {64, 65, 130} join the grid).
Decoder level: ground() on scene_from_tokens() against oracle/grounding.py per prompt (same tokens, the text hidden states the
device produced): selected queries equal, last-layer boxes 1e-4 relative L2, scores 1e-3 -- the bounds tests/test_gpu_grounding.py
holds the batched path to.  Precondition, asserted on the oracle's values alone: the oracle's sorted row maxima are further apart
than twice the contrastive bound of check_contrastive at every rank up to the (Q+1)-th (the indices are compared IN ORDER, so every
rank counts, not only the last).  The same call runs under engine.DEBUG_FWD in f32 and bf16: every record of the two new kinds is
checked in situ (the only bf16 bound).
Model level (GPU only): encode_scene + ground against predict on replicated samples.

Every body is a function of `dev`; tests/test_emu_shared_scene.py runs them on the CPU emulator on a reduced grid."""
import math

import pytest
import torch

import fwd_spec as F
import ground_spec as S
import test_gpu_ground_kernels as K

pytestmark = pytest.mark.gpu

SENT = K.SENT
PROMPTS = ['find the chair', 'the lamp next to the window on the left side of the door', 'a table', 'find the red sofa in the room that is close to the wall',
           'where is the other chair and the small shelf']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------------------ contrastive, shared
def contrastive_shared_case(dev, stats, L, P_, T, C, Tout, tlen, seed):
    hip = K._hip()
    P = hip.P
    g = torch.Generator().manual_seed(seed)
    v, text = torch.randn(L, C, generator=g), torch.randn(P_, T, C, generator=g)
    bias = torch.tensor([-4.6])
    tl = torch.tensor(tlen, dtype=torch.int32)
    vd, td, bd, tld = v.to(dev), text.to(dev), bias.to(dev), tl.to(dev)
    lo, lobuf = K._flat(dev, torch.zeros(P_, L, Tout))
    rm, rmbuf = K._flat(dev, torch.zeros(P_, L))
    st = K._st()
    hip.call('es_contrastive_shared_fwd', P(vd), L, P(td), P_, T, C, P(tld), P(bd), P(lo), Tout, P(rm), st)
    rm2, rm2buf = K._flat(dev, torch.zeros(P_, L))
    hip.call('es_contrastive_shared_fwd', P(vd), L, P(td), P_, T, C, P(tld), P(bd), 0, Tout, P(rm2), st)      # logits NULL
    # HIP against HIP: the composition it replaces, on P copies of the rows
    vrep = vd.repeat(P_, 1).contiguous()
    lo_r, rm_r = torch.zeros(P_, L, Tout, device=dev), torch.zeros(P_, L, device=dev)
    hip.call('es_contrastive_fwd', P(vrep), P_, L, P(td), T, C, P(tld), 0, P(bd), P(lo_r), Tout, P(rm_r), st)
    torch.cuda.synchronize()
    label = f'contrastive shared L={L} P={P_} T={T} C={C} Tout={Tout} tlen={tlen}'
    for buf, n in ((lobuf, P_ * L * Tout), (rmbuf, P_ * L), (rm2buf, P_ * L)):
        K._tail_ok(buf, n, label)
    m = min(T, Tout)
    assert bool(torch.isneginf(lo[:, :, m:]).all()), f'{label}: columns beyond T are not -inf'
    lo_T = torch.full((P_, L, T), -math.inf, device=dev)
    lo_T[:, :, :m] = lo[:, :, :m]
    F.check_contrastive(dict(B=P_, L=L, T=T, v=vrep, text=td.view(P_ * T, C), bias=bd, tlen=tl.clamp(max=m), vlen=None, logits=lo_T, rowmax=rm),
                        dev, stats)
    for p, t in enumerate(tlen):
        if t == 0:
            assert bool(torch.isneginf(lo[p]).all()) and bool(torch.isneginf(rm[p]).all()), f'{label}: tlen = 0 must give a row of -inf'
    assert torch.equal(lo, lo_r) and torch.equal(rm, rm_r), f'{label}: not bit-identical to es_contrastive_fwd on the replicated rows'
    assert torch.equal(rm, rm2), f'{label}: rowmax depends on whether logits are written'


def contrastive_shared_grid(dev):
    """(L, P, C, Tout, tlen): every (L, P, C) of the issue at T = 7, Tout = T; Tout < T and Tout > T once each.  Emulator: L = 1029
    at (P, C) = (2, 64) and (1, 320) only"""
    cases, i = [], 0
    pool = (0, 1, 3, 7)
    for L in (1, 3, 4, 5, 1029):
        for P_ in (1, 2, 5):
            for C in (64, 256, 320):
                if K._small(dev) and L == 1029 and (P_, C) not in ((2, 64), (1, 320)):
                    continue
                cases.append((L, P_, C, 7, [pool[(i + p) % 4] for p in range(P_)]))
                i += 1
    cases.append((5, 2, 256, 5, [7, 3]))
    cases.append((33, 5, 64, 9, [7, 0, 1, 3, 7]))
    assert {t for c in cases for t in c[4]} == set(pool)
    return cases


def test_contrastive_shared_on_the_shape_grid(dev):
    stats = F.Stats('contrastive shared grid')
    for i, (L, P_, C, Tout, tlen) in enumerate(contrastive_shared_grid(dev)):
        contrastive_shared_case(dev, stats, L, P_, 7, C, Tout, tlen, 700 + i)
    print(stats.report())


def test_contrastive_shared_refusals_leave_the_outputs_untouched(dev):
    """C = 513 and a text block beyond the LDS return -4 and write nothing"""
    P = K._hip().P
    for C, T in ((513, 3), (64, K._tmax(64) + 1), (512, K._tmax(512) + 1)):
        L, P_ = 3, 2
        t = lambda *s: torch.full(s, SENT, device=dev)
        v, text, lo, rm = t(L, C), t(P_, T, C), t(P_, L, T), t(P_, L)
        tl = torch.tensor([T, T], dtype=torch.int32, device=dev)
        assert K._rc('es_contrastive_shared_fwd', P(v), L, P(text), P_, T, C, P(tl), 0, P(lo), T, P(rm), K._st()) == -4
        torch.cuda.synchronize()
        assert bool((lo == SENT).all()) and bool((rm == SENT).all())


# ------------------------------------------------------------------------------------------------------------ attention, prepared
def attn_kv_case(dev, stats, bf, regime, H, Lq, Lk, seed):
    """es_attn_kv_prepare + es_attn_kv_fwd on column slices, the operand image poisoned two different ways before `prepare`"""
    hip = K._hip()
    P = hip.P
    E = H * 32
    q, k, v, _ = K.attn_inputs(regime, 1, H, Lq, Lk, seed)
    Q, Kc, Vc = (K.Cols(dev, r, E, ld, off, t) for (r, ld, off, t) in ((Lq, E + 8, 4, q), (Lk, E + 4, 0, k), (Lk, E + 12, 8, v)))
    nbytes = int(hip.raw('es_attn_kv_bytes')(H, Lk, bf))
    assert nbytes == H * ((Lk + 63) // 64) * 4096 * (2 if bf else 4)
    st = K._st()
    outs = []
    for poison in (0xFF, 0x4B):                        # (all-ones: NaN in either operand type; 0x4B4B..: large finite values)
        kv = torch.full((nbytes + 16,), poison, dtype=torch.uint8, device=dev)
        O = K.Cols(dev, Lq, E, E + 16, 8)
        lse, lse_buf = K._flat(dev, torch.zeros(H * Lq))
        hip.call('es_attn_kv_prepare', Kc.ptr(), Kc.ld, Vc.ptr(), Vc.ld, H, Lk, bf, P(kv), st)
        hip.call('es_attn_kv_fwd', Q.ptr(), Q.ld, P(kv), H, Lq, Lk, O.ptr(), O.ld, P(lse), bf, st)
        torch.cuda.synchronize()
        label = f'attention kv {regime} bf16={bf} H={H} Lq={Lq} Lk={Lk} poison={poison:#x}'
        assert bool((kv[nbytes:] == poison).all()), f'{label}: prepare wrote past the operand image'
        O.untouched_outside(label)
        K._tail_ok(lse_buf, H * Lq, label + ' lse')
        F.check_attention(dict(B=1, H=H, Lq=Lq, Lk=Lk, bf=bf, q=Q.v, k=Kc.v, v=Vc.v, klen=None, o=O.v, lse=lse), dev, stats)
        outs.append((kv[:nbytes].clone(), O.v.clone(), lse.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b), f'{label}: the result depends on what the operand image held before prepare'


ISSUE_LQ, ISSUE_LK = (1, 63, 64, 65, 99), (1, 31, 32, 33, 97)      # 99 = 3 prompts x 33 queries: a tile spans two prompts
OWN_EDGES = ((128, 64), (129, 65), (257, 130), (127, 63))           # (Lq, Lk) at the 128-row / 64-key tiles of this kernel


def attn_kv_grid(dev):
    """(bf, regime, H, Lq, Lk).  GPU: every (H, Lq, Lk) of the issue in both modes, regimes rotating, + the kernel's own edges at
    H in {1, 8}.  Emulator: every Lq and every Lk at least twice per mode over H in {1, 2}, + the own edges at H = 1"""
    cases, i = [], 0
    if not K._small(dev):
        for H in (1, 2, 8):
            for Lq in ISSUE_LQ:
                for Lk in ISSUE_LK:
                    for bf in (0, 1):
                        cases.append((bf, K.REGIMES[i % 3], H, Lq, Lk))
                        i += 1
        for Lq, Lk in OWN_EDGES:
            for H in (1, 8):
                for bf in (0, 1):
                    cases.append((bf, K.REGIMES[i % 3], H, Lq, Lk))
                    i += 1
        return cases
    for n in range(10):
        Lq, Lk = ISSUE_LQ[n % 5], ISSUE_LK[(n + n // 5) % 5]
        for bf in (0, 1):
            cases.append((bf, K.REGIMES[(n + bf) % 3], 1 + (n + bf) % 2, Lq, Lk))
    for n, (Lq, Lk) in enumerate(OWN_EDGES):
        for bf in (0, 1):
            cases.append((bf, K.REGIMES[(n + bf) % 3], 1, Lq, Lk))
    return cases


def test_attention_kv_on_the_tile_edge_grid(dev):
    stats = F.Stats('attention kv grid')
    for n, (bf, regime, H, Lq, Lk) in enumerate(attn_kv_grid(dev)):
        attn_kv_case(dev, stats, bf, regime, H, Lq, Lk, 800 + n)
    print(stats.report())


def test_attention_kv_reference_alone_meets_the_bounds():
    """the f32 torch evaluation of the formula (ground_spec.attn_ref, B = 1, no key mask) passes check_attention at the shapes of this
    file in all regimes and both modes: the bound is one the reference itself meets (CPU only: no kernel is looked at)"""
    dev = torch.device('cpu')
    stats = F.Stats('attention kv reference')
    for n, regime in enumerate(K.REGIMES):
        for bf in (0, 1):
            for (H, Lq, Lk) in ((2, 99, 97), (1, 65, 33), (8, 1, 31), (1, 257, 130)):
                q, k, v, do = K.attn_inputs(regime, 1, H, Lq, Lk, 17 + n)
                r = S.attn_ref(q, k, v, do, None, 1, H, Lq, Lk, bf)
                F.check_attention(dict(B=1, H=H, Lq=Lq, Lk=Lk, bf=bf, q=q, k=k, v=v, klen=None, o=r['o'], lse=r['lse'].reshape(-1)), dev, stats)
    print(stats.report())


def test_attention_kv_refuses_unaligned_leading_dimensions(dev):
    """an ld that is not a multiple of 4 returns -3 and nothing is written"""
    hip = K._hip()
    P = hip.P
    H, Lq, Lk = 1, 5, 7
    t = lambda n: torch.full((n, 40), SENT, device=dev)
    q, k, v, o = t(Lq), t(Lk), t(Lk), t(Lq)
    lse = torch.full((Lq,), SENT, device=dev)
    nbytes = int(hip.raw('es_attn_kv_bytes')(H, Lk, 1))
    kv = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    for ldk, ldv in ((34, 36), (36, 37)):
        assert K._rc('es_attn_kv_prepare', P(k), ldk, P(v), ldv, H, Lk, 1, P(kv), K._st()) == -3
    for ldq, ldo in ((34, 36), (36, 35)):
        assert K._rc('es_attn_kv_fwd', P(q), ldq, P(kv), H, Lq, Lk, P(o), ldo, P(lse), 1, K._st()) == -3
    torch.cuda.synchronize()
    assert bool((kv == 0x5A).all()) and bool((o == SENT).all()) and bool((lse == SENT).all())


# ------------------------------------------------------------------------------------------------------------ decoder level
TOKEN_SEED = 23         # searched over 0 .. 59: the widest margin of the precondition below over both coders, both L and all prompts (3.4 x)


def _tokens(L, seed=TOKEN_SEED):
    g = torch.Generator().manual_seed(seed * 1000 + L)
    return torch.randn(L, 256, generator=g), torch.rand(L, 3, generator=g) * 4.0 - 2.0


def _contrastive_gap_precondition(label, feats, text, mask, bias, Q):
    """on the ORACLE's values alone: the sorted row maxima of this prompt are further apart than twice the per-element bound of
    check_contrastive at every rank up to the (Q+1)-th, so neither the selected set nor its order can legitimately differ"""
    v, t = feats.double(), text.double()[mask]
    C = v.shape[1]
    inv = 1.0 / math.sqrt(C)
    dot, A = v @ t.T, v.abs() @ t.abs().T
    bound = float((F.G * F.U * math.sqrt(C) * A * inv + F.U * (2 * dot.abs() * inv + abs(float(bias)))).max())
    sc = torch.sort((dot * inv + float(bias)).amax(-1), descending=True)[0][:Q + 1]
    gap = float((sc[:-1] - sc[1:]).min()) if sc.numel() > 1 else math.inf
    print(f'{label}: smallest gap between consecutive row maxima up to rank Q+1 = {gap:.3e}, contrastive bound {bound:.3e} (ratio {gap / (2 * bound):.1f})')
    assert gap > 2 * bound, f'{label}: the token seed gives a near tie in the oracle\'s query selection: choose another TOKEN_SEED'


def ground_vs_oracle(dev, config, Ls=(20, 150)):
    """f32: ground() with 5 prompts in chunks of 2 on scene_from_tokens(L tokens) against the oracle, per prompt"""
    import torch.nn.functional as TF
    import test_gpu_grounding as TG
    from embodiedscan_amd import engine as E
    from oracle import grounding as OG
    cfg, det, sd = TG._small_grounder(dev, config=config)
    coder = det.bbox_head.box_coder
    assert E.PRECISION[0] == 'f32'
    for L in Ls:
        feats, points = _tokens(L)
        scene = det.scene_from_tokens(feats.to(dev), points.to(dev))
        assert scene.L == L and len(scene.keys) == 2
        res = det.ground(scene, PROMPTS, max_prompts=2)
        torch.cuda.synchronize()
        Q = min(32, L)
        assert len(res) == len(PROMPTS) and len(det.last_text_chunks) == 3
        idx = det.last_queries['idx'].cpu()
        for i in range(len(PROMPTS)):
            lt = det.last_text_chunks[i // 2]
            th, tm = lt['hidden'][i % 2].float().cpu()[None], lt['mask'][i % 2].cpu()[None]
            text = TF.linear(th, sd['text_feat_map.weight'], sd['text_feat_map.bias'])
            label = f'{coder} L={L} prompt {i} ({int(tm.sum())} tokens)'
            _contrastive_gap_precondition(label, feats, text[0], tm[0], sd['bbox_head.cls_branches.0.bias'], Q)
            with torch.no_grad():
                hid, boxes, aux = OG.forward_transformer([feats], [points], text, tm, sd, num_queries=32, num_layers=2, training=False, coder=coder)
                want = torch.sigmoid(OG.contrastive_embed(hid[-1], text, tm, sd['bbox_head.cls_branches.0.bias']).max(-1)[0])[0]
            assert torch.equal(idx[i].long(), aux['idx'][0]), f'{label}: selected queries differ from the oracle\'s'
            r = res[i]
            assert tuple(r.bboxes_3d.tensor.shape) == (Q, 9) and tuple(r.scores_3d.shape) == (Q,) and torch.equal(r.target_scores_3d, r.scores_3d)
            eb = TG._rel(r.bboxes_3d.tensor.cpu(), boxes[-1][0])
            es = float((r.scores_3d.cpu() - want).abs().max())
            print(f'{label}: last-layer boxes rel-L2 {eb:.2e} (tol 1e-4), scores max |err| {es:.2e} (tol 1e-3)')
            assert eb < 1e-4 and es < 1e-3 and TG._rel(r.scores_3d.cpu(), want) < 1e-3
    return det


def test_ground_on_tokens_vs_oracle_baseline_coder(dev):
    ground_vs_oracle(dev, 'mv_grounding.py')


def test_ground_on_tokens_vs_oracle_fcaf_coder(dev):
    ground_vs_oracle(dev, 'mv_grounding_fcaf.py')


NEW_ENTRIES = ('es_attn_kv_fwd', 'es_contrastive_shared_fwd')


def ground_records_in_situ(dev, mode, L=150):
    """the same call under engine.DEBUG_FWD: every record of the two new kinds passes its checker on the spot"""
    import test_gpu_grounding as TG
    from embodiedscan_amd import engine as E
    cfg, det, sd = TG._small_grounder(dev)
    stats = F.Stats(f'ground {mode}')

    def on_record(rec):
        if rec['entry'] in NEW_ENTRIES:
            F.check(rec, dev, stats)
    feats, points = _tokens(L)
    E.PRECISION[0] = mode
    E.DEBUG_FWD = on_record
    try:
        scene = det.scene_from_tokens(feats.to(dev), points.to(dev))
        res = det.ground(scene, PROMPTS, max_prompts=2)
        torch.cuda.synchronize()
    finally:
        E.DEBUG_FWD = None
        E.PRECISION[0] = 'f32'
    print(stats.report())
    # 3 chunks: one query-selection launch each, one point cross-attention per decoder layer each
    assert stats.count == {'es_attn_kv_fwd': 6, 'es_contrastive_shared_fwd': 3}, stats.count
    assert all(bool(torch.isfinite(r.bboxes_3d.tensor).all()) for r in res)


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_ground_records_in_situ(dev, mode):
    ground_records_in_situ(dev, mode)


# ------------------------------------------------------------------------------------------------------------ staleness and edges
def staleness_and_edges(dev):
    import test_gpu_grounding as TG
    from embodiedscan_amd import engine as E
    cfg, det, sd = TG._small_grounder(dev)
    feats, points = _tokens(40)
    fd, pd = feats.to(dev), points.to(dev)
    scene = det.scene_from_tokens(fd, pd)
    first = det.ground(scene, PROMPTS[:2])
    assert det.ground(scene, []) == []
    det.load_state_dict({k: v.to(dev) for k, v in sd.items()})
    with pytest.raises(ValueError, match='stale'):
        det.ground(scene, PROMPTS[:2])
    scene = det.scene_from_tokens(fd, pd)                  # rebuilt: works, and (same weights) gives the same answer
    again = det.ground(scene, PROMPTS[:2])
    assert all(torch.equal(a.bboxes_3d.tensor, b.bboxes_3d.tensor) and torch.equal(a.scores_3d, b.scores_3d) for a, b in zip(first, again))
    E.PRECISION[0] = 'bf16'
    try:
        with pytest.raises(ValueError, match='stale'):
            det.ground(scene, PROMPTS[:2])
        scene16 = det.scene_from_tokens(fd, pd)
        r16 = det.ground(scene16, PROMPTS[:2])
        assert len(r16) == 2 and bool(torch.isfinite(r16[0].bboxes_3d.tensor).all())
    finally:
        E.PRECISION[0] = 'f32'
    with pytest.raises(ValueError, match='stale'):
        det.ground(scene16, PROMPTS[:2])
    if dev.type == 'cuda':
        scene.feats = scene.feats.cpu()
        with pytest.raises(ValueError, match='is on'):
            det.ground(scene, PROMPTS[:2])
    return det


def empty_scene(dev, det):
    scene = det.scene_from_tokens(torch.zeros(0, 256, device=dev), torch.zeros(0, 3, device=dev))
    assert scene.L == 0
    res = det.ground(scene, PROMPTS[:3])
    assert len(res) == 3
    for r in res:
        assert tuple(r.bboxes_3d.tensor.shape) == (0, 9) and tuple(r.scores_3d.shape) == (0,) and tuple(r.target_scores_3d.shape) == (0,)


def test_stale_encodings_are_refused_and_the_edges(dev):
    det = staleness_and_edges(dev)
    empty_scene(dev, det)


# ------------------------------------------------------------------------------------------------------------ model level
def test_encode_scene_and_ground_vs_predict_on_replicated_samples(dev):
    """encode_scene on a two-scan batch, ground with four prompts on scene 0 (teacher-forced to the query indices predict selected)
    against predict on four samples that replicate scan 0 with those prompts.  The backbones run on different batch shapes on the two
    sides, so bit equality is not asked: tokens 1e-5 relative L2, boxes 1e-4, scores 1e-3."""
    import test_gpu_grounding as TG
    from embodiedscan_amd import pipeline
    from embodiedscan_amd.synth import make_grounding_sample
    cfg, det, sd = TG._small_grounder(dev)
    scans, anns, dscans = TG._grounding_batch(dev)
    prompts = [make_grounding_sample(scans[0], seed=10 + i) for i in range(4)]
    assert len({p['text'] for p in prompts}) == 4
    data = det.data_preprocessor(pipeline.make_grounding_batch([dscans[0]] * 4, prompts), False)
    out = det.forward(data['inputs'], data['data_samples'], mode='predict')
    nk = det.neck_3d.last
    L, Lmax = nk['lens'][0], nk['Lmax']
    assert list(nk['lens']) == [L] * 4
    ref_feats = nk['feats'].d[:L].clone()
    forced = det.last_queries['idx'].clone()
    want = [(s.pred_instances_3d.bboxes_3d.tensor.clone(), s.pred_instances_3d.scores_3d.clone()) for s in out]
    data2 = det.data_preprocessor(pipeline.make_grounding_batch(dscans, anns), False)
    scenes = det.encode_scene(data2['inputs'], data2['data_samples'])
    assert len(scenes) == 2 and scenes[0].L == L
    ef = TG._rel(scenes[0].feats, ref_feats)
    print(f'scene 0: {L} tokens, rel-L2 against the replicated batch\'s rows {ef:.2e} (tol 1e-5)')
    assert ef < 1e-5
    det.force_queries = forced
    try:
        res = det.ground(scenes[0], [p['text'] for p in prompts], tokens_positive=[p['tokens_positive'] for p in prompts])
    finally:
        det.force_queries = None
    torch.cuda.synchronize()
    print(f'free query selection equal to predict\'s: {torch.equal(det.free_queries.cpu(), forced.cpu())} (reported, not gated: the tokens differ by ~1e-6)')
    for i, (r, (wb, ws)) in enumerate(zip(res, want)):
        eb, es = TG._rel(r.bboxes_3d.tensor, wb), float((r.scores_3d - ws).abs().max())
        print(f'prompt {i}: boxes rel-L2 {eb:.2e} (tol 1e-4), scores max |err| {es:.2e} (tol 1e-3)')
        assert eb < 1e-4 and es < 1e-3
