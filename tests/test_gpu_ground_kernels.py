"""The grounding kernels (csrc/transformer.hip, csrc/ground.hip) held to the f64 specifications of tests/ground_spec.py and
tests/fwd_spec.py at every shape edge: attention forward / backward on both matrix-core modes over the query / key tile edges, every
kind of key length and three softmax regimes (N(0,1); peaked, max |S| = 25; ascending, the row maximum rises at every 32-key step so
that the online-softmax rescale matters); LayerNorm and ContrastiveEmbed forward / backward over C and n edges, NULL outputs, the
> 64 KiB LDS branch and the refusals; both box coders at the clamp; the focal loss at logits up to +-30; the assignment through both
solvers on heavily tied costs; the sorted top-k through its dynamic-LDS branch; the oriented-box IoU at rotations by multiples of
pi / 2.  Operands are column slices of wider buffers that hold a sentinel everywhere else; the sentinel must survive.

Every body is a function of `dev`: tests/test_emu_ground_kernels.py runs the same bodies on the CPU emulator (dev.type == 'cpu'
selects the reduced grid there: B <= 2, H <= 2, L <= 130, every tile edge kept).  Each body prints the worst bound ratio per class."""
import math

import numpy as np
import pytest
import torch

import ground_spec as S

pytestmark = pytest.mark.gpu

SENT = -7.25e5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _hip():
    from embodiedscan_amd import hip
    return hip


def _rc(name, *args):
    """the status an entry point returns (hip.call raises on anything but 0)"""
    return _hip().raw(name)(*args)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _small(dev):
    return dev.type == 'cpu'


class Cols:
    """a (rows, C) f32 view at column `off` of a (rows, ld) buffer that holds SENT everywhere else (and 8 floats past its end)"""

    def __init__(self, dev, rows, C, ld, off, init=None):
        assert off + C <= ld
        self.rows, self.C, self.ld, self.off = rows, C, ld, off
        self.buf = torch.full((rows * ld + 8,), SENT, dtype=torch.float32, device=dev)
        self.v = self._view(self.buf)
        if init is not None:
            self.v.copy_(init)

    def _view(self, b):
        return b[:self.rows * self.ld].view(self.rows, self.ld)[:, self.off:self.off + self.C]

    def ptr(self):
        return self.v.data_ptr()

    def untouched_outside(self, label):
        b = self.buf.clone()
        self._view(b).fill_(SENT)
        assert bool((b == SENT).all()), f'{label}: a launch wrote outside the ({self.rows}, {self.C}) view (ld {self.ld}, column {self.off})'


def _flat(dev, t, pad=8):
    """a contiguous copy of t followed by `pad` sentinels; returns (view, whole buffer)"""
    buf = torch.full((t.numel() + pad,), SENT, dtype=t.dtype, device=dev)
    buf[:t.numel()] = t.reshape(-1).to(dev)
    return buf[:t.numel()].view(t.shape), buf


def _tail_ok(buf, n, label):
    assert bool((buf[n:] == SENT).all()), f'{label}: a launch wrote past the end of its output'


# ------------------------------------------------------------------------------------------------------------------ attention
def attn_inputs(regime, B, H, Lq, Lk, seed):
    """q, k, v, dO as (B L, H 32) host tensors.  'normal': N(0,1).  'peaked': q scaled so that max |S| = 25.  'ascending': keys and
    queries share a +-1 direction per head and key j carries it j / 32 times, so S rises by ~3 per 32-key step in every row"""
    g = torch.Generator().manual_seed(seed)
    E = H * 32
    q, k = torch.randn(B * Lq, E, generator=g), torch.randn(B * Lk, E, generator=g)
    v, do = torch.randn(B * Lk, E, generator=g), torch.randn(B * Lq, E, generator=g)
    if regime == 'peaked':
        Sm = (S._heads(q.double() * S.S32, B, Lq, H) @ S._heads(k.double(), B, Lk, H).transpose(-1, -2)).abs().max()
        q = q * float(25.0 / Sm)
    elif regime == 'ascending':
        d = (torch.randint(0, 2, (1, E), generator=g) * 2 - 1).float()
        a = math.sqrt(3.0 / math.sqrt(32.0))
        j = (torch.arange(B * Lk) % Lk).float()[:, None]
        k = d * a * (j / 32.0) + 0.02 * k                        # (small enough that even a one-key last step tops its predecessor)
        q = d * a + 0.1 * q
    return q, k, v, do


def _klens(Lk, B, i):
    """the i-th choice of key lengths for a (Lk, B) case: None; all Lk; beyond Lk (clamped); ragged down to 1; ends on / one past a
    32-key step and a 64-key workgroup"""
    edges = [e for e in (1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, Lk - 1, Lk) if 1 <= e <= Lk]
    kinds = [None, [Lk] * B, [Lk + 7] + [Lk] * (B - 1), [edges[(i + b * 3) % len(edges)] for b in range(B)],
             [1] + [edges[(i + b) % len(edges)] for b in range(1, B)]]
    return kinds[i % len(kinds)]


def attn_case(dev, stats, bf, regime, B, H, Lq, Lk, klen, acc, seed, check_ascending=True):
    """one es_attn_fwd + es_attn_bwd pair on column slices with eight different leading dimensions; returns the records"""
    hip = _hip()
    P = hip.P
    E = H * 32
    q, k, v, do = attn_inputs(regime, B, H, Lq, Lk, seed)
    kl = None if klen is None else torch.tensor(klen, dtype=torch.int32, device=dev)
    lds = [E + 4 * (i + 1) for i in range(8)]
    Q, K, V, DO = (Cols(dev, r, E, ld, off, t) for (r, ld, off, t) in
                   ((B * Lq, lds[0], 4, q), (B * Lk, lds[1], 0, k), (B * Lk, lds[2], 8, v), (B * Lq, lds[3], 4, do)))
    O = Cols(dev, B * Lq, E, lds[4], 8)
    g = torch.Generator().manual_seed(seed + 1)
    pri = [torch.randn(n, E, generator=g) for n in (B * Lq, B * Lk, B * Lk)]
    DQ, DK, DV = (Cols(dev, r, E, ld, off, t) for (r, ld, off, t) in
                  ((B * Lq, lds[5], 0, pri[0]), (B * Lk, lds[6], 12, pri[1]), (B * Lk, lds[7], 4, pri[2])))
    lse, lse_buf = _flat(dev, torch.zeros(B * H * Lq))
    delta, delta_buf = _flat(dev, torch.zeros(B * H * Lq))
    st = _st()
    hip.call('es_attn_fwd', Q.ptr(), Q.ld, K.ptr(), K.ld, V.ptr(), V.ld, B, H, Lq, Lk, P(kl), O.ptr(), O.ld, P(lse), bf, st)
    hip.call('es_attn_bwd', Q.ptr(), Q.ld, K.ptr(), K.ld, V.ptr(), V.ld, O.ptr(), O.ld, DO.ptr(), DO.ld, P(lse), B, H, Lq, Lk, P(kl),
             P(delta), DQ.ptr(), DQ.ld, DK.ptr(), DK.ld, DV.ptr(), DV.ld, acc, bf, st)
    torch.cuda.synchronize()
    label = f'attention {regime} bf16={bf} B={B} H={H} Lq={Lq} Lk={Lk} klen={klen}'
    for c in (O, DQ, DK, DV):
        c.untouched_outside(label)
    _tail_ok(lse_buf, B * H * Lq, label + ' lse')
    _tail_ok(delta_buf, B * H * Lq, label + ' delta')
    fwd = dict(B=B, H=H, Lq=Lq, Lk=Lk, bf=bf, q=Q.v, k=K.v, v=V.v, klen=kl, o=O.v, lse=lse)
    S.check_attention(fwd, dev, stats)
    bwd = dict(fwd, do=DO.v, acc=acc, dq=DQ.v, dk=DK.v, dv=DV.v, dq0=pri[0], dk0=pri[1], dv0=pri[2])
    S.check_attn_bwd(bwd, dev, stats)
    if regime == 'ascending' and check_ascending and Lk > 32:
        kls = [Lk] * B if klen is None else [min(x, Lk) for x in klen]
        Sc = (S._heads(Q.v.double().cpu() * S.S32, B, Lq, H) @ S._heads(K.v.double().cpu(), B, Lk, H).transpose(-1, -2))
        for b in range(B):
            steps = [Sc[b, :, :, s:min(s + 32, kls[b])].amax(-1) for s in range(0, kls[b], 32)]
            for s0, s1 in zip(steps, steps[1:]):
                assert bool((s1 > s0).all()), f'{label}: the row maximum does not rise at every 32-key step'
    return fwd, bwd


LQ = (1, 63, 64, 65, 129)
LK = (1, 31, 32, 33, 64, 65, 150)
REGIMES = ('normal', 'peaked', 'ascending')


def attn_grid(dev):
    """(bf, regime, B, H, Lq, Lk, klen, acc) cases.  GPU: every (Lq, Lk) pair in both modes and all three regimes, H in {1, 8} and accumulate on independent strides,
    B = 3.  Emulator: every Lq and every Lk edge (Lk 150 -> 130) at least twice, both modes, regimes and H in {1, 2} rotating, B = 2."""
    cases, i = [], 0
    if not _small(dev):
        for Lq in LQ:
            for Lk in LK:
                for bf in (0, 1):
                    for regime in REGIMES:
                        # H, accumulate and the key-length kind advance on strides coprime with the 6 (mode, regime) pairs and with
                        # one another (5, 2 x 7 halves, 5 kinds offset by i // 6), so that every combination below does occur
                        H, acc = (8 if i % 5 in (0, 2) else 1), int(i % 7 < 3)
                        cases.append((bf, regime, 3, H, Lq, Lk, _klens(Lk, 3, i + i // 6), acc))
                        i += 1
        seen = {(c[0], c[1], c[3], c[7]) for c in cases}
        assert len(seen) == 24, 'every (mode, regime, H, accumulate) combination must occur in the attention grid'
        return cases
    pairs = ((1, 1), (63, 31), (64, 32), (65, 33), (129, 64), (65, 65), (64, 130), (1, 33), (129, 31), (63, 65), (1, 130), (65, 32), (64, 64),
             (63, 1))
    for n, (Lq, Lk) in enumerate(pairs):
        for bf in (0, 1):
            cases.append((bf, REGIMES[(n + bf) % 3], 2, 1 + (n + bf) % 2, Lq, Lk, _klens(Lk, 2, i), i % 2))
            i += 1
    return cases


def test_attention_fwd_bwd_on_the_tile_edge_grid(dev):
    stats = S.Stats('attention grid')
    for n, (bf, regime, B, H, Lq, Lk, klen, acc) in enumerate(attn_grid(dev)):
        attn_case(dev, stats, bf, regime, B, H, Lq, Lk, klen, acc, 100 + n)
    print(stats.report())
    assert {c.split()[1] for c in stats.ratio if c.startswith('attn_bwd')} == {'dq', 'dk', 'dv'}


def test_attention_reference_alone_meets_the_bounds():
    """the f32 torch evaluation of the specification's formula passes both checkers in all three regimes and both modes: the error
    model is not tighter than f32 arithmetic on the same roundings (CPU only: no kernel is looked at)"""
    dev = torch.device('cpu')
    stats = S.Stats('attention reference')
    for n, regime in enumerate(REGIMES):
        for bf in (0, 1):
            for (B, H, Lq, Lk, klen) in ((2, 2, 65, 130, [130, 37]), (1, 1, 129, 33, None), (2, 1, 1, 65, [1, 64])):
                q, k, v, do = attn_inputs(regime, B, H, Lq, Lk, 7 + n)
                kl = None if klen is None else torch.tensor(klen, dtype=torch.int32)
                r = S.attn_ref(q, k, v, do, kl, B, H, Lq, Lk, bf)
                rec = dict(B=B, H=H, Lq=Lq, Lk=Lk, bf=bf, q=q, k=k, v=v, klen=kl, o=r['o'], lse=r['lse'].reshape(-1))
                S.check_attention(rec, dev, stats)
                S.check_attn_bwd(dict(rec, do=do, acc=0, dq=r['dq'], dk=r['dk'], dv=r['dv']), dev, stats)
    print(stats.report())


def test_attention_sample_without_valid_keys(dev):
    """klen[b] <= 0: O = 0, lse = -inf, dQ / dK / dV exact zeros (accumulate = 0) or the untouched prior (accumulate = 1) for that
    sample; its neighbours in the batch are held to the specification as usual.  (Before the fix the forward wrote 0 * (1 / 0) = NaN.)"""
    stats = S.Stats('attention without keys')
    for bf in (0, 1):
        for acc in (0, 1):
            for klen in ([0, 40, 70], [33, -2, 0]):
                fwd, bwd = attn_case(dev, stats, bf, 'normal', 3, 2, 65, 70, klen, acc, 900 + bf)
                for b, kl in enumerate(klen):
                    if kl <= 0:
                        assert bool((fwd['o'][b * 65:(b + 1) * 65] == 0).all()) and bool(torch.isneginf(fwd['lse'].view(3, 2, 65)[b]).all())
                        for nm, L in (('dq', 65), ('dk', 70), ('dv', 70)):
                            got = bwd[nm][b * L:(b + 1) * L].cpu()
                            assert torch.equal(got, bwd[nm + '0'][b * L:(b + 1) * L] if acc else torch.zeros_like(got)), (nm, klen, acc)
    print(stats.report())


def test_attention_refuses_unaligned_leading_dimensions(dev):
    """an ld that is not a multiple of 4 returns -3 and nothing is written"""
    P = _hip().P
    B, H, Lq, Lk, E = 1, 1, 5, 7, 32
    t = lambda n: torch.full((n, 40), SENT, device=dev)
    q, k, v, o, do, dq, dk, dv = t(Lq), t(Lk), t(Lk), t(Lq), t(Lq), t(Lq), t(Lk), t(Lk)
    lse, delta = torch.full((Lq,), SENT, device=dev), torch.full((Lq,), SENT, device=dev)
    for bad in range(4):
        ld = [36] * 4
        ld[bad] = 34 + bad % 2
        assert _rc('es_attn_fwd', P(q), ld[0], P(k), ld[1], P(v), ld[2], B, H, Lq, Lk, 0, P(o), ld[3], P(lse), 1, _st()) == -3
    for bad in range(8):
        ld = [36] * 8
        ld[bad] = 37 + bad % 2
        assert _rc('es_attn_bwd', P(q), ld[0], P(k), ld[1], P(v), ld[2], P(o), ld[3], P(do), ld[4], P(lse), B, H, Lq, Lk, 0, P(delta),
                   P(dq), ld[5], P(dk), ld[6], P(dv), ld[7], 0, 1, _st()) == -3
    torch.cuda.synchronize()
    for x in (o, dq, dk, dv, lse, delta):
        assert bool((x == SENT).all())


# ------------------------------------------------------------------------------------------------------------------ LayerNorm
LN_C = (1, 3, 63, 64, 65, 256, 511, 512)
LN_N = (1, 3, 4, 5, 31, 32, 33, 700)
EPS = float(torch.tensor(1e-5, dtype=torch.float32))


def ln_case(dev, stats, n, C, use_res, acc, want_dw, want_db, seed):
    hip = _hip()
    P = hip.P
    g = torch.Generator().manual_seed(seed)
    x, r = torch.randn(n, C, generator=g) * 2 + 0.5, torch.randn(n, C, generator=g)
    w, b, dy = torch.rand(C, generator=g) + .5, torch.randn(C, generator=g), torch.randn(n, C, generator=g)
    xd, rd, wd, bd, dyd = (t.to(dev) for t in (x, r, w, b, dy))
    y, ybuf = _flat(dev, torch.zeros(n, C))
    z, zbuf = _flat(dev, torch.zeros(n, C))
    mean, mbuf = _flat(dev, torch.zeros(n))
    rstd, rbuf = _flat(dev, torch.zeros(n))
    st = _st()
    hip.call('es_layernorm_fwd', P(xd), P(rd) if use_res else 0, n, C, P(wd), P(bd), EPS, P(y), P(z) if use_res else 0, P(mean), P(rstd), st)
    zin = z if use_res else xd
    dz0 = torch.randn(n, C, generator=g)
    dz, dzbuf = _flat(dev, dz0)
    dw0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    dw, dwbuf = _flat(dev, dw0)
    db, dbbuf = _flat(dev, db0)
    need = int(hip.raw('es_layernorm_bwd_workspace_floats')(n, C))
    ws = torch.zeros(need, device=dev) if (want_dw or want_db) else None
    args = lambda dzp, dwp, dbp: ('es_layernorm_bwd', P(dyd), P(zin), n, C, P(wd), P(mean), P(rstd), P(dzp), acc, P(dwp) if want_dw else 0,
                                  P(dbp) if want_db else 0, P(ws), need if ws is not None else 0, st)
    hip.call(*args(dz, dw, db))
    dz2, _ = _flat(dev, dz0)
    dw2, _ = _flat(dev, dw0)
    db2, _ = _flat(dev, db0)
    hip.call(*args(dz2, dw2, db2))                          # a second launch on the same workspace: bit-identical sums, ticket back at 0
    torch.cuda.synchronize()
    label = f'layernorm n={n} C={C} res={use_res} acc={acc} dw={want_dw} db={want_db}'
    for buf, m in ((ybuf, n * C), (mbuf, n), (rbuf, n), (dzbuf, n * C), (dwbuf, C), (dbbuf, C)):
        _tail_ok(buf, m, label)
    if use_res:
        _tail_ok(zbuf, n * C, label)
    assert torch.equal(dw, dw2) and torch.equal(db, db2) and torch.equal(dz, dz2), f'{label}: two launches differ'
    if ws is not None:
        assert int(ws[:1].view(torch.int32)) == 0, f'{label}: the ticket does not read zero afterwards'
    if not want_dw:
        assert torch.equal(dw.cpu(), dw0)
    if not want_db:
        assert torch.equal(db.cpu(), db0)
    S.check_layernorm(dict(x=xd, res=rd if use_res else None, z=z if use_res else None, eps=EPS, mean=mean, rstd=rstd, w=wd, b=bd, y=y), dev, stats)
    rec = dict(dy=dyd, z=zin, w=wd, mean=mean, rstd=rstd, dz=dz, dz0=dz0 if acc else None, dw0=dw0, dw1=dw if want_dw else None, db0=db0,
               db1=db if want_db else None)
    S.check_layernorm_bwd(rec, dev, stats)
    return rec


def ln_grid(dev):
    """(n, C, res, acc, dw, db) cases.  n >= 32 (more than one wave slice; from n = 33 more than one workgroup, n = 700: 22 workgroups
    and a real last-workgroup election) runs all four dw / db choices at every C; below that the choice rotates.  res and accumulate
    advance on counters of their own (periods 2 and 3), so neither is tied to n, to C or to the dw / db choice.  The emulator keeps
    n = 700 at C in {65, 512} only."""
    cases, i = [], 0
    for C in LN_C:
        for n in LN_N:
            if _small(dev) and n == 700 and C not in (65, 512):
                continue
            for want in (((1, 1), (1, 0), (0, 1), (0, 0)) if n >= 32 else (((1, 1), (1, 0), (0, 1), (0, 0))[i % 4],)):
                cases.append((n, C, i % 2, int(i % 3 == 1), want[0], want[1]))
                i += 1
    big = {(c[4], c[5], c[2], c[3]) for c in cases if c[0] >= 33}
    assert {(1, 1), (1, 0), (0, 1), (0, 0)} == {b[:2] for b in big}, 'dw + db, dw-only, db-only and neither must occur on more than one workgroup'
    assert all((dw, db, r, a) in big for dw, db in ((1, 1), (1, 0)) for r in (0, 1) for a in (0, 1)), \
        'dw + db and dw-only must each occur with and without res / accumulate at n >= 33'
    assert any(c[0] == 700 and c[4] and c[5] for c in cases) and any(c[0] == 700 and c[4] and not c[5] for c in cases)
    return cases


def test_layernorm_fwd_bwd_on_the_shape_grid(dev):
    """every launch twice on one workspace: bit-identical dz / dw / db and a zero ticket afterwards (ln_case), on the whole grid"""
    stats = S.Stats('layernorm grid')
    for i, (n, C, res, acc, want_dw, want_db) in enumerate(ln_grid(dev)):
        ln_case(dev, stats, n, C, res, acc, want_dw, want_db, 300 + i)
    print(stats.report())


def test_layernorm_refusals_leave_the_outputs_untouched(dev):
    """C = 513 returns -4; a workspace that is too small (or NULL) returns -5; nothing is written in either case"""
    hip = _hip()
    P = hip.P
    n = 40
    for C, ws_short, want in ((513, 0, -4), (64, 1, -5), (64, None, -5)):
        t = lambda *s: torch.full(s, SENT, device=dev)
        x, w, b, y, mean, rstd, dz, dw, db = t(n, C), t(C), t(C), t(n, C), t(n), t(n), t(n, C), t(C), t(C)
        if want == -4:
            assert _rc('es_layernorm_fwd', P(x), 0, n, C, P(w), P(b), EPS, P(y), 0, P(mean), P(rstd), _st()) == -4
        need = int(hip.raw('es_layernorm_bwd_workspace_floats')(n, min(C, 512)))
        ws = None if ws_short is None else torch.zeros(need - ws_short, device=dev)
        rc = _rc('es_layernorm_bwd', P(x), P(x), n, C, P(w), P(mean), P(rstd), P(dz), 0, P(dw), P(db), P(ws), 0 if ws is None else ws.numel(), _st())
        torch.cuda.synchronize()
        assert rc == want, (C, ws_short, rc)
        for o in (y, mean, rstd, dz, dw, db):
            assert bool((o == SENT).all())
        assert ws is None or not bool(ws.any())


# ------------------------------------------------------------------------------------------------------------------ ContrastiveEmbed
def contrastive_case(dev, stats, B, L, T, C, Tout, tlen, vlen, want_dv, acc_v, seed, want_dtext=True, want_dbias=True):
    hip = _hip()
    P = hip.P
    g = torch.Generator().manual_seed(seed)
    v, text = torch.randn(B, L, C, generator=g), torch.randn(B, T, C, generator=g)
    bias = torch.tensor([-4.6])
    tl = torch.tensor(tlen, dtype=torch.int32)
    vl = None if vlen is None else torch.tensor(vlen, dtype=torch.int32)
    vd, td, bd, tld = v.to(dev), text.to(dev), bias.to(dev), tl.to(dev)
    vld = None if vl is None else vl.to(dev)
    lo, lobuf = _flat(dev, torch.zeros(B, L, Tout))
    rm, rmbuf = _flat(dev, torch.zeros(B, L))
    st = _st()
    hip.call('es_contrastive_fwd', P(vd), B, L, P(td), T, C, P(tld), P(vld), P(bd), P(lo), Tout, P(rm), st)
    torch.cuda.synchronize()
    label = f'contrastive B={B} L={L} T={T} C={C} Tout={Tout} tlen={tlen} vlen={vlen}'
    _tail_ok(lobuf, B * L * Tout, label)
    _tail_ok(rmbuf, B * L, label)
    # the forward specification works on T columns: columns T .. Tout must be -inf, and with Tout < T only Tout columns exist
    m = min(T, Tout)
    assert bool(torch.isneginf(lo[:, :, m:]).all()), f'{label}: columns beyond T are not -inf'
    lo_T = torch.full((B, L, T), -math.inf, device=dev)
    lo_T[:, :, :m] = lo[:, :, :m]
    tl_eff = tl.clamp(max=m)
    S.check_contrastive(dict(B=B, L=L, T=T, v=vd.view(B * L, C), text=td.view(B * T, C), bias=bd, tlen=tl_eff, vlen=vl, logits=lo_T, rowmax=rm),
                        dev, stats)
    # dlogits: 0 at masked positions (the contract of the backward); NaN in the columns a Tout < T launch must never read is not
    # possible inside a row (the next row starts there), so those launches are checked through the specification alone
    live = (torch.arange(Tout)[None, None, :] < tl.long().clamp(min=0, max=m)[:, None, None])
    if vl is not None:
        live = live & (torch.arange(L)[None, :, None] < vl.long().clamp(min=0, max=L)[:, None, None])
    dl = torch.randn(B, L, Tout, generator=g) * live
    dld, dlbuf = _flat(dev, dl)
    dv0, dt0, db0 = torch.randn(B, L, C, generator=g), torch.randn(B, T, C, generator=g), torch.randn(1, generator=g)
    dv, dvbuf = _flat(dev, dv0)
    dt, dtbuf = _flat(dev, dt0)
    db, dbbuf = _flat(dev, db0)
    need = int(hip.raw('es_contrastive_bwd_workspace_floats')(B, T))
    ws = torch.zeros(need, device=dev)
    hip.call('es_contrastive_bwd', P(dld), Tout, P(vd), B, L, P(td), T, C, P(tld), P(dv) if want_dv else 0, acc_v, P(dt) if want_dtext else 0,
             P(db) if want_dbias else 0, P(ws), need, st)
    torch.cuda.synchronize()
    for buf, n in ((dvbuf, B * L * C), (dtbuf, B * T * C), (dbbuf, 1)):
        _tail_ok(buf, n, label)
    if want_dtext or want_dbias:
        assert int(ws[:1].view(torch.int32)) == 0, f'{label}: the ticket does not read zero afterwards'
    if not want_dv:
        assert torch.equal(dv.cpu(), dv0)
    rec = dict(B=B, L=L, T=T, C=C, Tout=Tout, dl=dld, v=vd, text=td, tlen=tl, dv=dv if want_dv else None, dv0=dv0 if acc_v else None,
               dtext0=dt0, dtext1=dt if want_dtext else None, dbias0=db0, dbias1=db if want_dbias else None)
    S.check_contrastive_bwd(rec, dev, stats)
    return rec, dict(logits=lo, rowmax=rm)


def _tmax(C):
    """the largest T es_contrastive_fwd / _bwd accept: T C 4 <= 160 KiB - 1 KiB"""
    return (160 * 1024 - 1024) // (4 * C)


def test_contrastive_fwd_bwd_on_the_shape_grid(dev):
    stats = S.Stats('contrastive grid')
    small = _small(dev)
    B, L = 2, (9 if small else 45)
    cases = []
    for i, C in enumerate((64, 100, 256, 512)):
        t64 = 65536 // (4 * C)                                   # T C 4 = 64 KiB exactly at t64 (C = 100: 163 -> 65 200 B, just under)
        for T in (9, t64, t64 + 1, _tmax(C)):
            cases.append((C, T))
    for i, (C, T) in enumerate(cases):
        if small and T > 200 and C != 256 and T != _tmax(C):
            continue                                             # (emulator: the > 64 KiB branch at C = 256 and the largest T of every C)
        Lc = 5 if (small and T > 200) else L
        tlen = [T, (0, 1, T // 2, T - 1)[i % 4]]
        vlen = (None, [Lc, 0], [Lc - 1, Lc // 2], [Lc + 3, 1])[i % 4]
        contrastive_case(dev, stats, B, Lc, T, C, T + (0, 3, 0, 1)[i % 4], tlen, vlen, i % 3 != 2, i % 2, 500 + i)
    contrastive_case(dev, stats, 2, L, 9, 64, 12, [12, 4], None, True, 0, 560, want_dtext=False)
    contrastive_case(dev, stats, 2, L, 9, 64, 9, [9, 4], None, False, 0, 561, want_dbias=False)
    print(stats.report())


def test_contrastive_refuses_a_text_block_beyond_the_lds(dev):
    hip = _hip()
    P = hip.P
    for C in (64, 512):
        T, B, L = _tmax(C) + 1, 1, 3
        t = lambda *s: torch.full(s, SENT, device=dev)
        v, text, lo, rm, dv, dt, db = t(B, L, C), t(B, T, C), t(B, L, T), t(B, L), t(B, L, C), t(B, T, C), t(1)
        tl = torch.tensor([T], dtype=torch.int32, device=dev)
        ws = torch.zeros(int(hip.raw('es_contrastive_bwd_workspace_floats')(B, T)), device=dev)
        assert _rc('es_contrastive_fwd', P(v), B, L, P(text), T, C, P(tl), 0, 0, P(lo), T, P(rm), _st()) == -4
        assert _rc('es_contrastive_bwd', P(lo), T, P(v), B, L, P(text), T, C, P(tl), P(dv), 0, P(dt), P(db), P(ws), ws.numel(), _st()) == -4
        assert _rc('es_contrastive_bwd', P(lo), 9, P(v), B, L, P(text), 9, C, P(tl), P(dv), 0, P(dt), P(db), P(ws), 3, _st()) == -5
        torch.cuda.synchronize()
        for o in (lo, rm, dv, dt, db):
            assert bool((o == SENT).all())


def test_contrastive_tout_below_the_token_count(dev):
    """Tout < min(tlen, T): both kernels work on Tout columns.  The dlogits buffer ends with its last row (a sentinel follows), every
    row's successor holds different gradients, and dtext rows Tout .. T keep their prior: before the fix the backward read dl[t] for
    t up to tlen, i.e. into the next row (and past the buffer's end on the last one)"""
    stats = S.Stats('contrastive Tout < T')
    for i, (T, Tout, tlen) in enumerate(((9, 5, [9, 7]), (9, 1, [9, 3]), (40, 33, [40, 36]))):
        contrastive_case(dev, stats, 2, 9 if _small(dev) else 45, T, 64, Tout, tlen, None, True, i % 2, 600 + i)
    print(stats.report())


def test_contrastive_tout_at_least_t_is_unchanged(dev):
    """results for Tout >= T equal those of Tout = T bit for bit in the shared columns (the clamp of the fix is inert there)"""
    stats = S.Stats('contrastive Tout >= T')
    a, fa = contrastive_case(dev, stats, 2, 9, 9, 100, 9, [9, 4], [9, 5], True, 0, 610)
    b, fb = contrastive_case(dev, stats, 2, 9, 9, 100, 13, [9, 4], [9, 5], True, 0, 610)
    assert torch.equal(fa['logits'], fb['logits'][:, :, :9]) and torch.equal(fa['rowmax'], fb['rowmax'])


# ------------------------------------------------------------------------------------------------------------------ box coders
def _next(x, k):
    """the f32 k ulps above (k > 0) or below x"""
    t = torch.tensor([x], dtype=torch.float32)
    for _ in range(abs(k)):
        t = torch.nextafter(t, torch.tensor([math.inf if k > 0 else -math.inf]))
    return float(t)


def test_box_coders_at_the_clamp(dev):
    """baseline and FCAF coders, forward and backward (accumulate 0 and 1) on regression outputs as column slices: random rows, rows far
    below the clamp, rows 2 / 3 ulps of the argument on either side of log(2e-2) (exp is then 8 - 12 u away from the clamp: the
    kernel's f32 expf and the f64 exp agree on the side), angles up to +-8 and at multiples of pi / 2.  A row whose f32 expf equals
    2e-2 exactly -- the one point where the baseline rule (>) and the FCAF rule (>=) differ -- cannot be told from outside the kernel
    (ground_spec docstring), so the two rules are NOT distinguished by this test"""
    hip = _hip()
    P = hip.P
    stats = S.Stats('box coders')
    g = torch.Generator().manual_seed(41)
    n = 300
    pred = torch.randn(n, 9, generator=g)
    pred[:20, :6] = -6.0 + torch.randn(20, 6, generator=g) * 0.1
    l0 = math.log(S.LO)
    for r, kk in enumerate((-3, -2, 2, 3)):
        pred[20 + r, :6] = _next(l0, kk)
        pred[24 + r, 0:6:2] = _next(l0, kk)                       # one face of each pair at the clamp, the other free
    pred[30:60, 6:9] = (torch.rand(30, 3, generator=g) * 16 - 8)
    pred[60:70, 6:9] = torch.randint(-4, 5, (10, 3), generator=g).float() * (math.pi / 2)
    pts, gb = torch.randn(n, 3, generator=g) * 3, torch.randn(n, 9, generator=g)
    e = torch.exp(pred[:, :6].double())
    assert int((e < S.LO).sum()) > 100 and int(((e / S.LO - 1).abs() < 16 * S.U).sum()) >= 24
    for coder, fwd, bwd, cf, cb in (('baseline', 'es_ground_decode_fwd', 'es_ground_decode_bwd', S.check_decode_fwd, S.check_decode_bwd),
                                    ('fcaf', 'es_ground_decode_fcaf_fwd', 'es_ground_decode_fcaf_bwd', S.check_decode_fcaf_fwd,
                                     S.check_decode_fcaf_bwd)):
        Pr = Cols(dev, n, 9, 16, 3, pred)
        ptsd, gbd = pts.to(dev), gb.to(dev)
        box, boxbuf = _flat(dev, torch.zeros(n, 9))
        hip.call(fwd, Pr.ptr(), 16, P(ptsd), n, P(box), _st())
        torch.cuda.synchronize()
        _tail_ok(boxbuf, n * 9, coder)
        cf(coder, Pr.v, ptsd, box, stats)
        for acc in (0, 1):
            prior = torch.randn(n, 9, generator=g)
            D = Cols(dev, n, 9, 12, 2, prior)
            hip.call(bwd, Pr.ptr(), 16, P(gbd), n, D.ptr(), 12, acc, _st())
            torch.cuda.synchronize()
            D.untouched_outside(coder + ' bwd')
            cb(f'{coder} acc={acc}', Pr.v, gbd, D.v, prior.to(dev) if acc else None, stats)
    print(stats.report())


# ------------------------------------------------------------------------------------------------------------------ matching, focal
def _boxes(g, n):
    return torch.cat([torch.rand(n, 3, generator=g) * 2 - 1, torch.rand(n, 3, generator=g) * 1.5 + 0.2, torch.rand(n, 3, generator=g) * 6 - 3], 1)


def match_case(dev, Q, Gs, T, seed, dup=True, nan_boxes=True):
    """es_ground_match on B = len(Gs) samples with ties: duplicated queries (logits and boxes), duplicated ground-truth boxes (with
    their positive maps), NaN query boxes (cost 100 against every box).  Returns what check_assignment / check_focal need"""
    hip = _hip()
    P = hip.P
    g = torch.Generator().manual_seed(seed)
    B, Gmax = len(Gs), max(max(Gs), 1)
    logits = torch.randn(B, Q, T, generator=g) * 2
    boxes = torch.stack([_boxes(g, Q) for _ in range(B)])
    gtb, pm = [], []
    for b, n in enumerate(Gs):
        # ground-truth boxes near some of the sample's queries, so that the IoU term is live
        src = boxes[b, torch.randint(0, Q, (n,), generator=g)].clone()
        src[:, :6] += torch.randn(n, 6, generator=g) * 0.05
        src[:, 3:6] = src[:, 3:6].abs() + 0.05
        m = (torch.rand(n, T, generator=g) < 0.3).to(torch.uint8)
        if dup and n >= 2:
            for r in range(1, n, 2):                             # every second box repeats its predecessor
                src[r], m[r] = src[r - 1], m[r - 1]
        gtb.append(src)
        pm.append(m)
    if dup and Q >= 2:
        for b in range(B):
            for qi in range(1, Q, 3):                            # every third query repeats its predecessor
                logits[b, qi], boxes[b, qi] = logits[b, qi - 1], boxes[b, qi - 1]
    if nan_boxes and Q >= 7:
        boxes[:, 5::7, 0] = float('nan')
    tlen = torch.tensor([T - (b % 2) * (T // 3) for b in range(B)], dtype=torch.int32)
    gt_off = [0] + list(np.cumsum(Gs))
    gt_boxes = torch.cat(gtb) if sum(Gs) else torch.zeros(0, 9)
    pos_map = torch.cat(pm) if sum(Gs) else torch.zeros(0, T, dtype=torch.uint8)
    ld, bd, gd, pd = logits.to(dev), boxes.to(dev), gt_boxes.to(dev), pos_map.to(dev)
    god, tld = torch.tensor(gt_off, dtype=torch.int32, device=dev), tlen.to(dev)
    cost = torch.full((B, Gmax, Q), 1e300, dtype=torch.float64, device=dev)
    work = torch.zeros(B * (Gmax + 2 * Q), dtype=torch.float64, device=dev)
    iwork = torch.zeros(B * (4 * Q + 2 * Gmax), dtype=torch.int32, device=dev)
    q2g, qbuf = _flat(dev, torch.full((B, Q), -7, dtype=torch.int32))
    hip.call('es_ground_match', P(ld), T, P(bd), B, Q, P(gd), P(pd), P(god), Gmax if sum(Gs) else 0, P(tld), T, 1.0, 2.0, 2.0, P(cost), P(work),
             P(iwork), P(q2g), _st())
    torch.cuda.synchronize()
    assert bool((qbuf[B * Q:] == int(SENT)).all()), 'es_ground_match wrote past the end of q2g'
    return dict(logits=ld, boxes=bd, gt_boxes=gd, pos_map=pd, gt_off=gt_off, gt_off_dev=god, tlen=tld, T=T, cost=cost.cpu().numpy(),
                q2g=q2g, Gs=Gs, Q=Q)


def test_assignment_on_tied_costs_through_both_solvers(dev):
    """k_lsa_wave at Q in {1, 7, 64, 65, 256, 1024}, k_lsa at Q = 1025 (G <= 8); samples with G = 0 and G = Q; Gmax > Q returns -5"""
    small = _small(dev)
    cases = [(1, [1, 0]), (7, [7, 0, 3]), (64, [64, 5]), (65, [65, 0, 9]), (256, [0, 12, 40] if not small else [0, 12]),
             (1024, [8, 0, 30] if not small else [6, 0]), (1025, [8, 0, 5] if not small else [4, 0])]
    for i, (Q, Gs) in enumerate(cases):
        r = match_case(dev, Q, Gs, 6, 700 + i)
        cost = r['cost']
        for b, n in enumerate(Gs):
            if n >= 2:                                           # the case set does contain ties
                assert np.unique(cost[b, :n]).size < cost[b, :n].size
        S.check_assignment(f'match Q={Q} Gs={Gs}', cost, Gs, r['q2g'].cpu().numpy())
        print(f'es_ground_match Q={Q} G={Gs} ({"k_lsa" if Q > 1024 else "k_lsa_wave"}): optimal, one-to-one, scipy\'s tie resolution')
    P = _hip().P
    z = torch.zeros(64, device=dev)
    zi = torch.zeros(64, dtype=torch.int32, device=dev)
    q2g = torch.full((1, 3), -7, dtype=torch.int32, device=dev)
    assert _rc('es_ground_match', P(z), 2, P(z), 1, 3, P(z), P(zi), P(zi), 4, P(zi), 2, 1.0, 2.0, 2.0, P(z.double()), P(z.double()), P(zi),
               P(q2g), _st()) == -5
    torch.cuda.synchronize()
    assert bool((q2g == -7).all())


def test_focal_loss_per_element(dev):
    """es_ground_focal after a real assignment: logits up to +-30, unmatched rows, a sample without boxes, Tout > T"""
    hip = _hip()
    P = hip.P
    stats = S.Stats('focal')
    for i, (Q, Gs, T, Tout) in enumerate(((33, [5, 0, 9], 70, 70), (7, [7, 2], 6, 9), (130, [0, 0], 65, 65))):
        if _small(dev):
            Gs = Gs[:2]
        r = match_case(dev, Q, Gs, T, 800 + i, nan_boxes=False)
        B = len(Gs)
        g = torch.Generator().manual_seed(810 + i)
        x = torch.randn(B, Q, Tout, generator=g) * 3
        big = torch.tensor([30.0, 17.0, 9.0, 25.5])[torch.randint(0, 4, (B, Q, Tout), generator=g)]
        big = big * (torch.randint(0, 2, (B, Q, Tout), generator=g) * 2 - 1).float()
        x = torch.where(torch.rand(B, Q, Tout, generator=g) < 0.3, big, x)
        x[0, 0, 0], x[0, 0, 1] = 30.0, -30.0
        xd = x.to(dev)
        avg = torch.tensor([float(max(sum(Gs), 1))], device=dev)
        dl, dlbuf = _flat(dev, torch.full((B, Q, Tout), SENT))
        loss = torch.tensor([0.75], dtype=torch.float64, device=dev)
        hip.call('es_ground_focal', P(xd), Tout, B, Q, P(r['q2g']), P(r['pos_map']), P(r['gt_off_dev']), P(r['tlen']), T, 0.25, 2.0, P(avg), 0.5,
                 P(dl), P(loss), _st())
        torch.cuda.synchronize()
        _tail_ok(dlbuf, B * Q * Tout, 'focal')
        S.check_focal(dict(logits=xd, q2g=r['q2g'], pos_map=r['pos_map'], gt_off=r['gt_off'], tlen=r['tlen'], T=T, alpha=0.25, gamma=2.0,
                           avg=float(avg), grad_scale=0.5, dlogits=dl, loss0=0.75, loss1=loss), dev, stats)
    print(stats.report())


# ------------------------------------------------------------------------------------------------------------------ top-k
def topk_case(dev, vals, vlen, k):
    hip = _hip()
    P = hip.P
    B, L = vals.shape
    vd = vals.to(dev)
    vl = None if vlen is None else torch.tensor(vlen, dtype=torch.int32, device=dev)
    idx = torch.full((B * k + 8,), -9, dtype=torch.int32, device=dev)
    hip.call('es_topk_sorted', P(vd), B, L, P(vl), k, P(idx), _st())
    torch.cuda.synchronize()
    assert bool((idx[B * k:] == -9).all())
    S.check_topk(f'top-k L={L} vlen={vlen} k={k}', vals, vlen, k, idx[:B * k].view(B, k).cpu())
    return idx[:B * k].view(B, k).cpu()


def _topk_vals(g, B, L):
    """random values with blocks of equal values, +-inf and both zeros"""
    v = torch.randn(B, L, generator=g)
    if L >= 8:
        v[:, L // 4:L // 4 + max(L // 8, 2)] = 0.5                # a block of equal values
        v[:, 3::7] = torch.randint(-2, 3, v[:, 3::7].shape, generator=g).float()     # many small integers (0.0 among them)
        v[:, 1], v[:, L - 2] = math.inf, -math.inf
        v[:, 2], v[:, L // 2] = -0.0, 0.0
    return v


def test_topk_sorted_on_the_length_grid(dev):
    """L in {1, 2, 500, 1023, 1024, 1025, 8192, 8193, 16384} (dynamic LDS above 8192); vlen NULL / 0 / 1 / L; k = 1 and k > n;
    L = 16385 returns -4"""
    g = torch.Generator().manual_seed(51)
    small = _small(dev)
    for L in (1, 2, 500, 1023, 1024, 1025, 8192, 8193, 16384):
        B = 1 if (small and L > 1025) else 3
        v = _topk_vals(g, B, L)
        topk_case(dev, v, None if B == 1 else [L, 0, 1], 1)
        if not (small and L > 8193):
            topk_case(dev, v, [L + 5, L // 2, 1][:B], min(L + 3, 300))
        if L in (500, 1025) or (L == 8193 and not small):
            topk_case(dev, v, None, L)
    P = _hip().P
    idx = torch.full((4,), -9, dtype=torch.int32, device=dev)
    vd = torch.zeros(16385, device=dev)
    assert _rc('es_topk_sorted', P(vd), 1, 16385, 0, 4, P(idx), _st()) == -4
    torch.cuda.synchronize()
    assert bool((idx == -9).all())


def test_topk_sorted_treats_the_two_zeros_as_equal(dev):
    """+0.0 and -0.0 tie: the lower row comes first (torch.argsort(stable=True)); the sort key used to order +0.0 before -0.0"""
    v = torch.tensor([[-1.0, -0.0, 0.0, -0.0, 0.0, 2.0, -0.0]])
    got = topk_case(dev, v, None, 7)
    assert got[0].tolist() == [5, 1, 2, 3, 4, 6, 0]


# ------------------------------------------------------------------------------------------------------------------ box IoU
def _iou(dev, a, b):
    hip = _hip()
    P = hip.P
    ad, bd = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev), torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).to(dev)
    out = torch.full((a.shape[0] * b.shape[0] + 8,), SENT, device=dev)
    hip.call('es_box3d_iou', P(ad), a.shape[0], P(bd), b.shape[0], P(out), _st())
    torch.cuda.synchronize()
    assert bool((out[a.shape[0] * b.shape[0]:] == SENT).all())
    return out[:a.shape[0] * b.shape[0]].view(a.shape[0], b.shape[0]).cpu().double().numpy()


def _quarter_turns(box, axis, k):
    """the SAME box described with an Euler angle of k pi / 2 about one axis (ZXY order: angle 0 about z, 1 about x, 2 about y) and
    the two sizes across that axis swapped for odd k"""
    b = np.array(box, dtype=np.float64)
    b[6 + axis] = k * math.pi / 2
    if k % 2:
        i, j = ((3, 4), (4, 5), (3, 5))[axis]
        b[i], b[j] = b[j], b[i]
    return b


def test_box3d_iou_closed_form_quarter_turns_thin_boxes(dev):
    """axis-aligned pairs against the closed form (face-sharing, edge-touching, contained, identical, partial overlaps, thin boxes at
    the 2e-2 clamp, aspect ratios up to 100); the same pairs with each box described through quarter turns about each axis (IoU
    unchanged to 1e-6); symmetry; generic oriented pairs against the oracle's qhull construction"""
    from oracle import grounding as OG
    z3 = [0, 0, 0]
    A = np.array([[0, 0, 0, 2, 2, 2] + z3, [0, 0, 0, 2, 2, 2] + z3, [0, 0, 0, 2, 2, 2] + z3, [0, 0, 0, 2, 2, 2] + z3, [0, 0, 0, 2, 2, 2] + z3,
                  [0.1, -0.2, 0.3, 1, 2, 3] + z3, [0, 0, 0, 2, 0.02, 1] + z3, [0, 0, 0, 0.02, 0.02, 0.02] + z3, [0, 0, 0, 2, 0.02, 2] + z3,
                  [1, 1, 1, 0.5, 3, 0.7] + z3], dtype=np.float64)
    Bx = np.array([[2, 0, 0, 2, 2, 2] + z3,                       # shares a face
                   [2, 2, 0, 2, 2, 2] + z3,                       # touches along an edge
                   [0.2, 0.1, -0.3, 0.5, 0.6, 0.7] + z3,          # contained
                   [0, 0, 0, 2, 2, 2] + z3,                       # identical
                   [0.5, 0.25, -0.75, 2, 1, 3] + z3,              # partial
                   [0.4, 0.3, 0.2, 2, 1, 1.5] + z3,
                   [0.5, 0.01, 0.1, 2, 0.02, 1] + z3,             # thin plates, half a thickness apart
                   [0.01, 0, 0, 0.02, 0.02, 0.02] + z3,           # clamp-sized cubes
                   [0, 0, 0, 0.02, 2, 2] + z3,                    # crossing plates, aspect 100
                   [1.1, 1.5, 1.2, 0.5, 3, 0.7] + z3], dtype=np.float64)
    want = S.aligned_iou(A[:, :6], Bx[:, :6])
    got = np.diag(_iou(dev, A, Bx))
    err = float(np.abs(got - want).max())
    print(f'box3d IoU, {len(A)} axis-aligned pairs vs the closed form: max abs err {err:.2e} (tol 1e-6)')
    assert err < 1e-6 and got[0] == 0.0 and got[1] == 0.0 and abs(got[3] - 1) < 1e-6
    # Quarter turns.  f32 cannot hold k pi / 2: the box the kernel reads is tilted about its centre by d = |f32(k pi / 2) - k pi / 2|
    # (4.4e-8 .. 1.7e-7) around one world axis w.  To first order a tilt moves the points of a face with normal u (u perpendicular to
    # w) along u by d |t - c_t| (t the third axis, c the box centre), so a face of the tilted box that bounds the intersection changes
    # its volume by at most d o_w int |t - c_t| dt over the overlap's extent in t, and the IoU moves by (1 + IoU)^2 / (Va + Vb) times
    # the volume change.  Against the closed form of the unturned pair the kernel is held to 1e-6 + that term (2e-9 for the unit-sized
    # pairs, up to 4e-6 for the plates of aspect 100).  Against the IoU of the very f32 boxes it read it is held to a flat 1e-6, twice:
    # by the qhull construction (half-space intersection + convex hull, nothing in common with the kernel's clipping) wherever the
    # boxes overlap by more than a sliver, and by the oracle's polyhedral construction on every pair.
    WAX = (2, 0, 1)                                              # Euler angle index (ZXY) -> world axis of the turn

    def tilt_volume(X, Y, ang, d):
        c, h, w = X[:3], X[3:6] / 2, WAX[ang]
        lo, hi = np.maximum(c - h, Y[:3] - Y[3:6] / 2), np.minimum(c + h, Y[:3] + Y[3:6] / 2)
        if bool((hi - lo < -1e-9).any()):
            return 0.0
        o = np.clip(hi - lo, 0, None)
        total = 0.0
        for u in range(3):
            if u == w:
                continue
            t = 3 - u - w
            faces = int(abs(lo[u] - (c[u] - h[u])) < 1e-9) + int(abs(hi[u] - (c[u] + h[u])) < 1e-9)
            a, b = lo[t] - c[t], hi[t] - c[t]                    # int_a^b |x| dx
            lever = (b * abs(b) - a * abs(a)) / 2
            total += faces * o[w] * lever
        return d * total

    def angle_error(k):
        return abs(float(np.float32(k * math.pi / 2)) - k * math.pi / 2)
    worst, worst_o, worst_q, worst_ratio, n_q = 0.0, 0.0, 0.0, 0.0, 0
    va_vb = np.prod(A[:, 3:6], 1) + np.prod(Bx[:, 3:6], 1)
    for axis in range(3):
        for ka in (-3, -1, 1, 2, 4):
            for kb in (0, 1, 2, 3):
                axb = (axis + kb) % 3 if kb else axis
                a2 = np.stack([_quarter_turns(x, axis, ka) for x in A])
                b2 = np.stack([_quarter_turns(x, axb, kb) for x in Bx])
                got = np.diag(_iou(dev, a2, b2))
                a32, b32 = a2.astype(np.float32).astype(np.float64), b2.astype(np.float32).astype(np.float64)
                exact = np.array([OG.box3d_iou(a32[i], b32[i]) for i in range(len(A))])
                dI = np.array([tilt_volume(A[i], Bx[i], axis, angle_error(ka)) + tilt_volume(Bx[i], A[i], axb, angle_error(kb))
                               for i in range(len(A))])
                tol = 1e-6 + (1 + want) ** 2 / va_vb * dI
                worst, worst_o = max(worst, float(np.abs(got - want).max())), max(worst_o, float(np.abs(got - exact).max()))
                worst_ratio = max(worst_ratio, float((np.abs(got - want) / tol).max()))
                if (axis, kb) in ((0, 0), (1, 1), (2, 3)):       # (the qhull construction costs ~10 ms a pair: a third of the turns)
                    for i in np.nonzero(want > 1e-3)[0]:
                        worst_q, n_q = max(worst_q, abs(got[i] - OG.box3d_iou_qhull(a32[i], b32[i]))), n_q + 1
    print(f'the same pairs through quarter turns about each axis: max abs deviation from the IoU of the f32 boxes {worst_q:.2e} (qhull, {n_q} '
          f'pairs) / {worst_o:.2e} (polyhedral oracle), tol 1e-6; {worst:.2e} from the closed form (at most {worst_ratio:.2f} of 1e-6 + the '
          f'tilt of the f32 angles)')
    assert worst_o < 1e-6 and worst_q < 1e-6 and n_q >= 60 and worst_ratio < 1.0
    rng = np.random.default_rng(5)
    n = 12 if _small(dev) else 40
    a = np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.uniform(.2, 2., (n, 3)), rng.uniform(-3.1, 3.1, (n, 3))], 1)
    b = a + np.concatenate([rng.normal(0, .3, (n, 3)), rng.normal(0, .1, (n, 3)), rng.normal(0, .4, (n, 3))], 1)
    b[:, 3:6] = np.abs(b[:, 3:6]) + .05
    a[:3, 3:6] *= [[100, 1, 1], [1, 0.01, 1], [0.1, 10, 0.1]]      # aspect ratios up to 100
    a, b = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    ab, ba = _iou(dev, a, b), _iou(dev, b, a)
    assert float(np.abs(ab - ba.T).max()) < 1e-6, 'iou(a, b) != iou(b, a)'
    wq = np.array([OG.box3d_iou_qhull(a[i], b[i]) for i in range(n)])
    err = float(np.abs(np.diag(ab) - wq).max())
    print(f'{n} oriented pairs vs the qhull construction: max abs err {err:.2e} (tol 1e-6); symmetric to 1e-6')
    assert err < 1e-6 and float((wq > 0.05).mean()) > 0.3
