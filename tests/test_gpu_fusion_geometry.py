"""The geometry of all seven projection-fusion forward entry points (csrc/fusion.hip) held to tests/fusion_geom_spec.py: pix and cnt
of every launch against the f64 restatement of undo_aug + project_view with a running error bound per value, on a shape grid and on a
dyadic edge lattice whose every intermediate is exact in f32.

Grid: V in {1, 2, 63, 64, 65, 66, 67, 70} for es_point_sample_fwd / _fwd_h / _fwd_pts (65, 66: two ballot trips with a staged meta
block; 67, 70: two trips with the meta block read from global memory), V in {1, 2, 10, 63, 64} for the window and prefix kernels, five
one-view calls with the running sum and count for the step kernel; C in {1, 63, 64, 65, 128, 512}; n in {1, 15, 16, 17, 333} (50 for
333 on the CPU emulator); B in {1, 2, 3} with the sample boundary inside a 16-row workgroup and once on a multiple of 16;
reverse-augmentation op lists that differ between the samples, or none; 0, 1 or 3 leading views that look away; maps of 5 x 7,
15 x 20 and 60 x 80 pixels; ldo = C + 8 with a guard band; 8 sentinel ints behind pix and cnt; bf16 maps for the _h entry points
(exact bf16 values, so the f32 launch on the same values must agree bit for bit).

Per launch: fusion_geom_spec.check_geometry with the caps (undecided pairs <= 1 / 500, rows with one <= 1 / 100), `out` within the
sum bound of window_spec / prefix_spec on the launch's own pix and cnt, guard bands intact, two runs bit-equal.  The coverage the grid
must have is asserted from the SPECIFICATION.  Refusals write nothing.

Every body is a function of `dev`: tests/test_emu_fusion_geometry.py runs the same bodies on the CPU emulator."""
import pytest
import torch

import fusion_geom_spec as G
import prefix_spec as PS
import walk_spec as W
import window_spec as WS

pytestmark = pytest.mark.gpu

SENT = -7.25e5
ISENT = -77
ENTRIES = ('fwd', 'fwd_h', 'fwd_pts', 'win', 'win_h', 'prefix', 'step')
NAME = dict(fwd='es_point_sample_fwd', fwd_h='es_point_sample_fwd_h', fwd_pts='es_point_sample_fwd_pts', win='es_point_sample_win_fwd',
            win_h='es_point_sample_win_fwd_h', prefix='es_point_sample_prefix_fwd_pts', step='es_point_sample_step_fwd_pts')
INTS = ('fwd', 'fwd_h', 'win', 'win_h')                   # integer voxel coordinates * voxel_size; the others take float points
MAPS = ((5, 7), (15, 20), (60, 80))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _hip():
    from embodiedscan_amd import hip
    return hip


def _st():
    return torch.cuda.current_stream().cuda_stream


def _small(dev):
    return dev.type == 'cpu'


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def plant_shallow(case, k):
    """move the first k rows of every sample to a depth of 5e-4 in front of view 0 of their sample (0 < qz < 1e-3: the clamp decides
    their pixel), a fraction of a pixel off the optical axis.  Only for cases without reverse-augmentation ops"""
    assert not bool((case['meta'][:, PS.NOPS] != 0).any())
    pts, b = case['points'], case['coords'][:, 0]
    for s in range(case['B']):
        rows = torch.nonzero(b == s).squeeze(1)[:k]
        P = case['meta'][s, PS.PROJ:PS.PROJ + 12].double().reshape(3, 4)
        d = P[2, :3]
        rx, ry = (P[0, :3] - 32.0 * d) / 40.0, (P[1, :3] - 24.0 * d) / 40.0           # prefix_spec.make_case: focal 40, image 48 x 64
        cam = -P[2, 3] * d                                                            # the camera centre: d . cam = -P[2, 3]
        for j, i in enumerate(rows.tolist()):
            pts[i] = (cam + 5e-4 * d + 1e-5 * ((j % 3) - 1) * rx + 1e-5 * ((j % 2) - 0.5) * ry).float()
    return case


def make(entry, V, C, n, Hf, Wf, aug, seed, B=1, blind=0, kind='full', cut=None, shallow=0):
    """host tensors of one launch for `entry` on prefix_spec.make_case's cameras and points.  cut: row at which sample 1 begins
    (B = 2) in place of make_case's even split.  The record carries vs (None: float points) and, for the window kernels, win"""
    case = PS.make_case(V, C, n, Hf, Wf, aug, seed, B=B, blind=blind)
    if cut is not None:
        assert B == 2
        case['coords'][:, 0] = (torch.arange(n) >= cut).int()
    if shallow:
        plant_shallow(case, shallow)
    case.update(entry=entry, vs=None, win=None, aug=aug, blind=blind)
    if entry in INTS:
        case['coords'][:, 1:] = torch.round(case['points'] / WS.VS).int()
        case['vs'] = WS.VS
    if entry in ('fwd_h', 'win_h'):
        case['feats'] = case['feats'].to(torch.bfloat16).float()                      # exact bf16 values
    if entry in ('win', 'win_h'):
        case['win'] = torch.tensor([[b, w] for b, w in enumerate(WS.windows(kind, B, V)[:, 1].tolist())], dtype=torch.int32)
    return case


def launch(dev, case, half=None, ldo_pad=8):
    """one launch (the step kernel: V launches on a running sum and count) into buffers with guard bands; returns the record:
    the case with device coords / feats as read, out (rows, C), pix (n, V), cnt (n) or (V, n)"""
    hip = _hip()
    P = hip.P
    entry = case['entry']
    V, C, n, Hf, Wf = (case[k] for k in ('V', 'C', 'n', 'Hf', 'Wf'))
    is_h = entry in ('fwd_h', 'win_h')
    half = is_h if half is None else half                  # half=False on an _h entry: the f32 sibling on the same values
    name = NAME[entry] if half == is_h else NAME[entry[:-2]]
    label = f'{name} V={V} C={C} n={n} B={case["B"]} {Hf}x{Wf} seed={case["seed"]}'
    coords, meta = case['coords'].to(dev), case['meta'].to(dev)
    points = case['points'].to(dev)
    feats = case['feats'].to(dev)
    if half:
        feats = feats.to(torch.bfloat16)
    ldo = C + ldo_pad
    rows = V * n if entry == 'prefix' else n
    ncnt = V * n if entry == 'prefix' else n

    def band_ok(obuf, r, what):
        b = obuf.clone()
        b[:r * ldo].view(r, ldo)[:, :C].fill_(SENT)
        assert bool((b == SENT).all()), f'{label}: {what} written outside columns [0, {C}) of its (rows {r}, ld {ldo}) buffer'

    if entry == 'step':
        sbuf = torch.full((n * C + 8,), SENT, dtype=torch.float32, device=dev)
        sbuf[:n * C] = 0.0
        nbuf = torch.full((n + 8,), ISENT, dtype=torch.int32, device=dev)
        nbuf[:n] = 0
        steps = []
        for t in range(V):
            m_t, f_t = W.step_meta(case['meta'], t).to(dev), W.step_feats(case['feats'], t).to(dev)
            obuf = torch.full((n * ldo + 8,), SENT, dtype=torch.float32, device=dev)
            pbuf = torch.full((n + 8,), ISENT, dtype=torch.int32, device=dev)
            hip.call(name, P(coords), P(points), n, P(m_t), m_t.shape[1], P(f_t), Hf, Wf, C, P(sbuf), P(nbuf), P(obuf), ldo, P(pbuf), _st())
            torch.cuda.synchronize()
            band_ok(obuf, n, f'step {t}')
            assert bool((pbuf[n:] == ISENT).all()) and bool((nbuf[n:] == ISENT).all()) and bool((sbuf[n * C:] == SENT).all()), \
                f'{label} step {t}: pix / nvalid / sum written past their end'
            steps.append(dict(out=obuf[:n * ldo].view(n, ldo)[:, :C].clone(), nvalid=nbuf[:n].clone(), pix=pbuf[:n].clone()))
        return W.assemble(dict(case, coords=coords, feats=feats), steps)
    obuf = torch.full((rows * ldo + 8,), SENT, dtype=torch.float32, device=dev)
    pbuf = torch.full((n * V + 8,), 12345, dtype=torch.int32, device=dev)                # non-negative garbage: every entry must be written
    cbuf = torch.full((ncnt + 8,), ISENT, dtype=torch.int32, device=dev)
    if entry in ('fwd', 'fwd_h'):
        args = (P(coords), n, case['vs'], P(meta), meta.shape[1], V)
    elif entry in ('win', 'win_h'):
        win = case['win'].to(dev)
        args = (P(coords), n, case['vs'], P(meta), meta.shape[1], V, P(win))
    else:
        args = (P(coords), P(points), n, P(meta), meta.shape[1], V)
    hip.call(name, *args, P(feats), Hf, Wf, C, P(obuf), ldo, P(pbuf), P(cbuf), _st())
    torch.cuda.synchronize()
    band_ok(obuf, rows, 'out')
    assert bool((pbuf[n * V:] == 12345).all()) and bool((cbuf[ncnt:] == ISENT).all()), f'{label}: pix / cnt written past their end'
    cnt = cbuf[:ncnt].view(V, n) if entry == 'prefix' else cbuf[:ncnt]
    return dict(case, coords=coords, feats=feats, out=obuf[:rows * ldo].view(rows, ldo)[:, :C].contiguous(), pix=pbuf[:n * V].view(n, V),
                cnt=cnt.contiguous())


def same(a, b, label):
    assert torch.equal(a['pix'], b['pix']) and torch.equal(a['cnt'], b['cnt']) and _bits_equal(a['out'], b['out']), label


def check(dev, case, stats, tally):
    """everything one case must satisfy; returns the record"""
    entry = case['entry']
    label = f'{NAME[entry]} V={case["V"]} C={case["C"]} n={case["n"]} B={case["B"]} {case["Hf"]}x{case["Wf"]} seed={case["seed"]}'
    rec = launch(dev, case)
    geo = G.geometry(case, dev, case['vs'])
    r = G.check_geometry(rec, dev, case['vs'], caps=True, geo=geo, label=label)
    if entry in ('prefix', 'step'):
        PS.check_prefix_fwd(rec, dev, stats, cls=f'{entry}_fwd')
    else:
        full = rec if rec['win'] is not None else dict(rec, win=G.full_windows(case['B'], case['V']))
        WS.check_win_fwd(full, dev, stats, cls=f'{entry}_fwd')
    same(rec, launch(dev, case), f'{label}: two runs differ')
    if entry in ('fwd_h', 'win_h'):
        same(rec, launch(dev, case, half=False), f'{label}: the f32 launch on the same (exact bf16) values differs')
    cov = G.coverage(case, geo, G._inside(rec, dev, case['n'], case['V']))
    for k, v in cov.items():
        tally[k] = tally.get(k, 0) + v
    tally['und_pairs'] = tally.get('und_pairs', 0) + r['und_pairs']
    tally['und_rows'] = tally.get('und_rows', 0) + r['und_rows']
    tally['pairs'] = tally.get('pairs', 0) + r['pairs']
    return rec


# seeds: base 9000 + 16 * index, moved up by BUMP[index] where the specification alone (no kernel) left the caps at the base seed, at
# the full or at the reduced n; tests/test_emu_fusion_geometry.py::test_seeds_stay_inside_the_caps holds every one of them
BUMP = {6: 1, 28: 1}


def grid(small):
    """[(entry, V, C, n, Hf, Wf, aug, seed, B, blind, kind, cut, shallow)]: per entry point every V and every C at least once; n, B, the
    op lists, the blind views and the map size rotate on counters of their own; the 60 x 80 map goes with the short view lists (the
    finer the map and the longer the list, the more pairs near a rounding boundary: the caps)"""
    big = 50 if small else 333
    cases = []
    CS = (1, 63, 64, 65, 128, 512)
    for entry in ENTRIES:
        Vs = (1, 2, 63, 64, 65, 66, 67, 70) if entry in ('fwd', 'fwd_h', 'fwd_pts') else ((5,) if entry == 'step' else (1, 2, 10, 63, 64))
        e = ENTRIES.index(entry)
        for j in range(max(len(Vs), len(CS)) + 2):
            i = len(cases)
            V, C = Vs[(j + e) % len(Vs)], CS[j % len(CS)]
            n = (big, 17, 16, 15, 1)[(j + e) % 5]
            B = 1 if n == 1 else (2, 3, 1, 2)[(j + 2 * e) % 4]
            aug = int((j + e) % 2 == 0)
            blind = min((0, 1, 3)[(j + e) % 3], V - 1)
            Hf, Wf = MAPS[2 if V <= 2 and j % 2 == 0 else (1 if V <= 10 or j % 3 == 0 else 0)]
            kind = ('full', 'asc', 'arb')[j % 3]
            cut, shallow = None, 0
            if j == len(CS):                                   # the sample boundary on a multiple of 16: no workgroup straddles
                n, B, cut = big, 2, 32
            if j == len(CS) + 1 and entry not in INTS:         # float points at 0 < qz < 1e-3 (no op list: the points are placed)
                aug, shallow, blind = 0, 3, 0
            cases.append((entry, V, C, n, Hf, Wf, aug, 9000 + 16 * i + BUMP.get(i, 0), B, blind, kind, cut, shallow))
    # once more per entry point: the longest view list on the largest n, three samples with different op lists, one blind view (and, for
    # the window kernels, the detector's ascending table on ten views)
    for entry in ENTRIES:
        V = 70 if entry in ('fwd', 'fwd_h', 'fwd_pts') else (5 if entry == 'step' else 64)
        more = [(V, 65, 5, 7, 'full')] + ([(10, 128, 15, 20, 'asc')] if entry in ('win', 'win_h') else [])
        for V, C, Hf, Wf, kind in more:
            cases.append((entry, V, C, big, Hf, Wf, 1, 9000 + 16 * len(cases) + BUMP.get(len(cases), 0), 3, 1, kind, None, 0))
    for entry in ENTRIES:
        mine = [c for c in cases if c[0] == entry]
        assert {c[2] for c in mine} == set(CS) and {c[6] for c in mine} == {0, 1} and {c[8] for c in mine} >= {1, 2}
        assert {c[3] for c in mine} == {1, 15, 16, 17, big}
    assert {c[8] for c in cases} == {1, 2, 3} and {c[9] for c in cases} == {0, 1, 3} and {(c[4], c[5]) for c in cases} == set(MAPS)
    assert {c[1] for c in cases if c[0] == 'fwd'} == {1, 2, 63, 64, 65, 66, 67, 70} and {c[1] for c in cases if c[0] == 'win'} == {1, 2, 10, 63, 64}
    return cases


def build(c):
    entry, V, C, n, Hf, Wf, aug, seed, B, blind, kind, cut, shallow = c
    return make(entry, V, C, n, Hf, Wf, aug, seed, B=B, blind=blind, kind=kind, cut=cut, shallow=shallow)


COVER = ('straddle', 'dead_with_pixel', 'invalid_with_pixel', 'no_pixel', 'behind', 'shallow')


def run_grid(dev, entries=ENTRIES):
    stats, tally, aligned = WS.Stats('geometry grid'), {}, 0
    for c in grid(_small(dev)):
        if c[0] not in entries:
            continue
        case = build(c)
        if c[11] is not None:
            assert G.straddles(case['coords']) == 0
            aligned += 1
        check(dev, case, stats, tally)
    print(stats.report())
    print('geometry grid:', tally, 'cases with the sample boundary on a multiple of 16:', aligned)
    return tally, aligned


@pytest.mark.parametrize('entry', ENTRIES)
def test_geometry_on_the_shape_grid(dev, entry):
    tally, aligned = run_grid(dev, (entry,))
    assert aligned > 0 and tally['straddle'] > 0 and tally['no_pixel'] > 0 and tally['invalid_with_pixel'] > 0, tally


def test_grid_coverage_from_the_specification():
    """the whole grid, from the specification alone (host, no launch): straddling workgroups, rows with a pixel but no valid view, invalid views with a pixel beside valid ones, views without a pixel, points behind a
    camera and points at 0 < qz < 1e-3 all occur, at the full and at the reduced n"""
    tally = {}
    for small in (False, True):
        for c in grid(small):
            case = build(c)
            geo = G.geometry(case, torch.device('cpu'), case['vs'])
            for k, v in G.coverage(case, geo, G._inside(case, torch.device('cpu'), case['n'], case['V'])).items():
                tally[(small, k)] = tally.get((small, k), 0) + v
    print(tally)
    assert all(tally[(small, k)] > 0 for small in (False, True) for k in COVER), tally


LATTICE = ((0.0, (1.0, 1.0)), (4.0, (0.5, 2.0)))


def lattice(entry, crop, sf):
    case = G.lattice_case(5, crop, sf, seed=31, ints=entry in INTS)
    case.update(entry=entry, vs=0.125 if entry in INTS else None, win=None)
    if entry in ('fwd_h', 'win_h'):
        case['feats'] = case['feats'].to(torch.bfloat16).float()
    if entry in ('win', 'win_h'):
        case['win'] = G.full_windows(3, 2)
    return case


@pytest.mark.parametrize('entry', ENTRIES)
def test_edge_lattice_is_exact(dev, entry):
    """u = 0, u = w, v = 0, v = h exactly (not valid, but with a pixel), every half-pixel tie (-0.5 -> column 0, size - 0.5 -> the even
    neighbour), depth 0 and depth -1; flip off (sample 0) and on (1), all five reverse ops (2); crop 0 / scale 1 and crop 4 / scale
    (0.5, 2).  No pair of the z != 0 rows is undecided, every intermediate of the z in {1, 2} rows is representable, and every
    entry equals the exact rule"""
    stats = WS.Stats(f'edge lattice, {entry}')
    for crop, sf in LATTICE:
        case = lattice(entry, crop, sf)
        geo = G.geometry(case, dev, case['vs'])
        nz, ex = case['nonzero_rows'].to(dev), case['exact_rows'].to(dev)
        assert int(geo['und'][nz].sum()) == 0, 'an undecided pair on the z != 0 rows of the lattice'
        assert bool(geo['exact'][ex].all()), 'an intermediate of an exact row is not representable in f32'
        assert bool((geo['u'][1][ex] == 0).all() and (geo['ix'][1][ex] == 0).all() and (geo['iy'][1][ex] == 0).all())
        u, v = geo['u'][0][ex], geo['v'][0][ex]
        ix, iy = geo['ix'][0][ex], geo['iy'][0][ex]
        for what, hit in (('u = 0', u == 0), ('u = w', u == 64), ('v = 0', v == 0), ('v = h', v == 32), ('column -0.5', ix == -0.5),
                          ('column size - 0.5', ix == 8.5), ('row -0.5', iy == -0.5), ('row size - 0.5', iy == 4.5),
                          ('an inner tie', (ix == 2.5) & (iy == 1.5))):
            assert bool(hit.any()), f'the lattice has no pair on {what}'
        on_edge = (u == 0) | (u == 64)
        assert bool((geo['pix'][ex][on_edge & (iy > 0) & (iy < 4)] >= 0).all()) and not bool(geo['valid'][ex][on_edge].any())
        rec = launch(dev, case)
        r = G.check_geometry(rec, dev, case['vs'], caps=True, geo=geo, label=f'lattice {entry} crop {crop}')
        pix, dec = rec['pix'].long(), geo['pix_dec']
        print(f'lattice {entry} crop {crop} scale {sf}: {int((pix != geo["pix"])[dec].sum())} mismatches of {int(dec.sum())} decided pix, '
              f'{r["und_pairs"]} undecided pairs')
        if entry in ('prefix', 'step'):
            PS.check_prefix_fwd(rec, dev, stats, cls=f'{entry}_fwd')
        else:
            WS.check_win_fwd(rec if rec['win'] is not None else dict(rec, win=G.full_windows(3, 2)), dev, stats, cls=f'{entry}_fwd')
        if not _small(dev):
            same(rec, launch(dev, case), f'lattice {entry}: two runs differ')
    print(stats.report())


def test_refusals_write_nothing(dev):
    """C = 513 returns -4 on all seven entry points; V = 65 returns -9 on the window and prefix ones; out, pix and cnt keep their
    sentinels"""
    hip = _hip()
    P = hip.P
    n = 20
    for V, C, want, entries in ((2, 513, -4, ENTRIES), (65, 32, -9, ('win', 'win_h', 'prefix'))):
        case = PS.make_case(min(V, 3), 32, n, 4, 5, 0, 5)
        coords, points = case['coords'].to(dev), case['points'].to(dev)
        meta = torch.zeros(1, PS.PROJ + 16 * V, device=dev)
        win = torch.tensor([[0, 1]], dtype=torch.int32, device=dev)
        feats = torch.zeros(V * 20 * C, device=dev)
        for entry in entries:
            out = torch.full((V * n, C), SENT, device=dev)
            ssum = torch.full((n, C), SENT, device=dev)
            pix = torch.full((n, V), ISENT, dtype=torch.int32, device=dev)
            cnt = torch.full((V, n), ISENT, dtype=torch.int32, device=dev)
            f = hip.raw(NAME[entry])
            if entry in ('fwd', 'fwd_h'):
                rc = f(P(coords), n, WS.VS, P(meta), meta.shape[1], V, P(feats), 4, 5, C, P(out), C, P(pix), P(cnt), _st())
            elif entry in ('win', 'win_h'):
                rc = f(P(coords), n, WS.VS, P(meta), meta.shape[1], V, P(win), P(feats), 4, 5, C, P(out), C, P(pix), P(cnt), _st())
            elif entry == 'step':
                rc = f(P(coords), P(points), n, P(meta), meta.shape[1], P(feats), 4, 5, C, P(ssum), P(cnt), P(out), C, P(pix), _st())
            else:
                rc = f(P(coords), P(points), n, P(meta), meta.shape[1], V, P(feats), 4, 5, C, P(out), C, P(pix), P(cnt), _st())
            torch.cuda.synchronize()
            assert rc == want, (entry, V, C, rc)
            assert bool((out == SENT).all()) and bool((ssum == SENT).all()) and bool((pix == ISENT).all()) and bool((cnt == ISENT).all()), entry
