"""tests/test_gpu_fusion_geometry.py on the CPU emulator (tests/emu): the same bodies under the `emulated` fixture of
tests/test_emu_product.py (random thread schedule; n = 50 in place of 333, every V and C kept) and under the ascending and the descending
schedule.  Before any kernel runs: the seeds of the grid stay inside the caps by the specification alone, the grid holds every
situation it must, and the specification agrees with oracle.model.batch_point_sample on the golden fixtures.  Then the checker
itself: a correct lattice record and a correct random record, with pix and cnt changed to what a kernel with ONE wrong rule would
have written (fusion_geom_spec.wrong_rule), must be rejected.
TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fusion_geom_spec as G
import test_gpu_fusion_geometry as T
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)

CPU = torch.device('cpu')


def _schedule(order):
    import build as emu_build
    lib = ctypes.CDLL(emu_build.build())
    lib.es_emu_set_schedule.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
    lib.es_emu_set_schedule(order, 4242)


def test_seeds_stay_inside_the_caps():
    """every case of the grid, at the full and at the reduced n, and the lattice: the caps hold by the specification alone"""
    worst = (0.0, 0.0)
    for small in (False, True):
        for c in T.grid(small):
            case = T.build(c)
            geo = G.geometry(case, CPU, case['vs'])
            up, ur, pairs, rows, ok = G.within_caps(geo, G._inside(case, CPU, case['n'], case['V']))
            assert ok, f'{c}: {up} of {pairs} pairs, {ur} of {rows} rows undecided'
            worst = (max(worst[0], up / pairs), max(worst[1], ur / rows))
    print(f'largest undecided share of a case: {worst[0]:.2e} of its pairs, {worst[1]:.2e} of its rows')
    for entry in ('fwd', 'fwd_pts'):
        for crop, sf in T.LATTICE:
            case = T.lattice(entry, crop, sf)
            geo = G.geometry(case, CPU, case['vs'])
            assert int(geo['und'][case['nonzero_rows']].sum()) == 0 and bool(geo['exact'][case['exact_rows']].all())


def test_grid_coverage_from_the_specification():
    T.test_grid_coverage_from_the_specification()


def test_spec_agrees_with_the_oracle(golden_dir):
    """the second yardstick: on the two golden fixtures (one sample, float points, f32 maps) the mean of the rows the specification
    names equals oracle.model.batch_point_sample on every decided row, within the sum bound (k + 1) u sum |f| / cnt of each side"""
    from embodiedscan_amd.models.layers.fusion_layers.point_fusion import build_fusion_meta
    from oracle import model as OM
    from test_gpu_fusion_losses import _meta_from
    for name in ('point_sample_plain', 'point_sample_aug'):
        d = np.load(os.path.join(golden_dir, name + '.npz'))
        meta = _meta_from(d)
        V = d['proj'].shape[0]
        meta['depth2img'] = dict(intrinsic=[np.eye(4, dtype=np.float32)] * V, extrinsic=[d['proj'][v] for v in range(V)])
        pts = torch.from_numpy(d['points']).float()
        feats = torch.from_numpy(d['feats'])
        ref = OM.batch_point_sample(meta, feats, pts, torch.from_numpy(d['proj']), torch.from_numpy(d['scale_factor']),
                                    torch.from_numpy(d['crop_offset']), bool(d['flip']), tuple(d['pad_shape']), tuple(d['img_shape']))
        Vn, C, H, W = feats.shape
        md = build_fusion_meta([meta], 'DEPTH', tuple(int(v) for v in d['pad_shape']), V)
        case = dict(V=V, Hf=H, Wf=W, coords=torch.zeros(len(pts), 4, dtype=torch.int32), points=pts, meta=md)
        geo = G.geometry(case, CPU)
        out, bnd, und = G.spec_out(geo, feats.permute(0, 2, 3, 1).reshape(1, Vn, H * W, C), case['coords'][:, 0], CPU)
        err = (ref.double() - out).abs()
        bad = (err > 2 * bnd) & ~und[:, None]
        print(f'{name}: {int(und.sum())} of {len(pts)} rows undecided; decided rows beyond the bound: {int(bad.any(1).sum())}; '
              f'non-zero rows {int((out != 0).any(1).sum())}')
        assert not bool(bad.any()) and 100 * int(und.sum()) <= len(pts) and int((out != 0).any(1).sum()) > 20


@pytest.mark.parametrize('entry', T.ENTRIES)
def test_geometry_on_the_shape_grid(emulated, entry):  # noqa: F811
    T.test_geometry_on_the_shape_grid(emulated, entry)


@pytest.mark.parametrize('entry', T.ENTRIES)
def test_edge_lattice_is_exact(emulated, entry):  # noqa: F811
    T.test_edge_lattice_is_exact(emulated, entry)


def test_refusals_write_nothing(emulated):  # noqa: F811
    T.test_refusals_write_nothing(emulated)


def test_point_sample_vs_reference_golden(emulated, golden_dir):  # noqa: F811
    """tests/test_gpu_fusion_losses.py's golden comparison: no decided row differs from the oracle"""
    import test_gpu_fusion_losses as L
    L.point_sample_golden(emulated, golden_dir)


def test_point_sample_bwd_is_an_ordered_gather(emulated):  # noqa: F811
    """tests/test_gpu_fusion_losses.py's base backward, held per element"""
    import test_gpu_fusion_losses as L
    L.point_sample_bwd_ordered_gather(emulated)


@pytest.mark.parametrize('order', [0, 1])
def test_geometry_under_other_schedules(emulated, order):  # noqa: F811
    """one straddling case per entry point under the ascending and the descending thread schedule"""
    _schedule(order)
    stats, tally = T.WS.Stats(f'schedule {order}'), {}
    for entry in T.ENTRIES:
        c = next(c for c in T.grid(True) if c[0] == entry and c[8] >= 2 and c[3] >= 15 and c[11] is None)
        T.check(emulated, T.build(c), stats, tally)
    print(stats.report())
    print(tally)
    assert tally['straddle'] > 0


def _rejected(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError(f'the checker accepted {what}')


def _planted(rec, geo, pix_w, valid_w):
    """the record with the entries a wrong rule changes: pix where the wrong rule's differs from the specification's on a decided pair,
    cnt moved by the change in the number of valid views over the decided pairs; and how many decided entries changed"""
    dp = geo['pix_dec'] & (pix_w != geo['pix'])
    dv = geo['valid_dec'] & (valid_w != geo['valid'])
    pix = torch.where(dp, pix_w, rec['pix'].long()).int()
    cnt = (rec['cnt'].long() + (dv & valid_w).sum(1) - (dv & ~valid_w).sum(1)).int()
    return dict(rec, pix=pix, cnt=cnt), int(dp.sum()), int(dv.sum())


def test_checker_rejects_wrong_rules(emulated):  # noqa: F811
    """records of es_point_sample_fwd_pts: the lattice (crop 4, scale (0.5, 2); samples with flip off, on, and the five reverse ops) and
    a random case (three samples with different op lists, flip and crop on, a blind view, straddling workgroups)"""
    dev = emulated
    lat = T.lattice('fwd_pts', 4.0, (0.5, 2.0))
    rnd = T.make('fwd_pts', 3, 4, 200, 15, 20, 1, 9000, B=3, blind=1)
    recs = []
    for case in (lat, rnd):
        rec = T.launch(dev, case)
        geo = G.geometry(case, dev)
        G.check_geometry(rec, dev, geo=geo, caps=False)
        recs.append((case, rec, geo))
    assert G.straddles(rnd['coords']) > 0 and G.straddles(lat['coords']) > 0
    for rule in G.RULES:
        touched = 0
        for case, rec, geo in recs:
            pix_w, valid_w = G.wrong_rule(case, dev, rule)
            bad, dp, dv = _planted(rec, geo, pix_w, valid_w)
            print(f'{rule}: {dp} decided pix and {dv} decided valid flags change (n = {case["n"]})')
            if dp + dv:
                touched += 1
                _rejected(lambda: G.check_geometry(bad, dev, geo=geo, caps=False), f'the outputs of a kernel with the wrong rule {rule}')
        assert touched, f'{rule} changes no decided entry of either record'
    # the rules that only show ON an edge must be caught on the lattice
    for rule in ('u_ge_0', 'u_le_w', 'v_ge_0', 'v_le_h', 'qz_ge_0', 'half_up'):
        pix_w, valid_w = G.wrong_rule(lat, dev, rule)
        _, dp, dv = _planted(recs[0][1], recs[0][2], pix_w, valid_w)
        assert dp + dv > 0, f'{rule} changes nothing on the lattice'
    for case, rec, geo in recs:
        i = int(torch.nonzero(geo['valid_dec'].all(1))[0])
        for d in (1, -1):
            c2 = rec['cnt'].clone()
            c2[i] += d
            _rejected(lambda: G.check_geometry(dict(rec, cnt=c2), dev, geo=geo, caps=False), 'a cnt off by one')
        hit = torch.nonzero(geo['pix_dec'] & (geo['pix'] >= 0) & (geo['pix'] % case['Wf'] < case['Wf'] - 1))[0]
        p2 = rec['pix'].clone()
        p2[int(hit[0]), int(hit[1])] += 1
        _rejected(lambda: G.check_geometry(dict(rec, pix=p2), dev, geo=geo, caps=False), 'a decided pix moved by one column')
