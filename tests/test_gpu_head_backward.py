"""The FCAF3D head's backward without the work its result does not need (engine.HEAD_BWD_FUSED), on the device.
Kernel level -- the cases of tests/test_emu_head_backward.py (tests/head_backward_cases.py): es_gen_transpose_wgrad_bf16 against the
eight per-tap launches (bits), es_focal_loss_clear against es_focal_loss (bits, and exact zeros around the class block).
Step level -- the head's loss and backward on a small synthetic input (2 samples, 4 levels, the finest above the streaming
weight-gradient kernel's 4 096 rows) with the switch off and on: the same head-output gradients and parameter gradients bit for bit (the
bias gradient also within the column-sum bound of f64), the zero fill replaced by the clearing focal launch, no prune score for level 0."""
import numpy as np
import pytest
import torch

import head_backward_cases as cases

pytestmark = [pytest.mark.gpu]


class _Buf:
    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.shape, self.dtype = a.shape, a.dtype
        # (torch has no uint16 arithmetic: the bf16 bit patterns travel as int16 of the same bytes)
        self.t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a.copy()).to('cuda:0')
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == 0

    def get(self):
        return self.t.cpu().numpy().view(self.dtype).reshape(self.shape)


class _Backend:
    def fn(self, name):
        from embodiedscan_amd import hip
        return hip.raw(name)

    def put(self, a):
        return _Buf(a)

    def launches(self):
        return None                                          # (launch counts are the emulator's to check)


@pytest.fixture(scope='module')
def be():
    torch.cuda.current_stream().synchronize()
    return _Backend()


def test_fused_generative_weight_gradient_equals_the_per_tap_launches(be):
    todo = cases.gen_wgrad_cases(be)
    split = [cases.check_gen_wgrad(be, *c, seed=i) for i, c in enumerate(todo)]
    assert todo[2][0] > 1 and split[2] > 0                   # the last case splits its rows through the workspace
    cases.check_gen_wgrad_unserved(be)


def test_fused_generative_weight_gradient_on_the_128_tile(be):
    """k_spconv_wgrad_bf16_big<0, 0> (library option 24 = 0 takes the whole-stage 64 x 64 kernel out of the plan): one slice with
    accumulation, rows split over two slices"""
    assert be.fn('es_set_option')(24, 0) == 0
    try:
        assert cases.check_gen_wgrad(be, 512, 128, 128, 0, 1, seed=10) == 0
        assert cases.check_gen_wgrad(be, 600, 256, 128, 8, 0, seed=11) > 0
    finally:
        be.fn('es_set_option')(24, 256)


@pytest.mark.parametrize('N', [5, 4 * 2048 + 3])
def test_focal_loss_clear_equals_focal_loss_and_clears_the_rest(be, N):
    cases.check_focal_clear(be, N)


# ---------------------------------------------------------------------------------------------------------------- the head's step
IN_CHANNELS = (256, 512, 512, 256)      # up-blocks 256 -> 512 on ~12 rows (not served: the per-tap launches), 512 -> 512 and 512 -> 256 (one launch)
WATCHED = ('es_colsum', 'es_row_max', 'es_rows_wgrad1_bf16', 'es_focal_loss', 'es_focal_loss_clear')


def _head_step(fused, head, arena, sets, feats, gts, event):
    from embodiedscan_amd import engine as E, hip
    from embodiedscan_amd.sparse import SparseTensor
    E.HEAD_BWD_FUSED[0] = fused
    E.TAPE.clear()
    E.WEIGHT_VERSION[0] += 1
    E.new_grad_epoch()
    arena.grad.zero_()
    records = []
    hip.PROFILE = dict(names=set(WATCHED), records=records, event=event)
    try:
        levels = head._levels([SparseTensor(cs, E.Var(f.clone())) for cs, f in zip(sets, feats)])
        losses = head.loss_by_levels(levels, gts)
        seeds = [lv['ho'].g for lv in levels]
        E.TAPE.backward()
        torch.cuda.synchronize()
    finally:
        hip.PROFILE = None
    return dict(losses={k: float(v) for k, v in losses.items()}, seeds=[s.clone() for s in seeds], rows=[lv['cs'].n for lv in levels],
                grads={k: v.clone() for k, v in arena.g.items()}, calls=[(r[0], r[3]) for r in records])


def test_head_loss_and_backward_with_the_switch_off_and_on():
    _check_head(torch.device('cuda:0'), IN_CHANNELS, lambda: torch.cuda.Event(enable_timing=True))


def _check_head(dev, IN_CHANNELS, event):
    from embodiedscan_amd import engine as E, sparse
    from embodiedscan_amd.models.dense_heads.fcaf3d_head import FCAF3DHeadRotMat
    from embodiedscan_amd.params import ParamArena, fcaf3d_head_specs
    vs = 0.1
    g = torch.Generator().manual_seed(5)
    # sample 0 fills 2 x 2 x 2 cells of the coarsest level (8 voxels wide), sample 1 2 x 2 x 1: 12 rows there, 8 x as many per finer level
    pts = [(torch.rand(4000, 3, generator=g) * torch.tensor(ext) * vs).to(dev) for ext in ((16., 16., 16.), (16., 16., 8.))]
    sets = [sparse.voxelize(pts, vs)[0]]
    for _ in range(3):
        sets.append(sets[-1].strided(2))
    feats = [torch.randn(cs.n, c, generator=g).to(dev) for cs, c in zip(sets, IN_CHANNELS)]
    arena = ParamArena(fcaf3d_head_specs(in_channels=IN_CHANNELS, out_channels=128, n_classes=284), seed=0).to(dev)
    head = FCAF3DHeadRotMat(num_classes=284, in_channels=IN_CHANNELS, out_channels=128, num_reg_outs=12, voxel_size=vs,
                            pts_prune_threshold=100000, pts_assign_threshold=27, pts_center_threshold=18).bind(arena)
    gts = [(torch.tensor([[0.8, 0.8, 0.8, 1.0, 1.2, 0.9, 0.3, 0., 0.], [0.4, 1.1, 0.5, 0.5, 0.6, 0.7, 0., 0., 0.]]), torch.tensor([3, 283])),
           (torch.tensor([[0.8, 0.7, 0.4, 1.1, 0.9, 0.6, -0.2, 0., 0.]]), torch.tensor([0]))]
    res = {}
    old = E.HEAD_BWD_FUSED[0], E.PRECISION[0]
    E.PRECISION[0] = 'bf16'
    try:
        for fused in (False, True):
            res[fused] = _head_step(fused, head, arena, sets, feats, gts, event)
    finally:
        E.HEAD_BWD_FUSED[0], E.PRECISION[0] = old
    off, on = res[False], res[True]
    rows = on['rows']
    print('rows per level', rows, 'losses', on['losses'])
    assert rows == off['rows'] and rows[0] > 4096 and all(r < 4096 for r in rows[1:]), rows
    assert on['losses'] == off['losses'] and all(np.isfinite(v) for v in on['losses'].values()) and on['losses']['loss_bbox'] > 0
    for a, b in zip(on['seeds'], off['seeds']):
        assert torch.equal(a, b)
    bias = 'bbox_head.head_out.bias'
    for k in off['grads']:
        assert torch.equal(on['grads'][k], off['grads'][k]), (k, float((on['grads'][k] - off['grads'][k]).abs().max()))
    # bias gradient: column sums of the head-output gradients over all levels, from column 13 on
    want = sum(s.double().sum(0) for s in off['seeds'])[13:].cpu()
    bound = 2e-6 * sum(float(s[:, 13:].abs().sum(0).max()) for s in off['seeds'])
    for name, r in (('off', off), ('on', on)):
        got = r['grads'][bias].double().cpu()
        err = float((got[13:] - want).abs().max())
        print(f'head bias gradient, switch {name}: |got - f64| max {err:.3g}, bound {bound:.3g}')
        assert err <= bound and not got[:13].any()
    # the launches: es_colsum / es_row_max carry their row count as third argument
    def count(r, name, n=None):
        return sum(1 for nm, args in r['calls'] if nm == name and (n is None or args[2] == n))
    for r in (off, on):                                     # (the bias gradient stays es_colsum's: see DESIGN.md section 7)
        assert count(r, 'es_colsum') == 4 and count(r, 'es_rows_wgrad1_bf16') == 1
    assert count(off, 'es_row_max', rows[0]) == 0 and count(off, 'es_row_max') == 3      # (the finest level's score has no reader: never launched)
    assert count(off, 'es_focal_loss_clear') == 0 and count(off, 'es_focal_loss') > 0
    assert count(on, 'es_row_max', rows[0]) == 0 and count(on, 'es_row_max') == 3
    assert count(on, 'es_focal_loss') == 0 and count(on, 'es_focal_loss_clear') == count(off, 'es_focal_loss')
