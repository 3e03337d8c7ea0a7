"""Specification of the one-view step of the prefix fusion (csrc/fusion.hip: es_point_sample_step_fwd_pts), the kernel behind the
walk sessions (EmbodiedOccPredictor.open_walk): a running (n, C) sum and (n) valid-view count advanced by one view per call.  Used by
tests/test_gpu_walk_step.py (MI355X) and tests/test_emu_walk_step.py (the same bodies on the CPU emulator, plus mutated records the
checker must reject).

A walk of T steps from sum = 0, nvalid = 0 is held to three statements per step t:
  (a) out, nvalid and pix are bit-equal to row block t, cnt[t] and column t of es_point_sample_prefix_fwd_pts on views 0 .. t
      (same_as_prefix; the test bodies make that launch);
  (b) the T step outputs, laid out as ONE record of the prefix layout (assemble: out (T n, C), pix (n, T), cnt (T, n)), pass
      prefix_spec.check_prefix_fwd -- the f64 bound (k + 1) u sum |f| / cnt of tests/prefix_spec.py, so the check is not only HIP
      against HIP;
  (c) two walks from zero state are bit-equal (the test bodies).
The per-step meta block is the case's header with the ONE projection matrix of view t (step_meta): what
build_fusion_meta(..., n_views=1) makes of frame t's matrices."""
import torch

import prefix_spec as S
from prefix_spec import PROJ, Stats  # noqa: F401

__all__ = ['Stats', 'step_meta', 'step_feats', 'assemble', 'check_walk', 'same_as_prefix', 'grid']


def step_meta(meta, t, pad=4):
    """(B, 32 + 16 + pad) one-view meta rows of step t from the (B, 32 + 16 V + ..) rows of a prefix_spec case"""
    out = torch.zeros(meta.shape[0], PROJ + 16 + pad, dtype=torch.float32)
    out[:, :PROJ] = meta[:, :PROJ]
    out[:, PROJ:PROJ + 16] = meta[:, PROJ + 16 * t:PROJ + 16 * (t + 1)]
    return out


def step_feats(feats, t):
    """(B Hf Wf, C) sample-major map of frame t from the (B, V, Hf Wf, C) maps of a prefix_spec case"""
    return feats[:, t].reshape(-1, feats.shape[-1]).contiguous()


def assemble(case, steps):
    """steps: [dict(out (n, C) f32, nvalid (n) int, pix (n) int)] of steps 0 .. T-1 -> the record check_prefix_fwd reads"""
    T = len(steps)
    assert T == case['V']
    return dict(case, out=torch.cat([s['out'] for s in steps]), pix=torch.stack([s['pix'] for s in steps], 1).contiguous(),
                cnt=torch.stack([s['nvalid'] for s in steps]).contiguous())


def check_walk(case, steps, dev, stats, cls='walk_step'):
    """(b): the assembled walk against the f64 specification of the prefix fusion"""
    rec = assemble(case, steps)
    return S.check_prefix_fwd(dict(rec, coords=rec['coords'].to(dev), feats=rec['feats'].to(dev)), dev, stats, cls=cls)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_as_prefix(label, steps, pre):
    """(a): pre = dict(out (T n, C), pix (n, T), cnt (T, n)) of the prefix kernel on the same views"""
    n = steps[0]['out'].shape[0]
    for t, s in enumerate(steps):
        assert torch.equal(s['nvalid'], pre['cnt'][t]), f'{label}: nvalid after step {t} differs from cnt[{t}] of the prefix kernel'
        assert torch.equal(s['pix'], pre['pix'][:, t]), f'{label}: pix of step {t} differs from column {t} of the prefix kernel'
        assert _bits_equal(s['out'], pre['out'][t * n:(t + 1) * n]), f'{label}: out of step {t} is not bit-equal to row block {t} of the prefix kernel'


def grid(small):
    """(T, C, n, B, blind, cluster, aug, ldo_pad): T in {1, 3, 10} x C in {32, 40, 256, 512} x n in {1, 37, 150} (small, the emulator: 1, 37,
    50), Hf, Wf = 5, 7.  B = 2 at every n = 37 with C in {40, 512}: rows 0 .. 18 are sample 0, so the workgroup of rows 16 .. 31 straddles
    the sample boundary and reads its meta block from global memory.  blind, cluster, aug and ldo = C + 8 rotate on counters of their own"""
    cases, i = [], 0
    for T in (1, 3, 10):
        for C in (32, 40, 256, 512):
            for n in (1, 37, 50 if small else 150):
                B = 2 if (n == 37 and C in (40, 512)) else 1
                blind = min((0, 1, 2)[i % 3], T - 1)
                cluster = ((20 if small else 70) if i % 2 == 0 else 9) if n > 37 else 0
                cases.append((T, C, n, B, blind, cluster, int(i % 4 in (1, 2)), (8, 0)[i % 5 == 3]))
                i += 1
    assert {c[6] for c in cases} == {0, 1} and any(c[3] == 2 for c in cases) and any(c[4] > 0 for c in cases)
    assert any(c[5] > 0 for c in cases) and any(c[7] == 8 for c in cases) and any(c[7] == 0 for c in cases)
    return cases
