"""k_focal_inflight (es_losses_set_option 40 = 1, the default: a lane loads its five logits of a row before the first expf and the
wave keeps the next row's loads in flight) against k_focal (40 = 0): the same arithmetic in the same order, so the loss scalar, the
whole gradient matrix -- the class block, the `lead` / `tail` columns the launch clears, and every column it must not touch -- and the
`partial` buffer must be IDENTICAL bit for bit.  N covers one row, a whole and a ragged workgroup, and the second and third trip of the
capped grid (2048 workgroups x 4 rows) with odd counts for the two-row pairing; C covers one class, the 64-lane edges, the shipped 284,
the five-slot limit 320 and 321, which keeps the loop kernel."""
import pytest
import torch

pytestmark = pytest.mark.gpu
PITCH, COL0 = 320, 13


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize('C', [1, 64, 65, 284, 320, 321])
@pytest.mark.parametrize('N', [1, 4, 5, 8193, 16385])
def test_inflight_kernel_is_bit_identical_to_the_loop_kernel(N, C):
    from embodiedscan_amd import hip
    from embodiedscan_amd.hip import P
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    opt = hip.raw('es_losses_set_option')
    g = torch.Generator().manual_seed(1000 * N + C)
    pitch = max(PITCH, COL0 + C + 23)                     # (C = 321 does not fit the 320-column rows of the head)
    logits = (torch.randn(N, pitch, generator=g) * 4).to(dev)
    labels = torch.randint(0, C, (N,), generator=g, dtype=torch.int32)
    kind = torch.randint(0, 4, (N,), generator=g)
    labels[kind == 0] = -1                                # background
    labels[kind == 1] = C + (N % 3)                       # past the classes: no positive column
    labels[N // 2] = 0
    labels[N - 1] = C - 1
    if N >= 4:
        labels[0], labels[1] = -1, C
    labels = labels.to(dev)
    avg = torch.tensor([37.5], device=dev)
    assert opt(41, 0) == -2
    try:
        for lead, tail in ((13, 23), (0, 0)):
            for gamma in (2.0, 1.5):
                for with_grad in (True, False):
                    out = {}
                    for on in (0, 1):
                        assert opt(40, on) == 0
                        grad = torch.full((N, pitch), 123.25, device=dev)
                        partial = torch.full((2048,), -5.0, dtype=torch.float64, device=dev)
                        loss = torch.tensor([0.625], device=dev)
                        if with_grad:
                            rc = hip.raw('es_focal_loss_clear')(logits.data_ptr() + 4 * COL0, pitch, P(labels), N, C, gamma, 0.25, P(avg), 0.75,
                                                                grad.data_ptr() + 4 * COL0, pitch, P(partial), P(loss), lead, tail, st)
                        else:
                            rc = hip.raw('es_focal_loss')(logits.data_ptr() + 4 * COL0, pitch, P(labels), N, C, gamma, 0.25, P(avg), 0.75,
                                                          0, 0, P(partial), P(loss), st)
                        assert rc == 0
                        torch.cuda.synchronize()
                        out[on] = (loss, grad, partial)
                    for a, b, what in zip(out[1], out[0], ('loss', 'gradient matrix', 'partial sums')):
                        assert torch.equal(_bits(a), _bits(b)), (what, lead, tail, gamma, with_grad)
                    loss, grad, partial = out[1]
                    assert torch.isfinite(loss).all() and float(loss) != 0.625
                    if with_grad:                         # written: [COL0 - lead, COL0 + C + tail), everything else untouched
                        lo, hi = COL0 - lead, COL0 + C + tail
                        assert (grad[:, :lo] == 123.25).all() and (grad[:, hi:] == 123.25).all()
                        assert (grad[:, lo:COL0] == 0).all() and (grad[:, COL0 + C:hi] == 0).all()
                        assert (grad[:, COL0:COL0 + C] != 123.25).all()
                    else:
                        assert (grad == 123.25).all()
    finally:
        opt(40, 1)
