"""embodiedscan_amd.eval.gather_results on the row layouts of GroundingMetric and OccupancyMetric, on two gloo ranks (CPU; the launch
follows tests/test_det_metric_gather.py): (hit (1,) int32, flags (1,) uint8) pairs, (1, 3C) int32 confusion rows and the ragged
(boxes (n,9) f32, scores (n) f32) pairs of format_only, with uneven counts per rank, one rank empty and a `size` cut.

Interleaving rule (what mmengine's collect_results does with the padded samples of the last batch): the gathered list is rank 0's
first result, rank 1's first, rank 0's second, rank 1's second, ...; a rank that has run out is passed over; `size` keeps the first
`size` entries of that list, None keeps all.  Dtypes and trailing shapes survive the trip."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3 = 3 * 81


def _results(kind, rank, n):
    """result i of a rank, with values that say who made it"""
    out = []
    for i in range(n):
        tag = 100 * rank + i
        if kind == 'ground':
            out.append((torch.tensor([tag], dtype=torch.int32), torch.tensor([(rank + 3 * i) % 8], dtype=torch.uint8)))
        elif kind == 'occ':
            out.append((torch.arange(C3, dtype=torch.int32).reshape(1, C3) * 1000 + tag,))
        else:
            k = (7 * i + 5 * rank) % 21                       # 0 .. 20 saved boxes
            out.append((torch.full((k, 9), tag + 0.5), torch.arange(k, dtype=torch.float32) + tag))
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _worker():
    import torch.distributed as dist
    from embodiedscan_amd.eval import gather_results
    dist.init_process_group('gloo')
    rank = dist.get_rank()
    for kind in ('ground', 'occ', 'saved'):
        for counts, size in (((3, 2), 5), ((3, 2), 4), ((2, 5), None), ((0, 3), 2), ((4, 0), None), ((0, 0), 3)):
            got = gather_results(_results(kind, rank, counts[rank]), size)
            per_rank = [_results(kind, r, counts[r]) for r in range(2)]
            want = []
            for i in range(max(counts)):
                want += [per_rank[r][i] for r in range(2) if i < counts[r]]
            want = want if size is None else want[:size]
            assert len(got) == len(want), (kind, counts, size, len(got), len(want))
            assert all(_same(a, b) for a, b in zip(got, want)), (kind, counts, size)
    dist.destroy_process_group()
    print(f'rank {rank} ok')


def test_gather_results_on_the_row_layouts_two_gloo_ranks():
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', PYTHONPATH=ROOT)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
           '--master-port', '29627', os.path.abspath(__file__), '--gather-worker']
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count('ok') == 2


if __name__ == '__main__' and '--gather-worker' in sys.argv:
    sys.path.insert(0, ROOT)
    _worker()
