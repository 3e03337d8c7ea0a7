"""embodiedscan_amd.eval.gather_results on two gloo ranks (CPU; the launch follows tests/test_host_logic.py): ragged tensors of uneven
lengths, one rank without any result, the rank-by-rank interleave and the cut to `size` that mmengine's collect_results applies to
the padded samples of the last batch."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _results(rank, n):
    """result i of a rank: tensors whose lengths and values say who made them (a zero-length one among them)"""
    out = []
    for i in range(n):
        g, p = (3 * i + rank) % 4, (5 * i + 2 * rank) % 7
        tag = 100 * rank + i
        out.append((torch.full((g, 9), float(tag)), torch.full((g,), tag, dtype=torch.int64), torch.full((p, 9), tag + 0.5),
                    torch.arange(p, dtype=torch.float32) + tag, torch.full((p,), tag, dtype=torch.int64)))
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def _worker():
    import torch.distributed as dist
    from embodiedscan_amd.eval import gather_results
    dist.init_process_group('gloo')
    rank = dist.get_rank()
    for counts, size in (((3, 2), 5), ((3, 2), 4), ((2, 3), None), ((0, 3), 3), ((2, 0), None), ((0, 0), None)):
        mine = _results(rank, counts[rank])
        got = gather_results(mine, size)
        per_rank = [_results(r, counts[r]) for r in range(2)]
        want = []
        for i in range(max(counts)):
            want += [per_rank[r][i] for r in range(2) if i < counts[r]]
        want = want if size is None else want[:size]
        assert len(got) == len(want), (counts, size, len(got), len(want))
        assert all(_same(a, b) for a, b in zip(got, want)), (counts, size)
    dist.destroy_process_group()
    print(f'rank {rank} ok')


def test_gather_results_two_gloo_ranks():
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', PYTHONPATH=ROOT)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2', '--master-addr', '127.0.0.1',
           '--master-port', '29617', os.path.abspath(__file__), '--gather-worker']
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count('ok') == 2


if __name__ == '__main__' and '--gather-worker' in sys.argv:
    sys.path.insert(0, ROOT)
    _worker()
