"""dev tool: many prompts per scan on one shared scene encoding, training side.

Kernel table (the decision rule of DESIGN section 3c): es_attn_kv_bwd against es_attn_bwd(B = 1) on the same operands at Lq = P * 256 for P in
{1, 4, 12, 64}, Lk = 3 148, H = 8, in both modes; es_rows_scatter_sum at the same P (L = Lk, Q = 256, C = 256) for the record.
Workload: the benchmark's grounding shape (full config, 12 prompts per step, 20 views of 480x640, bf16) on synthetic scans:
  train_step on 12 distinct scans (one prompt each) -- what training does today;
  train_step_shared at S x P = 12 x 1 (the same batch through the new path), 3 x 4 and 1 x 12;
for each ms per step and prompts per second.

One process; every form and shape is warmed up; workload samples are host wall times between device synchronisations, kernel samples
device-event times around --calls back-to-back launches; the forms are sampled in alternation --repeats times; median [min .. max] are
printed, the spread of one form between its repeats is the yardstick for a difference between two.  Each GPU step of the tool runs under
its own time limit (SIGALRM: the process ends there, nothing further is started) and the tool stops at the first failure.
  python tools/bench_shared_train.py [--json profiles/shared_train.json] [--skip-workload | --skip-kernels]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402

from bench_shared_scene import alternate, fmt, limit, sample, wall  # noqa: E402
from embodiedscan_amd import engine as E, hip, pipeline  # noqa: E402
from embodiedscan_amd.hip import P, call  # noqa: E402


def kernel_table(dev, args, out):
    Lk, C, H, Q = args.keys, 256, 8, 256
    g = torch.Generator().manual_seed(3)
    s = hip.stream()
    k, v = (torch.randn(Lk, C, generator=g).to(dev) for _ in range(2))
    for n_p in args.prompts:
        Lq = n_p * Q
        q, do = (torch.randn(Lq, C, generator=g).to(dev) for _ in range(2))
        for bf in (1, 0):
            mode = 'bf16' if bf else 'f32'
            kv = torch.empty(int(hip.raw('es_attn_kv_bytes')(H, Lk, bf)), dtype=torch.uint8, device=dev)
            o, lse = torch.empty(Lq, C, device=dev), torch.empty(H * Lq, device=dev)
            nws = int(hip.raw('es_attn_kv_bwd_workspace_bytes')(H, Lq, bf))
            ws = torch.empty(nws, dtype=torch.uint8, device=dev)
            delta = torch.empty(H * Lq, device=dev)
            ga = [torch.empty(n, C, device=dev) for n in (Lq, Lk, Lk)]
            gb = [torch.empty(n, C, device=dev) for n in (Lq, Lk, Lk)]

            def kv_bwd():
                call('es_attn_kv_bwd', P(q), C, P(k), C, P(v), C, P(o), C, P(do), C, P(lse), H, Lq, Lk, P(delta), P(ws), nws, P(ga[0]), C, P(ga[1]),
                     C, P(ga[2]), C, 0, bf, s)

            def plain():
                call('es_attn_bwd', P(q), C, P(k), C, P(v), C, P(o), C, P(do), C, P(lse), 1, H, Lq, Lk, 0, P(delta), P(gb[0]), C, P(gb[1]), C,
                     P(gb[2]), C, 0, bf, s)
            with limit(300, f'attention backward kernels at P = {n_p}, {mode}'):
                call('es_attn_kv_prepare', P(k), C, P(v), C, H, Lk, bf, P(kv), s)
                call('es_attn_kv_fwd', P(q), C, P(kv), H, Lq, Lk, P(o), C, P(lse), bf, s)
                for fn in (kv_bwd, plain):
                    sample(fn, 3)
                diff = max(float((a - b).abs().max()) for a, b in zip(ga, gb))
                row = alternate({'es_attn_kv_bwd': kv_bwd, 'es_attn_bwd_B1': plain}, args.repeats, lambda fn: sample(fn, args.calls))
            a, b = row['es_attn_kv_bwd'], row['es_attn_bwd_B1']
            spread = max(a['max_ms'] - a['min_ms'], b['max_ms'] - b['min_ms'])
            row.update(Lq=Lq, Lk=Lk, H=H, max_abs_diff=diff, gain_ms=round(b['median_ms'] - a['median_ms'], 4), spread_ms=round(spread, 4),
                       faster_beyond_spread=bool(b['median_ms'] - a['median_ms'] > spread))
            out['kernels'][f'attention backward P={n_p} {mode}'] = row
            print(f'attention backward Lq={Lq} Lk={Lk} {mode}: es_attn_kv_bwd {fmt(a)}; es_attn_bwd(B=1) {fmt(b)}; gain {row["gain_ms"]:.3f} ms, '
                  f'spread {row["spread_ms"]:.3f} ms, max |difference| {diff:.2e}', flush=True)
        idx = torch.stack([torch.randperm(Lk, generator=g)[:Q] for _ in range(n_p)]).int().to(dev)
        dy, dx = torch.randn(Lq, C, generator=g).to(dev), torch.empty(Lk, C, device=dev)
        tab = torch.empty(n_p * Lk, dtype=torch.int32, device=dev)

        def scatter():
            call('es_rows_scatter_sum', P(dy), C, P(idx), n_p, Q, Lk, C, P(dx), C, 0, P(tab), n_p * Lk, s)
        with limit(120, f'scatter-sum at P = {n_p}'):
            sample(scatter, 3)
            row = alternate({'es_rows_scatter_sum': scatter}, args.repeats, lambda fn: sample(fn, args.calls))
        out['kernels'][f'scatter-sum P={n_p}'] = dict(row, L=Lk, Q=Q, C=C)
        print(f'scatter-sum L={Lk} P={n_p} Q={Q} C={C}: {fmt(row["es_rows_scatter_sum"])}', flush=True)
    d = out['kernels'].get('attention backward P=12 bf16')
    if d is not None:
        out['decision'] = dict(rule='loss_shared calls es_attn_kv_bwd if it is faster than es_attn_bwd(B = 1) by more than the spread between repeats of '
                                    'one form at P = 12 in bf16', gain_ms=d['gain_ms'], spread_ms=d['spread_ms'],
                               use_es_attn_kv_bwd=d['faster_beyond_spread'])
        print(f'decision at P = 12, bf16: gain {d["gain_ms"]:.3f} ms against a spread of {d["spread_ms"]:.3f} ms -> '
              f'{"es_attn_kv_bwd" if d["faster_beyond_spread"] else "es_attn_bwd(B = 1)"}', flush=True)


def workload(dev, args, out):
    from embodiedscan_amd.config import build_detector, build_optim_wrapper, load_config
    from embodiedscan_amd.synth import make_grounding_sample, make_scan
    n = args.batch
    E.PRECISION[0] = 'bf16'
    with limit(900, 'building the grounder and its scans'):
        cfg = load_config(os.path.join(ROOT, 'configs', 'mv_grounding.py'))
        det = build_detector(cfg, device=dev, seed=0).to(dev)
        optim = build_optim_wrapper(cfg)
        scans = [make_scan(777 + i, n_views=20, augment=True, render_device=str(dev)) for i in range(n)]
        anns = [[make_grounding_sample(sc, seed=100 * i + p) for p in range(n)] for i, sc in enumerate(scans)]
        dscans = [pipeline.upload_scan(sc, dev) for sc in scans]
        torch.cuda.synchronize()
    forms = {f'train_step {n} scans x 1 prompt': lambda: det.train_step(pipeline.make_grounding_batch(dscans, [a[0] for a in anns]), optim)}
    shapes = [(S, n // S) for S in (n, max(n // 4, 1), 1)]
    for S, Pp in shapes:
        forms[f'train_step_shared {S} x {Pp}'] = (lambda S=S, Pp=Pp: det.train_step_shared(
            pipeline.make_shared_grounding_batch(dscans[:S], [a[:Pp] for a in anns[:S]]), optim))
    for name, fn in forms.items():
        with limit(600, f'warm-up of {name}'):
            for _ in range(args.warmup):                # (the first steps of a shape run long: lazy maps, allocator, graph captures)
                losses = fn()
            torch.cuda.synchronize()
            assert all(bool(torch.isfinite(v)) for v in losses.values()), f'{name}: non-finite loss'
    with limit(900, 'timing the train steps'):
        rows = alternate(forms, args.repeats, wall)
    out['workload'] = dict(prompts_per_step=n, views=20, precision='bf16', num_queries=det.num_queries, layers=det.decoder.num_layers,
                           attn_kv_bwd=bool(E.ATTN_KV_BWD[0]), tokens_per_scan=[int(x) for x in det.neck_3d.last['lens']], forms={})
    for name, r in rows.items():
        r['prompts_per_s'] = round(n / r['median_ms'] * 1e3, 1)
        out['workload']['forms'][name] = r
        print(f'{name}: {fmt(r)} per step = {r["prompts_per_s"]:.1f} prompts / s', flush=True)
    E.PRECISION[0] = 'f32'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--prompts', type=int, nargs='+', default=[1, 4, 12, 64])
    ap.add_argument('--keys', type=int, default=3148)
    ap.add_argument('--batch', type=int, default=12, help='prompts per step of the workload')
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=6)
    ap.add_argument('--skip-workload', action='store_true')
    ap.add_argument('--skip-kernels', action='store_true')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU fallback'
    dev = torch.device('cuda:0')
    out = dict(kernels={}, decision=None, workload=None)
    if not args.skip_kernels:
        kernel_table(dev, args, out)
    if not args.skip_workload:
        workload(dev, args, out)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
