"""dev tool: the grounder's frozen text encoder, transformers module (eager / captured graph replay) against text.HipTextEncoder (bf16 / f32),
at roberta-base shapes, and the 12-scan grounding train step with either implementation.  One process; every form is warmed up; a
sample is the device-event time around `--calls` back-to-back calls; the forms are sampled in alternation `--repeats` times; median and
min .. max are printed.  Each step runs under its own time limit (SIGALRM: the process ends there, nothing further is started).
  python tools/bench_text_encoder.py [--layers 12] [--no-step] [--step-only torch|hip] [--json PATH]
--step-only IMPL: only the grounding step with that implementation (the run to put under a kernel trace: does a library GEMM remain?)"""
import argparse
import json
import math
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from embodiedscan_amd import engine as E  # noqa: E402
from embodiedscan_amd.text import HipTextEncoder, TextGraph, build_text_encoder  # noqa: E402


class limit:
    """`with limit(seconds, what):` -- the step's own time limit"""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def _fire(self, *_):
        print(f'TIME LIMIT: {self.what} did not finish in {self.seconds} s; stopping here', flush=True)
        os._exit(124)

    def __enter__(self):
        signal.signal(signal.SIGALRM, self._fire)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def sample(fn, calls, stream=None):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def summarise(xs):
    return dict(median_ms=round(statistics.median(xs), 4), min_ms=round(min(xs), 4), max_ms=round(max(xs), 4), samples=len(xs))


def encoder_table(dev, args, out):
    cfg = dict(num_hidden_layers=args.layers)
    with limit(240, 'building the encoders'):
        module = build_text_encoder(cfg, seed=0).to(dev)
        enc = HipTextEncoder.from_module(module, dev)
        torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.Generator().manual_seed(1)
    for (B, T) in ((12, 16), (12, 32), (12, 64)):
        mask = torch.ones((B, T), dtype=torch.long)
        for b in range(B):
            mask[b, T - (b % 7):] = 0
        ids = torch.where(mask.bool(), torch.randint(3, 50000, (B, T), generator=g), torch.ones((B, T), dtype=torch.long)).to(dev)
        mask = mask.to(dev)

        def eager():
            with torch.no_grad():
                return module(input_ids=ids, attention_mask=mask).last_hidden_state

        def hip_in(mode):
            def run():
                E.PRECISION[0] = mode
                try:
                    return enc(ids, mask)
                finally:
                    E.PRECISION[0] = 'f32'
            return run

        with limit(120, f'capturing the graph for {(B, T)}'):
            tg = TextGraph(module, B, T, dev, side)
        forms = [('torch eager', eager, None), ('torch graph replay', lambda: tg.run(ids, mask), side), ('hip bf16', hip_in('bf16'), None),
                 ('hip f32', hip_in('f32'), None)]
        with limit(120, f'warm-up and agreement at {(B, T)}'):
            ref = eager().double()
            for name, fn, st in forms:
                for _ in range(3):
                    sample(fn, 2, st)
            torch.cuda.synchronize()
            agree = {m: float((hip_in(m)().double() - ref).abs().max()) for m in ('f32', 'bf16')}
            torch.cuda.synchronize()
        times = {name: [] for name, _, _ in forms}
        with limit(300, f'timing at {(B, T)}'):
            for _ in range(args.repeats):
                for name, fn, st in forms:              # alternating: a drift of the machine reaches every form alike
                    times[name].append(sample(fn, args.calls, st))
        row = {name: summarise(xs) for name, xs in times.items()}
        row['max_abs_diff_vs_torch_f32'] = agree
        out['encoder'][f'B={B} T={T}'] = row
        print(f'encoder B={B} T={T} ({args.layers} layers): ' + '; '.join(
            f'{n} {r["median_ms"]:.3f} ms [{r["min_ms"]:.3f} .. {r["max_ms"]:.3f}]' for n, r in row.items() if n != 'max_abs_diff_vs_torch_f32')
            + f'; max |hip - torch f32|: f32 {agree["f32"]:.2e}, bf16 {agree["bf16"]:.2e}', flush=True)


def grounding_step(dev, args, out):
    """configs/mv_grounding.py as bench.py runs it (12 scans x 20 views, bf16), inputs resident on the device; ONE detector, its text
    encoder switched between the module and its HipTextEncoder conversion (identical weights), blocks of steps in alternation"""
    from embodiedscan_amd import pipeline
    from embodiedscan_amd.config import build_detector, build_optim_wrapper, load_config
    from embodiedscan_amd.synth import make_grounding_sample, make_scan
    E.PRECISION[0] = 'bf16'
    with limit(600, 'building the grounder and its batch'):
        cfg = load_config(os.path.join(ROOT, 'configs', 'mv_grounding.py'))
        det = build_detector(cfg, device=dev, seed=0).to(dev)
        optim = build_optim_wrapper(cfg)
        impls = {'torch': det.text_encoder}
        impls['hip'] = HipTextEncoder.from_module(det.text_encoder, dev)
        dscans = []
        for i in range(args.batch):
            sc = make_scan(777 + i, n_views=20, augment=True, render_device=str(dev))
            a = make_grounding_sample(sc, seed=i)
            dscans.append(pipeline.upload_scan(dict(sc, text=a['text'], tokens_positive=a['tokens_positive'], gt_boxes=a['gt_boxes'],
                                                    gt_labels=a['gt_labels']), dev))
        torch.cuda.synchronize()
    names = [args.step_only] if args.step_only else ['torch', 'hip']

    def use(name):
        det.text_encoder, det.text_encoder_impl = impls[name], name

    def block(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            losses = det.train_step(pipeline.make_grounding_batch(dscans), optim)
        e1.record()
        e1.synchronize()
        assert all(math.isfinite(float(v)) for v in losses.values()), losses
        return e0.elapsed_time(e1) / n

    for name in names:
        with limit(600, f'warm-up steps with the {name} encoder'):
            use(name)
            block(8 if name == names[0] else 4)
    times = {n: [] for n in names}
    for r in range(args.step_rounds):
        for name in names:
            with limit(300, f'timed steps with the {name} encoder'):
                use(name)
                block(1)                               # (the switch itself: first step after it is not timed)
                times[name].append(block(args.step_block))
    T = int(det.last_text['mask'].shape[1])
    out['grounding_step'] = dict({n: summarise(xs) for n, xs in times.items()}, batch=args.batch, T=T, steps_per_sample=args.step_block)
    print(f'grounding train step, {args.batch} scans, T={T}, bf16: ' + '; '.join(
        f'{n} {summarise(xs)["median_ms"]:.2f} ms [{min(xs):.2f} .. {max(xs):.2f}]' for n, xs in times.items()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--layers', type=int, default=12)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--batch', type=int, default=12)
    ap.add_argument('--step-block', type=int, default=4)
    ap.add_argument('--step-rounds', type=int, default=5)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--step-only', choices=['torch', 'hip'], default=None)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU fallback'
    dev = torch.device('cuda:0')
    out = dict(encoder={}, grounding_step=None, layers=args.layers)
    if not args.step_only:
        encoder_table(dev, args, out)
    if not args.no_step:
        grounding_step(dev, args, out)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
