"""dev tool: one scene, many prompts.  The full grounding config (256 queries, 6 decoder layers) on ONE synthetic scan at the benchmark's
grounding shape (20 views of 480x640, bf16), for P in {1, 16, 64} prompts:
  encode_scene once; ground() per call and per prompt; predict() on P samples that replicate the scan (the only way without the
  feature; in batches of at most --predict-batch scans, the benchmark's grounding batch);
and at kernel level, for the scene's actual token count Lk, in both precisions:
  es_contrastive_shared_fwd against es_contrastive_fwd on P copies of the rows (the copy itself is not timed);
  es_attn_kv_fwd against es_attn_fwd(B = 1, Lq = P * 256) on the same projections; es_attn_kv_prepare shown separately (once per scene
  and layer: its cost per ground() call is six launches spread over every later call).
One process; every form and shape is warmed up; model-level samples are host wall times between device synchronisations, kernel-level
samples device-event times around --calls back-to-back launches; the forms are sampled in alternation --repeats times; median and
min .. max are printed, the spread of one form between its repeats is the yardstick for a difference between two.  Each step runs
under its own time limit (SIGALRM: the process ends there, nothing further is started).
  python tools/bench_shared_scene.py [--json profiles/shared_scene.json]"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from embodiedscan_amd import engine as E, hip, pipeline  # noqa: E402
from embodiedscan_amd.hip import P, call  # noqa: E402


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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def sample(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def summarise(xs):
    return dict(median_ms=round(statistics.median(xs), 4), min_ms=round(min(xs), 4), max_ms=round(max(xs), 4), samples=len(xs))


def fmt(r):
    return f'{r["median_ms"]:.3f} ms [{r["min_ms"]:.3f} .. {r["max_ms"]:.3f}]'


def alternate(forms, repeats, take):
    times = {n: [] for n in forms}
    for _ in range(repeats):
        for n, fn in forms.items():                     # alternating: a drift of the machine reaches every form alike
            times[n].append(take(fn))
    return {n: summarise(xs) for n, xs in times.items()}


def model_level(dev, args, out):
    from embodiedscan_amd.config import build_detector, load_config
    from embodiedscan_amd.synth import make_grounding_sample, make_scan
    E.PRECISION[0] = 'bf16'
    with limit(600, 'building the grounder and its scan'):
        cfg = load_config(os.path.join(ROOT, 'configs', 'mv_grounding.py'))
        det = build_detector(cfg, device=dev, seed=0).to(dev)
        sc = make_scan(777, n_views=20, augment=True, render_device=str(dev))
        anns = [make_grounding_sample(sc, seed=i) for i in range(max(args.prompts))]
        dscan = pipeline.upload_scan(sc, dev)
        torch.cuda.synchronize()

    def batch_of(n, first=0):
        return det.data_preprocessor(pipeline.make_grounding_batch([dscan] * n, anns[first:first + n]), False)
    one = batch_of(1)
    scenes = []

    def encode():
        scenes[:] = det.encode_scene(one['inputs'], one['data_samples'])
    with limit(600, 'warm-up of encode_scene'):
        for _ in range(3):
            encode()
    with limit(300, 'timing encode_scene'):
        enc = summarise([wall(encode) for _ in range(args.repeats)])
    scene = scenes[0]
    out['scene'] = dict(tokens=scene.L, views=20, precision='bf16', num_queries=det.num_queries, layers=det.decoder.num_layers)
    out['encode_scene'] = enc
    print(f'scene: {scene.L} tokens; encode_scene {fmt(enc)}', flush=True)
    for n_p in args.prompts:
        texts, spans = [a['text'] for a in anns[:n_p]], [a['tokens_positive'] for a in anns[:n_p]]
        chunks = [batch_of(min(args.predict_batch, n_p - c0), c0) for c0 in range(0, n_p, args.predict_batch)]

        def ground():
            return det.ground(scene, texts, tokens_positive=spans)

        def predict():
            for d in chunks:
                det.forward(d['inputs'], d['data_samples'], mode='predict')
        with limit(900, f'warm-up at P = {n_p}'):
            for _ in range(3):
                ground()
            for _ in range(2):
                predict()
        with limit(900, f'timing at P = {n_p}'):
            row = alternate({'ground': ground, 'predict_replicated': predict}, args.repeats, wall)
        row['ground_per_prompt_ms'] = round(row['ground']['median_ms'] / n_p, 4)
        row['predict_per_prompt_ms'] = round(row['predict_replicated']['median_ms'] / n_p, 4)
        row['T'] = int(det.last_text['mask'].shape[1])
        out['model'][f'P={n_p}'] = row
        print(f'P={n_p}: ground {fmt(row["ground"])} = {row["ground_per_prompt_ms"]:.3f} ms / prompt; predict on {n_p} replicated samples '
              f'{fmt(row["predict_replicated"])} = {row["predict_per_prompt_ms"]:.3f} ms / prompt', flush=True)
    E.PRECISION[0] = 'f32'
    feats = scene.feats.clone()
    del det, scenes, scene
    torch.cuda.empty_cache()
    return feats


def kernel_level(dev, args, out, feats):
    Lk, C, H, Q, T = feats.shape[0], feats.shape[1], 8, 256, args.tokens
    g = torch.Generator().manual_seed(3)
    s = hip.stream()
    k, v = (torch.randn(Lk, C, generator=g).to(dev) for _ in range(2))
    bias = torch.tensor([-4.6], device=dev)
    for n_p in args.prompts:
        Lq = n_p * Q
        q = torch.randn(Lq, C, generator=g).to(dev)
        text = torch.randn(n_p * T, C, generator=g).to(dev)
        tlen = torch.randint(4, T + 1, (n_p,), generator=g).to(torch.int32).to(dev)
        vrep = feats.repeat(n_p, 1).contiguous()
        rm_a, rm_b = torch.empty(n_p * Lk, device=dev), torch.empty(n_p * Lk, device=dev)

        def shared():
            call('es_contrastive_shared_fwd', P(feats), Lk, P(text), n_p, T, C, P(tlen), P(bias), 0, T, P(rm_a), s)

        def replicated():
            call('es_contrastive_fwd', P(vrep), n_p, Lk, P(text), T, C, P(tlen), 0, P(bias), 0, T, P(rm_b), s)
        with limit(300, f'contrastive kernels at P = {n_p}'):
            for fn in (shared, replicated):
                sample(fn, 3)
            assert torch.equal(rm_a, rm_b), 'es_contrastive_shared_fwd differs from es_contrastive_fwd on the replicated rows'
            row = alternate({'es_contrastive_shared_fwd': shared, 'es_contrastive_fwd_replicated': replicated}, args.repeats,
                            lambda fn: sample(fn, args.calls))
        out['kernels'][f'contrastive P={n_p}'] = dict(row, L=Lk, T=T)
        print(f'contrastive Lk={Lk} P={n_p} T={T}: ' + '; '.join(f'{n} {fmt(r)}' for n, r in row.items()), flush=True)
        del vrep
        for bf in (1, 0):
            kv = torch.empty(int(hip.raw('es_attn_kv_bytes')(H, Lk, bf)), dtype=torch.uint8, device=dev)
            o_a, o_b = torch.empty(Lq, C, device=dev), torch.empty(Lq, C, device=dev)
            lse_a, lse_b = torch.empty(H * Lq, device=dev), torch.empty(H * Lq, device=dev)

            def prepare():
                call('es_attn_kv_prepare', P(k), C, P(v), C, H, Lk, bf, P(kv), s)

            def kv_fwd():
                call('es_attn_kv_fwd', P(q), C, P(kv), H, Lq, Lk, P(o_a), C, P(lse_a), bf, s)

            def plain():
                call('es_attn_fwd', P(q), C, P(k), C, P(v), C, 1, H, Lq, Lk, 0, P(o_b), C, P(lse_b), bf, s)
            with limit(300, f'attention kernels at P = {n_p}, bf16 = {bf}'):
                for fn in (prepare, kv_fwd, plain):
                    sample(fn, 3)
                diff = float((o_a - o_b).abs().max())
                row = alternate({'es_attn_kv_fwd': kv_fwd, 'es_attn_fwd_B1': plain, 'es_attn_kv_prepare': prepare}, args.repeats,
                                lambda fn: sample(fn, args.calls))
            a, b = row['es_attn_kv_fwd'], row['es_attn_fwd_B1']
            spread = max(a['max_ms'] - a['min_ms'], b['max_ms'] - b['min_ms'])
            row.update(Lq=Lq, Lk=Lk, max_abs_diff=diff, gain_ms=round(b['median_ms'] - a['median_ms'], 4), spread_ms=round(spread, 4),
                       faster_beyond_spread=bool(b['median_ms'] - a['median_ms'] > spread))
            out['kernels'][f'attention P={n_p} {"bf16" if bf else "f32"}'] = row
            print(f'attention Lq={Lq} Lk={Lk} {"bf16" if bf else "f32"}: ' + '; '.join(f'{n} {fmt(row[n])}' for n in ('es_attn_kv_fwd', 'es_attn_fwd_B1', 'es_attn_kv_prepare'))
                  + f'; gain {row["gain_ms"]:.3f} ms, spread {row["spread_ms"]:.3f} ms, max |difference| {diff:.2e}', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--prompts', type=int, nargs='+', default=[1, 16, 64])
    ap.add_argument('--predict-batch', type=int, default=12)
    ap.add_argument('--tokens', type=int, default=24, help='padded token count of the kernel-level text blocks')
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--kernels-only', type=int, default=0, metavar='LK', help='skip the model level; kernel level at LK random tokens')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU; there is no CPU fallback'
    dev = torch.device('cuda:0')
    out = dict(scene=None, encode_scene=None, model={}, kernels={})
    if args.kernels_only:
        feats = torch.randn(args.kernels_only, 256, generator=torch.Generator().manual_seed(1)).to(dev)
    else:
        feats = model_level(dev, args, out)
    kernel_level(dev, args, out, feats)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
