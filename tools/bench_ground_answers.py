"""Time the answer selection of a grounder and the grounding walk session against what a user had without them.

    python tools/bench_ground_answers.py [--reps 30] [--inner 10] [--frames 50] [--at 0 9 24 49] [--prompts 8] [--precision bf16]
                                         [--parts select walk] [--out profiles/ground_answers.txt]

select   es_ground_answers -- ONE launch for all P prompts and one read of the P counts -- against the parent's composition per prompt:
         es_topk_sorted + es_box3d_iou_filter with zero labels and one class + the read of the kept count.  P = 1, 16, 64 x Q = 256 x
         topk = 1, 5, 10 at select_answers' default thresholds (IoU 0.25, score 0.0) on clustered populations
         (tests/scene_filter_spec.clustered with 32 objects of 8 jittered boxes, a seeded row permutation and score reshuffle per prompt).
         Both forms must choose the same rows, or the tool fails.  A timed window is --inner calls of one form (a single call is a
         fraction of a millisecond), the two forms alternate inside every repetition, every shape is warmed first; reported per CALL:
         median [min, max] in ms of a host clock around work that ends in a host read, and for the one launch its device time (events).
walk     GroundWalk on a synthetic walk of T = 50 frames at 480 x 480 with 10 000 points per frame, the shipped mv-grounding model: at
         every t of --at, on a session that has seen frames 0 .. t: scene() (the cache dropped first) and ground(scene, prompts), against
         encode_scene + ground on views 0 .. t and the cloud prefix -- what answering at frame t costs without the session -- and the
         observe() of frame t itself.  Alternating, warmed, median [min, max] of --reps.
One JSON line per record.  There is no CPU path: without a GPU the tool fails."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

LINES = []
PROMPTS = ['the chair next to the window', 'find the table that is closer to the door', 'the lamp', 'a monitor on the desk',
           'the sofa facing the television', 'the cabinet in the corner', 'the bed under the shelf', 'the bin beside the door']


def emit(d):
    line = json.dumps(d)
    LINES.append(line)
    print(line, flush=True)


def _stats(ts, per=1):
    ts = sorted(t / per for t in ts)
    return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4))


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


# ------------------------------------------------------------------------------------------------------------------ select
def bench_select(reps, inner, dev):
    import scene_filter_spec as S
    from embodiedscan_amd import hip
    P_, st = hip.P, hip.stream
    Q = 256
    for n_p in (1, 16, 64):
        boxes, scores = [], []
        for k in range(n_p):
            pop = S.clustered(7 + k % 3, n_clusters=Q // 8)
            rng = np.random.default_rng(500 + k)
            perm = rng.permutation(Q)
            boxes.append(pop['boxes'][perm])
            scores.append(pop['scores'][rng.permutation(Q)])
        b = torch.from_numpy(np.stack(boxes)).to(dev)
        s = torch.from_numpy(np.stack(scores)).to(dev)
        labels = torch.zeros(Q, dtype=torch.int32, device=dev)
        order = torch.empty(Q, dtype=torch.int32, device=dev)
        keep_idx = torch.empty((n_p, Q), dtype=torch.int32, device=dev)
        keep_cnt = torch.empty(1, dtype=torch.int32, device=dev)
        for topk in (1, 5, 10):
            ans_idx = torch.empty((n_p, topk), dtype=torch.int32, device=dev)
            ans_cnt = torch.empty(n_p, dtype=torch.int32, device=dev)

            def one():
                hip.call('es_ground_answers', P_(b), P_(s), n_p, Q, 0.25, 0.0, topk, P_(ans_idx), P_(ans_cnt), st())
                return ans_cnt.tolist()

            def comp():
                cnt = []
                for p in range(n_p):
                    hip.call('es_topk_sorted', P_(s[p]), 1, Q, 0, Q, P_(order), st())
                    hip.call('es_box3d_iou_filter', P_(b[p]), P_(s[p]), P_(labels), P_(order), Q, 1, 0.25, 0.0, topk, P_(keep_idx[p]), P_(keep_cnt), st())
                    cnt.append(int(keep_cnt.item()))
                return cnt

            def one_device():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hip.call('es_ground_answers', P_(b), P_(s), n_p, Q, 0.25, 0.0, topk, P_(ans_idx), P_(ans_cnt), st())
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)

            for _ in range(3):
                c1, c2 = one(), comp()
            torch.cuda.synchronize()
            got, want = ans_idx.cpu().numpy(), keep_idx.cpu().numpy()
            assert c1 == c2 and all((got[p, :c] == want[p, :c]).all() for p, c in enumerate(c1)), f'P = {n_p}, topk = {topk}: the two forms choose different rows'
            t1, t2 = [], []
            for _ in range(reps):
                t1.append(_timed(lambda: [one() for _ in range(inner)]))
                t2.append(_timed(lambda: [comp() for _ in range(inner)]))
            a, c = _stats(t1, inner), _stats(t2, inner)
            emit(dict(bench='ground_answers', P=n_p, Q=Q, topk=topk, reps=reps, calls_per_window=inner, answers=int(sum(c1)), one_launch=a,
                      one_launch_device=_stats([one_device() for _ in range(reps)]), composition=c, launches=[1, 2 * n_p], host_reads=[1, n_p],
                      composition_over_one_launch=round(c['median_ms'] / a['median_ms'], 2)))


# ------------------------------------------------------------------------------------------------------------------ walk
def bench_walk(T, at, reps, n_prompts, dev):
    from bench_walk import _const_meta, sweep_scan
    from embodiedscan_amd import pipeline
    from embodiedscan_amd.config import build_detector, load_config
    from embodiedscan_amd.structures import Det3DDataSample
    det = build_detector(load_config(os.path.join(ROOT, 'configs', 'mv_grounding.py')), device=dev, seed=0).to(dev)
    det.train(False)
    prompts = [PROMPTS[k % len(PROMPTS)] + (f' number {k}' if k >= len(PROMPTS) else '') for k in range(n_prompts)]
    scan = sweep_scan(T, (480, 480))
    dscan = pipeline.upload_scan(scan, dev)
    cloud = pipeline.depth_to_points(dscan)
    pre = det.data_preprocessor({'inputs': {'points': [cloud], 'img': dscan['img'][None]}, 'data_samples': [Det3DDataSample(scan['meta'])]}, False)
    imgs = pre['inputs']['imgs'].clone()
    meta = pre['data_samples'][0].metainfo
    d2i = meta['depth2img']
    frames = [(t, r, dict(extrinsic=e, intrinsic=i)) for t, r, e, i in pipeline.walk_frames(dscan, cloud.shape[0])]
    walk = det.open_walk(_const_meta(meta), max_frames=T)

    def observe(t):
        _, (r0, r1), m = frames[t]
        return walk.observe(imgs[0, t], cloud[r0:r1], m)

    def rollback(t, n):
        walk.t, walk.cloud.n = t, n
        walk.meta.pop()
        walk._scene = None

    def fresh_scene():
        walk._scene = None
        return walk.scene()

    def baseline_scene(t):
        m = dict(meta, depth2img=dict(d2i, extrinsic=d2i['extrinsic'][:t + 1], intrinsic=d2i['intrinsic'][:t + 1]))
        return det.encode_scene({'points': [cloud[:frames[t][1][1]]], 'imgs': imgs[:, :t + 1]}, [Det3DDataSample(m)])[0]

    for t in range(T):
        if t in at:
            snap = (walk.t, walk.cloud.n)
            for _ in range(3):                                              # every shape warmed on both sides
                observe(t)
                det.ground(fresh_scene(), prompts)
                rollback(*snap)
                det.ground(baseline_scene(t), prompts)
            to, ts, tg, tb, tbg = [], [], [], [], []
            for _ in range(reps):
                to.append(_timed(lambda: observe(t)))
                ts.append(_timed(fresh_scene))
                sc = walk.scene()
                tg.append(_timed(lambda: det.ground(sc, prompts)))
                rollback(*snap)
                box = []
                tb.append(_timed(lambda: box.append(baseline_scene(t))))
                tbg.append(_timed(lambda: det.ground(box[0], prompts)))
            o, s, g, b, bg = (_stats(v) for v in (to, ts, tg, tb, tbg))
            emit(dict(bench='ground_walk_ask', t=t, reps=reps, prompts=n_prompts, cloud_rows=frames[t][1][1], tokens=int(sc.L), observe=o,
                      scene=s, ground=g, baseline_encode_scene=b, baseline_ground=bg,
                      first_ask_speedup=round((b['median_ms'] + bg['median_ms']) / (s['median_ms'] + g['median_ms']), 3),
                      next_ask_speedup=round((b['median_ms'] + bg['median_ms']) / g['median_ms'], 3)))
        observe(t)
    torch.cuda.synchronize()
    emit(dict(bench='ground_walk_state', T=T, state_bytes=walk.state_bytes()))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--frames', type=int, default=50)
    ap.add_argument('--at', type=int, nargs='+', default=[0, 9, 24, 49])
    ap.add_argument('--prompts', type=int, default=8)
    ap.add_argument('--precision', default='bf16', choices=['bf16', 'f32'])
    ap.add_argument('--parts', nargs='+', default=['select', 'walk'], choices=['select', 'walk'])
    ap.add_argument('--out', default=None, help='also write the JSON lines to this file')
    a = ap.parse_args()
    at = sorted(t for t in a.at if t < a.frames)
    assert at and a.frames <= 64 and a.reps >= 1 and a.inner >= 1
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_ground_answers.py needs the GPU: there is no CPU path')
    from embodiedscan_amd import engine as _E
    _E.PRECISION[0] = a.precision
    device = torch.device('cuda:0')
    emit(dict(bench='ground_answers_tool', precision=a.precision, device=torch.cuda.get_device_name(0)))
    if 'select' in a.parts:
        bench_select(a.reps, a.inner, device)
    if 'walk' in a.parts:
        sys.path.insert(0, os.path.join(ROOT, 'tools'))
        bench_walk(a.frames, at, a.reps, a.prompts, device)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')
