"""Time per frame of the overlays of embodiedscan_amd.render against the numpy specification on the host.

    python tools/bench_render.py [--reps 20] [--frames 20] [--boxes 10 100 1000] [--host-frames 2] [--out profiles/render_overlay.txt]

boxes      V = 20 frames of 480 x 640 (V, 3, H, W) u8, n boxes spread through a 10 m room seen by a ring of cameras: es_render_project +
           es_render_boxes together, and each alone
occupancy  the same frames over a 40 x 40 x 16 volume, about a third of it occupied: es_render_occupancy
Every launch is warmed three times; the clock is device events around a window of back-to-back repetitions -- at least `reps`, and as many
as fill 100 ms -- median of 5 windows with [min, max]; ms per frame = window / repetitions / V.  bytes per frame = the least the overlay must move,
2 H W 3 (read the frame, write the frame), the GB/s that is at the measured time, and for the boxes what the kernel moves by its own
shape (moved_bytes: the frame, the cull's read of every record by every tile, the records a tile keeps).  `host` = tests/render_spec.py (numpy, f64 / int64,
the only alternative a user has without the kernels) on --host-frames of the same frames, wall clock, and the first host frame is compared
byte for byte with the device's.  One JSON line per record.
There is no CPU path: without a GPU the tool fails."""
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


def emit(d):
    line = json.dumps(d)
    LINES.append(line)
    print(line, flush=True)


def windows(fn, reps, n_windows=5, least_ms=100.0):
    """-> [ms per call] of n_windows windows of back-to-back calls, by device events: `reps` calls, or as many as fill least_ms"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    reps = max(reps, min(5000, int(np.ceil(least_ms * reps / max((time.perf_counter() - t0) * 1e3, 1e-3)))))
    out = []
    for _ in range(n_windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def stats(ms, V):
    per = sorted(m / V for m in ms)
    return dict(ms_per_frame=round(per[len(per) // 2], 5), min=round(per[0], 5), max=round(per[-1], 5))


def moved_bytes(rec, H, W, radius_q=4):
    """bytes per frame the box kernel moves, from the shapes and the records: the frame in and out, the 5 ints wave 0 of every 64 x 4 tile reads
    of every record to cull it, and the 17 ints + 3 colour bytes of every record a tile keeps"""
    V, n = rec.shape[:2]
    tx = np.arange(0, W, 64)
    ty = np.arange(0, H, 4)
    x0, x1 = 4 * tx + 2, 4 * np.minimum(tx + 63, W - 1) + 2
    y0, y1 = 4 * ty + 2, 4 * np.minimum(ty + 3, H - 1) + 2
    live = ((rec[:, :, 16] & 256) == 0) & ((rec[:, :, 16] & 255) != 0)
    kx = ((rec[:, :, 17, None] - radius_q <= x1) & (rec[:, :, 19, None] + radius_q >= x0)).sum(-1)      # tile columns a record reaches
    ky = ((rec[:, :, 18, None] - radius_q <= y1) & (rec[:, :, 20, None] + radius_q >= y0)).sum(-1)
    kept = int((kx * ky * live).sum())
    return 2 * H * W * 3 + len(tx) * len(ty) * n * 20 + kept * 71 // V, kept / (V * len(tx) * len(ty))


def ring(V, H, W):
    import render_spec as S
    cams = [S.camera((5 + 4.5 * np.cos(a), 5 + 4.5 * np.sin(a), 1.5), a + np.pi, -0.1, 0.8 * W, H, W) for a in np.linspace(0, 2 * np.pi, V, endpoint=False)]
    return np.stack([c[0] for c in cams]), np.stack([c[1] for c in cams])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--boxes', type=int, nargs='+', default=[10, 100, 1000])
    ap.add_argument('--host-frames', type=int, default=2)
    ap.add_argument('--size', type=int, nargs=2, default=[480, 640])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_render.py measures the MI355X: no GPU, no number'
    import render_spec as S
    from embodiedscan_amd import hip, render as RD
    dev = torch.device('cuda:0')
    V, (H, W) = a.frames, a.size
    P, st = hip.P, hip.stream()
    rng = np.random.default_rng(0)
    src = S.frames(V, H, W, 1, 1)
    frames = torch.from_numpy(src).to(dev)
    out = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
    E, K = ring(V, H, W)
    least = 2 * H * W * 3
    hv = min(a.host_frames, V)
    emit(dict(record='setup', device=torch.cuda.get_device_name(0), frames=V, height=H, width=W, reps=a.reps, least_bytes_per_frame=least))
    for n in a.boxes:
        boxes = np.zeros((n, 9), np.float32)
        boxes[:, :3] = rng.uniform((0.5, 0.5, 0.0), (9.5, 9.5, 2.5), (n, 3))
        boxes[:, 3:6] = rng.uniform(0.2, 1.5, (n, 3))
        boxes[:, 6:] = rng.uniform(-np.pi, np.pi, (n, 3)) * (1.0, 0.2, 0.2)
        col = RD.class_palette(n + 1)[1:] if n < 256 else S.colours(n, 2)
        b, c = torch.from_numpy(boxes).to(dev), torch.from_numpy(np.ascontiguousarray(col)).to(dev)
        Ed, Kd = torch.from_numpy(E).to(dev), torch.from_numpy(K).to(dev)
        rec = torch.empty((V, n, hip.CONSTS['ES_RENDER_REC']), dtype=torch.int32, device=dev)

        def project():
            hip.call('es_render_project', P(b), n, P(Ed), P(Kd), V, H, W, P(rec), st)

        def draw():
            hip.call('es_render_boxes', P(frames), 1, V, H, W, P(rec), P(c), n, 4, 192, P(out), st)

        def both():
            project()
            draw()
        r_both, r_proj, r_draw = stats(windows(both, a.reps), V), stats(windows(project, a.reps), V), stats(windows(draw, a.reps), V)
        both()
        torch.cuda.synchronize()
        got = out[:hv].cpu().numpy()
        rec_h = rec.cpu().numpy()
        m = rec_h[:, :, 16]
        moved, kept_per_tile = moved_bytes(rec_h.astype(np.int64), H, W)
        usable = np.array([[bin(int(x) & 255).count('1') for x in row] for row in m])
        t0 = time.perf_counter()
        want = S.render_boxes(src[:hv], 1, boxes, E[:hv], K[:hv], col, 4, 192, check=False)
        host_ms = (time.perf_counter() - t0) * 1e3 / hv
        emit(dict(record='boxes', n=n, **r_both, project_ms_per_frame=r_proj['ms_per_frame'], draw_ms_per_frame=r_draw['ms_per_frame'],
                  gb_per_s_at_least_bytes=round(least / (r_both['ms_per_frame'] * 1e-3) / 1e9, 1), bytes_moved_per_frame=int(moved),
                  moved_over_least=round(moved / least, 2), records_kept_per_tile=round(kept_per_tile, 1), host_spec_ms_per_frame=round(host_ms, 1),
                  host_over_device=round(host_ms / r_both['ms_per_frame'], 1), equals_host_spec=bool(np.array_equal(got, want)),
                  boxes_partly_usable=int(((usable > 0) & (usable < 8)).sum()), boxes_skipped=int((m & 256).astype(bool).sum()),
                  box_views=int(m.size), pixels_touched_share=round(float((got != S.to_hwc(src[:hv], 1)).any(-1).mean()), 3)))
    shape, pr = (40, 40, 16), (0.0, 0.0, 0.0, 10.0, 10.0, 3.2)
    occ = rng.integers(1, 12, shape).astype(np.uint8) * (rng.random(shape) < 0.33)
    pal = RD.class_palette(12)
    occ_d = torch.from_numpy(occ).to(dev)

    def occupancy():
        RD.render_occupancy(frames, E, K, occ_d, pr, pal, alpha=0.5, out=out)
    rays = torch.from_numpy(RD.camera_rays(E, K)).to(dev)
    pal_d = torch.from_numpy(pal).to(dev)
    import ctypes
    size = (np.array(pr[3:]) - np.array(pr[:3])) / np.array(shape)
    grid = (ctypes.c_double * 6)(*pr[:3], *size.tolist())

    def occupancy_launch():
        hip.call('es_render_occupancy', P(frames), 1, V, H, W, P(rays), P(occ_d), *shape, ctypes.cast(grid, ctypes.c_void_p), P(pal_d), 12, 128, P(out), st)
    r_launch, r_api = stats(windows(occupancy_launch, a.reps), V), stats(windows(occupancy, a.reps), V)
    occupancy_launch()
    torch.cuda.synchronize()
    got = out[:hv].cpu().numpy()
    t0 = time.perf_counter()
    want = S.draw_occupancy(src[:hv], 1, S.rays_of(E[:hv], K[:hv]), occ, np.array(pr[:3]), size, pal, 128)
    host_ms = (time.perf_counter() - t0) * 1e3 / hv
    emit(dict(record='occupancy', volume=list(shape), **r_launch, through_render_occupancy_ms_per_frame=r_api['ms_per_frame'],
              gb_per_s_at_least_bytes=round(least / (r_launch['ms_per_frame'] * 1e-3) / 1e9, 1), host_spec_ms_per_frame=round(host_ms, 1),
              host_over_device=round(host_ms / r_launch['ms_per_frame'], 1), equals_host_spec=bool(np.array_equal(got, want)),
              pixels_touched_share=round(float((got != S.to_hwc(src[:hv], 1)).any(-1).mean()), 3)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
