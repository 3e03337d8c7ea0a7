"""Time of the bird's-eye map of embodiedscan_amd.scene_map against the least bytes of each launch and against what a user had without it.

    python tools/bench_scene_map.py [--reps 20] [--frames 20] [--walk-t 49] [--host-frames 2] [--out profiles/scene_map.txt]

splat      V = 20 depth maps of 480 x 640 with frames of the same size, a ring of cameras in a 10 m room, into a 1024 x 1024 map (cells of
           1 cm round the room): ms per frame, and the GB/s that is at the least bytes of the launch, 7 B per depth pixel (4 depth + 3 colour).
           (profiles/scene_map.txt also holds the comparison with the same kernel WITHOUT the load in front of the atomic, made with a
           build that exported both and alternated them window by window in this tool; that variant lost and is deleted.)
resolve    8 B in and 3 B out per cell.
walk map   one whole map of a walk at t = --walk-t as inference.walk_scene(map=) makes it: splat of ONE frame, resolve, footprints of 10
           boxes, the trail of t + 1 centres (host-side argument checks and uploads included).
host       tests/scene_map_spec.py (numpy f64) on --host-frames of the same frames, wall clock; torch: the same keys computed with torch
           tensor operations on the device and scatter_reduce_('amax') on int64.  Both are compared with the kernel's keys bit for bit.
Every launch is warmed three times; the clock is device events around a window of back-to-back repetitions -- at least `reps`, and as many
as fill 100 ms (`window_ms` of every record says what the windows came to) -- median of 5 windows with [min, max].  Nothing clears the keys
inside or between the windows: every timed splat meets a map that already holds the scene, which is what a walk meets after its first
frames; the splat onto an EMPTY map is timed separately, one launch at a time behind a clear, as `first_ms_per_frame`.  `enqueue_ms` is the
host's time to issue one launch (wall clock around the window's loop, before the device is waited for): where it is not well below the
device's ms per launch the figure is bounded by the launch rate, not by the kernel.
One JSON line per record.  There is no CPU path: without a GPU the tool fails."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_render import LINES, emit, ring  # noqa: E402


def windows(fn, reps, n_windows=5, least_ms=100.0):
    """-> ([ms per call] of n_windows windows of back-to-back calls by device events, calls per window, host ms to enqueue one call): `reps`
    calls, or as many as fill least_ms of device time, found by trial windows (no upper bound: a 4 us launch takes 25 000 of them)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    while True:                                                  # grow the window until the device itself spends least_ms in it
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        trial = e0.elapsed_time(e1)
        if trial >= least_ms:
            break
        reps = int(np.ceil(reps * 1.3 * least_ms / max(trial, 1e-3)))
    out, enq = [], []
    for _ in range(n_windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        enq.append((time.perf_counter() - t0) * 1e3 / reps)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out, reps, sorted(enq)[len(enq) // 2]


def stats(w, per=1):
    ms, reps, enq = w
    v = sorted(m / per for m in ms)
    return dict(ms=round(v[len(v) // 2], 5), min=round(v[0], 5), max=round(v[-1], 5), window_ms=round(sorted(ms)[len(ms) // 2] * reps, 1),
                calls_per_window=reps, enqueue_ms=round(enq, 5))


def room_depth(E, K, H, W, seed=0):
    """depth maps of the 10 x 10 x 3 m room the ring stands in: every ray meets a wall, the floor or the ceiling (f64, then f32), with 2 % of
    the pixels invalid (0)"""
    import render_spec as RS
    rays = RS.rays_of(E, K)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    out = np.zeros((len(rays), H, W), np.float32)
    rng = np.random.default_rng(seed)
    lo, hi = np.array([0.0, 0.0, 0.0]), np.array([10.0, 10.0, 3.0])
    for v in range(len(rays)):
        M, c = rays[v, :9].reshape(3, 3), rays[v, 9:]
        t = np.full((H, W), np.inf)
        for k in range(3):
            r = (M[k, 0] * x + M[k, 1] * y) + M[k, 2]
            with np.errstate(divide='ignore', invalid='ignore'):
                tk = np.where(r > 0, (hi[k] - c[k]) / r, np.where(r < 0, (lo[k] - c[k]) / r, np.inf))
            t = np.minimum(t, tk)
        t = t * rng.uniform(0.6, 1.0, (H, W))                    # furniture: something nearer than the wall
        t[rng.random((H, W)) < 0.02] = 0.0
        out[v] = t
    return out, rays


def torch_keys(depth, frames_hwc, rays, g, Wm, Hm):
    """the composition a user could write: the splat in torch tensor operations (f64) and scatter_reduce_('amax') on int64 keys"""
    V, H, W = depth.shape
    dev = depth.device
    x0, y0, cell, z_min, z_max, max_d = g
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing='ij')
    d = depth.double()
    M = rays[:, :9].reshape(V, 3, 3)
    p = [rays[:, 9 + k, None, None] + d * ((M[:, k, 0, None, None] * x + M[:, k, 1, None, None] * y) + M[:, k, 2, None, None]) for k in range(3)]
    ok = (d > 0) & (d <= max_d) & (p[2] >= z_min) & (p[2] < z_max)
    zq = torch.floor((p[2] - z_min) * 1024.0)
    ix, iy = torch.floor((p[0] - x0) / cell), torch.floor((p[1] - y0) / cell)
    ok &= (ix >= 0) & (ix < Wm) & (iy >= 0) & (iy < Hm)
    col = frames_hwc.long()
    key = ((torch.where(ok, zq, torch.zeros_like(zq)).long() + 1) << 24) | (col[..., 0] << 16) | (col[..., 1] << 8) | col[..., 2]
    idx = torch.where(ok, (Hm - 1 - iy) * Wm + ix, torch.zeros_like(ix)).long()
    keys = torch.zeros(Hm * Wm, dtype=torch.int64, device=dev)
    keys.scatter_reduce_(0, idx[ok], key[ok], 'amax', include_self=True)
    return keys.reshape(Hm, Wm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--walk-t', type=int, default=49)
    ap.add_argument('--host-frames', type=int, default=2)
    ap.add_argument('--size', type=int, nargs=2, default=[480, 640])
    ap.add_argument('--map', type=int, nargs=2, default=[1024, 1024])
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_scene_map.py measures the MI355X: no GPU, no number'
    import render_spec as RS
    import scene_map_spec as S
    from embodiedscan_amd import hip, scene_map as SM
    dev = torch.device('cuda:0')
    V, (H, W), (Hm, Wm) = a.frames, a.size, a.map
    P, st = hip.P, hip.stream()
    E, K = ring(V, H, W)
    depth_h, rays_h = room_depth(E, K, H, W)
    frames_h = RS.frames(V, H, W, 1, 1)
    cell = 10.24 / Wm
    grid = SM.MapGrid(-0.12, -0.12, cell, Wm, Hm, z_min=-0.5, z_max=2.5)
    G = S.Grid(grid.x0, grid.y0, grid.cell, Wm, Hm, grid.z_min, grid.z_max, 8.0)
    m = SM.SceneMap(grid, dev, max_depth=8.0)
    depth, frames, rays = torch.from_numpy(depth_h).to(dev), torch.from_numpy(frames_h).to(dev), torch.from_numpy(rays_h).to(dev)
    gp = m._gp()
    least_splat, least_resolve = 7 * H * W, 11 * Hm * Wm
    emit(dict(record='setup', device=torch.cuda.get_device_name(0), frames=V, height=H, width=W, map=[Hm, Wm], cell_m=cell, reps=a.reps,
              least_bytes_per_frame_splat=least_splat, least_bytes_resolve=least_resolve))

    keys_a = m.keys

    def check_run():
        hip.call('es_map_splat', P(depth), V, H, W, P(frames), 1, H, W, P(rays), gp, Wm, Hm, P(keys_a), st)
    check_run()                                                 # the cold splat: an empty map, one launch over all V frames, 5 times
    torch.cuda.synchronize()
    cold = []
    for _ in range(5):
        keys_a.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check_run()
        e1.record()
        e1.synchronize()
        cold.append(e0.elapsed_time(e1) / V)
    cold = sorted(cold)
    r = stats(windows(check_run, a.reps), V)
    torch.cuda.synchronize()
    got = keys_a.cpu().numpy()
    cen = S.census(depth_h[:a.host_frames], frames_h[:a.host_frames], 1, rays_h[:a.host_frames], G, exact=True)
    ms_check = r['ms']
    emit(dict(record='splat', ms_per_frame=r['ms'], min=r['min'], max=r['max'], window_ms=r['window_ms'], launches_per_window=r['calls_per_window'],
              enqueue_ms_per_launch=r['enqueue_ms'], ms_per_launch=round(r['ms'] * V, 5), first_ms_per_frame=round(cold[2], 5),
              first_min=round(cold[0], 5), first_max=round(cold[-1], 5), gb_per_s_at_least_bytes=round(least_splat / (r['ms'] * 1e-3) / 1e9, 1),
              first_gb_per_s_at_least_bytes=round(least_splat / (cold[2] * 1e-3) / 1e9, 1),
              cells_filled_share=round(float((got != 0).mean()), 3), accepted_share_first_frames=round(cen['accepted'], 3)))
    # the alternatives a user had
    hv = min(a.host_frames, V)
    t0 = time.perf_counter()
    want = S.splat(depth_h[:hv], frames_h[:hv], 1, rays_h[:hv], G, exact=True)
    host_ms = (time.perf_counter() - t0) * 1e3 / hv
    m.clear()
    hip.call('es_map_splat', P(depth), hv, H, W, P(frames), 1, H, W, P(rays), gp, Wm, Hm, P(m.keys), st)
    torch.cuda.synchronize()
    dev_first = m.keys.cpu().numpy()
    hwc = frames.permute(0, 2, 3, 1).contiguous()
    g6 = (grid.x0, grid.y0, grid.cell, grid.z_min, grid.z_max, 8.0)
    tk = torch_keys(depth, hwc, rays, g6, Wm, Hm)
    r_torch = stats(windows(lambda: torch_keys(depth, hwc, rays, g6, Wm, Hm), 3), V)
    emit(dict(record='alternatives', host_spec_ms_per_frame=round(host_ms, 1), host_over_device=round(host_ms / ms_check, 1),
              host_equals_device=bool(np.array_equal(want, dev_first)), torch_scatter_ms_per_frame=r_torch['ms'], torch_min=r_torch['min'],
              torch_max=r_torch['max'], torch_window_ms=r_torch['window_ms'], torch_over_device=round(r_torch['ms'] / ms_check, 1), torch_equals_device=bool(np.array_equal(tk.cpu().numpy(), got))))
    # resolve, on the whole map again
    m.clear()
    check_run()
    img = torch.empty((Hm, Wm, 3), dtype=torch.uint8, device=dev)
    hz = torch.empty((Hm, Wm), dtype=torch.float32, device=dev)
    r_img = stats(windows(lambda: hip.call('es_map_resolve', P(keys_a), Wm, Hm, gp, 0, 1, P(img), 0, st), a.reps))
    r_hz = stats(windows(lambda: hip.call('es_map_resolve', P(keys_a), Wm, Hm, gp, 0, 1, P(img), P(hz), st), a.reps))
    emit(dict(record='resolve', ms=r_img['ms'], min=r_img['min'], max=r_img['max'], window_ms=r_img['window_ms'], launches_per_window=r_img['calls_per_window'],
              enqueue_ms_per_launch=r_img['enqueue_ms'], gb_per_s_at_least_bytes=round(least_resolve / (r_img['ms'] * 1e-3) / 1e9, 1),
              with_height_ms=r_hz['ms'], with_height_min=r_hz['min'], with_height_max=r_hz['max'], equals_host_spec=bool(np.array_equal(img.cpu().numpy(), S.resolve(got, G, (0, 0, 0), 1)[0]))))
    # one whole map of a walk at t
    t = a.walk_t
    rng = np.random.default_rng(3)
    boxes = np.zeros((10, 9), np.float32)
    boxes[:, :3] = rng.uniform((0.5, 0.5, 0.0), (9.5, 9.5, 1.5), (10, 3))
    boxes[:, 3:6] = rng.uniform(0.3, 1.5, (10, 3))
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, 10)
    b, col = torch.from_numpy(boxes).to(dev), torch.from_numpy(RS.colours(10, 1)).to(dev)
    ang = np.linspace(0, 2 * np.pi, t + 1, endpoint=False)
    trail = np.stack([5 + 4.5 * np.cos(ang), 5 + 4.5 * np.sin(ang), np.full(t + 1, 1.5)], 1)
    E64, K64 = E.astype(np.float64), K.astype(np.float64)
    v = t % V

    def walk_map():
        m.add(depth[v:v + 1], frames[v:v + 1], E64[v:v + 1], K64[v:v + 1], layout='chw')
        m.image(out=img)
        m.draw_boxes(img, b, col)
        m.draw_trail(img, trail)
    r_walk = stats(windows(walk_map, a.reps))
    emit(dict(record='walk_map', t=t, boxes=10, trail=t + 1, ms=r_walk['ms'], min=r_walk['min'], max=r_walk['max'], window_ms=r_walk['window_ms'], state_bytes=m.state_bytes()))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
