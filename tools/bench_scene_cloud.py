"""Time of the 3-D scene export of embodiedscan_amd.scene_cloud at the product's shape, against the map's splat and against what a user had
without these kernels.

    python tools/bench_scene_cloud.py [--reps 5] [--frames 50] [--size 480 640] [--host-frames 2] [--out profiles/scene_cloud.json]

The recording is embodiedscan_amd.synth.write_demo_scene at --frames frames of --size pixels, read back through inference.scene_info (depth
PNG in millimetres, JPEG frames, the folder's own poses); cell 0.02 m, capacity 2^22, max_depth 8 m.

splat      es_cloud_splat, one launch over all frames.  cold: behind a clear(), one launch at a time, median of 5 with [min, max]; filled:
           on a table that already holds the scene (what a walk meets after its first frames), windows of back-to-back launches.
map_splat  es_map_splat of the same frames into a 2 cm map that covers the cloud, cold and filled the same way: the same reads with one atomic
           per pixel and no probing.  The yardstick; the ratio is reported, not gated.
points     SceneCloud.points(): mask, compaction, sort, rows (synchronises twice: wall clock).
label      es_cloud_label of the cloud's rows against m = 10, 100, 1000 boxes spread over the room.
faces      occupancy_mesh of a 40 x 40 x 16 volume with a third of its voxels labelled (synchronises once: wall clock).
torch      the composition a user could write: unprojection in torch (f64), torch.unique on the packed keys, scatter_reduce_ amax / sum;
           it must give the kernel's rows (keys, values and hits) bit for bit.  ACCEPTANCE: the splat (cold, which does the same work) is faster.
host       tests/scene_cloud_spec.py (numpy f64) on --host-frames frames, wall clock, compared with the device's table on those frames.
walk       what one frame of a walk adds with cloud=: one frame joins the cloud, points(), the labels of 10 boxes (wall clock, files not written).
Clock and windows as tools/bench_scene_map.py (device events round windows of back-to-back repetitions that fill 100 ms, median of 5 with
[min, max]).  One JSON line per record.  There is no CPU path: without a GPU the tool fails."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from bench_render import LINES, emit  # noqa: E402
from bench_scene_map import stats, windows  # noqa: E402


def load_recording(frames, H, W, seed=3):
    """-> (depth (V, H, W) f32 metres, frames (V, 3, H, W) u8, extrinsic (V, 4, 4) f64, intrinsic (V, 4, 4) f64) of a demo folder"""
    from PIL import Image
    from embodiedscan_amd.inference import scene_info
    from embodiedscan_amd.synth import write_demo_scene
    with tempfile.TemporaryDirectory() as root:
        write_demo_scene(root, 'room', n_frames=frames, height=H, width=W, seed=seed)
        info = scene_info(os.path.join(root, 'room'))
        depth = np.stack([np.asarray(Image.open(p)).astype(np.float32) / np.float32(info['depth_shift']) for p in info['depth_img_path']])
        img = np.stack([np.asarray(Image.open(p).convert('RGB')) for p in info['img_path']])
    E = np.stack([np.asarray(e, np.float64) for e in info['depth2img']['extrinsic']])
    K = np.repeat(np.asarray(info['depth2img']['intrinsic'], np.float64)[None], len(E), 0)
    return depth, np.ascontiguousarray(img.transpose(0, 3, 1, 2)), E, K


def cold(clear, run, per=1):
    """one launch at a time behind clear() -> sorted ms / per of 5"""
    out = []
    for _ in range(5):
        clear()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / per)
    return sorted(out)


def wall(fn, n=5):
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)


def table_rows(cl):
    """the occupied slots of a SceneCloud's table -> (keys ascending, vals, hits) on the device"""
    full = cl.tkeys != -1
    k, order = torch.sort(cl.tkeys[full])
    return k, cl.tvals[full][order], cl.thits[full][order].long() & 0xffffffff


def torch_cloud(depth, frames_hwc, rays, cell, z_min, z_max, max_d):
    """the composition a user could write -> (keys ascending, vals, hits)"""
    V, H, W = depth.shape
    dev = depth.device
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing='ij')
    d = depth.double()
    M = rays[:, :9].reshape(V, 3, 3)
    p = [rays[:, 9 + k, None, None] + d * ((M[:, k, 0, None, None] * x + M[:, k, 1, None, None] * y) + M[:, k, 2, None, None]) for k in range(3)]
    ok = (d > 0) & (d <= max_d) & (p[2] >= z_min) & (p[2] < z_max)
    i = [torch.floor(a / cell) for a in p]
    for a in i:
        ok &= (a >= -131072.0) & (a < 131072.0)
    i = [a[ok].long() + 131072 for a in i]
    key = (i[0] << 36) | (i[1] << 18) | i[2]
    col = frames_hwc[ok].long()
    val = ((2097152 - torch.floor(d[ok] * 256.0).long()) << 24) | (col[:, 0] << 16) | (col[:, 1] << 8) | col[:, 2]
    keys, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    top = torch.zeros(len(keys), dtype=torch.int64, device=dev)
    top.scatter_reduce_(0, inv, val, 'amax', include_self=True)
    return keys, top, cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--frames', type=int, default=50)
    ap.add_argument('--size', type=int, nargs=2, default=[480, 640])
    ap.add_argument('--cell', type=float, default=0.02)
    ap.add_argument('--capacity', type=int, default=1 << 22)
    ap.add_argument('--host-frames', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_scene_cloud.py measures the MI355X: no GPU, no number'
    import render_spec as RS
    import scene_cloud_spec as S
    from embodiedscan_amd import hip, scene_cloud as SC, scene_map as SM
    dev = torch.device('cuda:0')
    V, (H, W) = a.frames, a.size
    depth_h, frames_h, E, K = load_recording(V, H, W)
    rays_h = RS.rays_of(E, K)
    depth, frames, rays = torch.from_numpy(depth_h).to(dev), torch.from_numpy(frames_h).to(dev), torch.from_numpy(rays_h).to(dev)
    cl = SC.SceneCloud(dev, cell=a.cell, capacity=a.capacity, max_depth=8.0)
    P, st = hip.P, hip.stream()
    gp = SC._dptr(cl._g)
    emit(dict(record='setup', device=torch.cuda.get_device_name(0), frames=V, height=H, width=W, pixels=V * H * W, cell_m=a.cell, capacity=a.capacity,
              state_bytes=cl.state_bytes(), reps=a.reps))

    def splat():
        hip.call('es_cloud_splat', P(depth), V, H, W, P(frames), 1, H, W, P(rays), gp, P(cl.tkeys), P(cl.tvals), P(cl.thits), cl.capacity,
                 P(cl.counters), st)
    splat()
    torch.cuda.synchronize()
    first = cold(cl.clear, splat, V)
    accepted, dropped = cl.pixel_counts()
    r = stats(windows(splat, a.reps), V)
    cl.clear()
    splat()
    rows = table_rows(cl)
    accepted, dropped = cl.pixel_counts()
    emit(dict(record='splat', cold_ms_per_frame=round(first[2], 5), cold_min=round(first[0], 5), cold_max=round(first[-1], 5), filled_ms_per_frame=r['ms'],
              filled_min=r['min'], filled_max=r['max'], window_ms=r['window_ms'], launches_per_window=r['calls_per_window'],
              accepted_pixels=accepted, dropped_pixels=dropped, voxels=int(rows[0].numel()), load=round(rows[0].numel() / cl.capacity, 4)))
    # the map's splat on the same frames
    xyz, rgb, hits = cl.points()
    lo, hi = xyz.min(0).values.cpu().numpy().astype(np.float64), xyz.max(0).values.cpu().numpy().astype(np.float64)
    grid = SM.MapGrid.covering(lo[:2], hi[:2], a.cell, z_min=-100.0, z_max=100.0)
    m = SM.SceneMap(grid, dev, max_depth=8.0)

    def map_splat():
        hip.call('es_map_splat', P(depth), V, H, W, P(frames), 1, H, W, P(rays), m._gp(), grid.width, grid.height, P(m.keys), st)
    map_splat()
    mfirst = cold(m.clear, map_splat, V)
    mr = stats(windows(map_splat, a.reps), V)
    emit(dict(record='map_splat', map=[grid.height, grid.width], cold_ms_per_frame=round(mfirst[2], 5), cold_min=round(mfirst[0], 5),
              cold_max=round(mfirst[-1], 5), filled_ms_per_frame=mr['ms'], filled_min=mr['min'], filled_max=mr['max'],
              cloud_over_map_cold=round(first[2] / mfirst[2], 2), cloud_over_map_filled=round(r['ms'] / mr['ms'], 2)))
    # rows, labels, faces
    pts = wall(lambda: cl.points())
    emit(dict(record='points', rows=int(xyz.shape[0]), ms=round(pts[2], 3), min=round(pts[0], 3), max=round(pts[-1], 3)))
    rng = np.random.default_rng(3)
    for mb in (10, 100, 1000):
        b = np.zeros((mb, 9), np.float32)
        b[:, :3] = rng.uniform(lo, hi, (mb, 3))
        b[:, 3:6] = rng.uniform(0.3, 1.5, (mb, 3))
        b[:, 6] = rng.uniform(-np.pi, np.pi, mb)
        bt = torch.from_numpy(b).to(dev)
        lab, sup = SC.label(xyz, bt)
        rl = stats(windows(lambda: SC.label(xyz, bt), a.reps))
        emit(dict(record='label', boxes=mb, points=int(xyz.shape[0]), ms=rl['ms'], min=rl['min'], max=rl['max'], window_ms=rl['window_ms'],
                  labelled_share=round(float((lab >= 0).float().mean()), 3)))
    occ = torch.from_numpy((rng.random((40, 40, 16)) < 1 / 3).astype(np.uint8) * rng.integers(1, 5, (40, 40, 16), dtype=np.uint8)).to(dev)
    pal = torch.from_numpy(RS.colours(5, 1)).to(dev)
    fc = wall(lambda: SC.occupancy_mesh(occ, (-3.2, -3.2, -0.78, 3.2, 3.2, 1.78), pal))
    emit(dict(record='faces', volume=[40, 40, 16], faces=int(SC.occupancy_mesh(occ, (-3.2, -3.2, -0.78, 3.2, 3.2, 1.78), pal)[1].shape[0]), ms=round(fc[2], 3),
              min=round(fc[0], 3), max=round(fc[-1], 3)))
    # the alternatives a user had
    hwc = frames.permute(0, 2, 3, 1).contiguous()
    tk = torch_cloud(depth, hwc, rays, a.cell, cl.z_min, cl.z_max, cl.max_depth)
    same = all(torch.equal(x, y) for x, y in zip(tk, rows))
    rt = stats(windows(lambda: torch_cloud(depth, hwc, rays, a.cell, cl.z_min, cl.z_max, cl.max_depth), 1, least_ms=1.0), V)
    emit(dict(record='torch', ms_per_frame=rt['ms'], min=rt['min'], max=rt['max'], window_ms=rt['window_ms'], equals_device=bool(same),
              torch_over_splat_cold=round(rt['ms'] / first[2], 1), splat_is_faster=bool(first[-1] < rt['min'])))
    hv = min(a.host_frames, V)
    t0 = time.perf_counter()
    want = S.splat(depth_h[:hv], frames_h[:hv], 1, rays_h[:hv], S.Grid(a.cell, max_depth=8.0), exact=True)
    host_ms = (time.perf_counter() - t0) * 1e3 / hv
    cl.clear()
    hip.call('es_cloud_splat', P(depth), hv, H, W, P(frames), 1, H, W, P(rays), gp, P(cl.tkeys), P(cl.tvals), P(cl.thits), cl.capacity, P(cl.counters), st)
    got = [t.cpu().numpy() for t in table_rows(cl)]
    emit(dict(record='host', frames=hv, spec_ms_per_frame=round(host_ms, 1), host_over_splat_cold=round(host_ms / first[2], 1),
              equals_device=bool(all(np.array_equal(g, w) for g, w in zip(got, want)))))
    # one frame of a walk with cloud=
    cl.clear()
    splat()
    boxes10 = torch.from_numpy(b[:10].copy()).to(dev)

    def walk_frame():
        cl.add(depth[V - 1:V], frames[V - 1:V], E[V - 1:V], K[V - 1:V], layout='chw')
        SC.label(cl.points()[0], boxes10)
    wf = wall(walk_frame)
    emit(dict(record='walk_frame', t=V - 1, boxes=10, ms=round(wf[2], 3), min=round(wf[0], 3), max=round(wf[-1], 3)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(LINES) + '\n')


if __name__ == '__main__':
    main()
