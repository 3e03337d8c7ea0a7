"""Predictions drawn onto the recording's frames on the device: what the reference's visualization/img_drawer.py and
continuous_drawer.py do through cv2 / open3d on the host, as three launches of csrc/predict.hip.

    render_boxes      9-DoF boxes -> translucent faces and solid edges   (es_render_project + es_render_boxes)
    render_occupancy  an (X, Y, Z) label volume -> the first occupied voxel along every pixel's ray   (es_render_occupancy)
    class_palette     one colour per class, an integer formula of this project
    save_frames       (V, H, W, 3) u8 -> PNG files through PIL: the only host synchronisation of this module

Frames are u8, (V, 3, H, W) -- what upload_scan leaves in dscan['img'] -- or (V, H, W, 3); the result is always (V, H, W, 3).  extrinsic /
intrinsic are the 4 x 4 matrices of the fusion (depth2img: aligned frame -> camera, camera -> pixels) AT THE RESOLUTION OF THE FRAMES: a
caller that resized the frames scales the intrinsic's first two rows (inference.frame_matrices does).  Text labels, the 3-D viewer and
occlusion against the depth maps are out of scope."""
import ctypes
import os

import numpy as np
import torch

from . import hip

MAX_SIDE = 4096


def class_palette(n):
    """(n, 3) u8, deterministic, rows pairwise distinct for n <= 256.  Integer HSV: the hue advances by the golden ratio of the 1530-step
    colour circle (row i: i * 0x9E3779B1 mod 2^32, scaled), saturation and value cycle through small tables with periods 3 and 4; row 0
    (the detection background / the `empty` voxel class) is mid grey."""
    n = int(n)
    if n < 0:
        raise ValueError(f'class_palette: n = {n}')
    sat, val = (255, 176, 216), (255, 208, 160, 232)
    out = np.zeros((n, 3), np.uint8)
    for i in range(n):
        if i == 0:
            out[i] = (128, 128, 128)
            continue
        h = (((i * 0x9E3779B1) & 0xFFFFFFFF) * 1530) >> 32
        s, v = sat[i % 3], val[(i // 3) % 4]
        sec, f = divmod(h, 255)
        p = v * (255 - s) // 255
        q = v * (255 * 255 - s * f) // (255 * 255)
        t = v * (255 * 255 - s * (255 - f)) // (255 * 255)
        out[i] = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))[sec]
    return out


def _frames(fn, frames, layout, out):
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4:
        raise ValueError(f'{fn}: frames are a 4-d uint8 tensor, got {getattr(frames, "dtype", type(frames))} {tuple(getattr(frames, "shape", ()))}')
    first, last = frames.shape[1] == 3, frames.shape[3] == 3
    if layout is None:
        if first == last:
            raise ValueError(f'{fn}: frames of shape {tuple(frames.shape)} are neither clearly (V, 3, H, W) nor (V, H, W, 3): pass layout=')
        layout = 'chw' if first else 'hwc'
    if layout not in ('chw', 'hwc') or not (first if layout == 'chw' else last):
        raise ValueError(f'{fn}: layout {layout!r} does not fit frames of shape {tuple(frames.shape)}')
    chw = layout == 'chw'
    V = int(frames.shape[0])
    H, W = (int(frames.shape[2]), int(frames.shape[3])) if chw else (int(frames.shape[1]), int(frames.shape[2]))
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f'{fn}: frames of {H} x {W} pixels, the kernels take 1 .. {MAX_SIDE} per side')
    if not frames.is_contiguous():
        raise ValueError(f'{fn}: frames must be contiguous')
    if out is None:
        out = torch.empty((V, H, W, 3), dtype=torch.uint8, device=frames.device)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (V, H, W, 3) or not out.is_contiguous()
          or out.device != frames.device):
        raise ValueError(f'{fn}: out is a contiguous uint8 ({V}, {H}, {W}, 3) tensor on {frames.device}')
    elif chw and out.data_ptr() == frames.data_ptr():
        raise ValueError(f'{fn}: in place only for (V, H, W, 3) frames')
    return chw, V, H, W, out


def _matrices(fn, m, V, name):
    """-> (V, 4, 4) f64 numpy on the host (a device tensor is read back: pass host matrices, as the meta dicts carry them)"""
    if isinstance(m, torch.Tensor):
        m = m.detach().cpu().numpy()
    m = np.asarray(m, np.float64)
    if m.shape != (V, 4, 4):
        raise ValueError(f'{fn}: {name} of shape {m.shape}, expected ({V}, 4, 4)')
    return m


def _alpha(fn, alpha):
    a = int(round(float(alpha) * 256))
    if not 0 <= a <= 256:
        raise ValueError(f'{fn}: alpha = {alpha}, the image weight lies in 0 .. 1')
    return a


def _u8_rows(fn, t, dev, name, rows=None):
    t = torch.as_tensor(t)
    if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != 3 or (rows is not None and t.shape[0] != rows):
        raise ValueError(f'{fn}: {name} is uint8 ({"n" if rows is None else rows}, 3), got {t.dtype} {tuple(t.shape)}')
    if isinstance(dev, torch.device) and t.device.type != 'cpu' and t.device != dev:
        raise ValueError(f'{fn}: {name} on {t.device}, frames on {dev}')
    return t.to(dev).contiguous()


def render_boxes(frames, extrinsic, intrinsic, boxes, colors, thickness=2, alpha=0.75, out=None, layout=None):
    """frames u8 (V, 3, H, W) or (V, H, W, 3); extrinsic / intrinsic (V, 4, 4) (host arrays or tensors); boxes (n, 9) f32 tensor or
    EulerDepthInstance3DBoxes on the frames' device; colors (n, 3) u8 -> (V, H, W, 3) u8 on the device.  thickness in pixels (the line is
    thickness / 2 to either side; 0.5 .. 32), alpha = the image's weight under a face.  The defaults are the reference drawer's.
    ValueError before any launch: frames not u8 / 4-d / contiguous, boxes on another device or not (n, 9), a wrong count of colours or
    matrices, thickness or alpha out of range, `out` of the wrong shape."""
    fn = 'render_boxes'
    chw, V, H, W, out = _frames(fn, frames, layout, out)
    dev = frames.device
    boxes = getattr(boxes, 'tensor', boxes)
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or boxes.shape[1] != 9:
        raise ValueError(f'{fn}: boxes (n, 9), got {tuple(getattr(boxes, "shape", ()))}')
    if boxes.device != dev:
        raise ValueError(f'{fn}: boxes on {boxes.device}, frames on {dev}')
    n = int(boxes.shape[0])
    colors = _u8_rows(fn, colors, dev, 'colors', n)
    radius_q = int(round(float(thickness) * 2))
    if not 1 <= radius_q <= 64:
        raise ValueError(f'{fn}: thickness = {thickness} pixels, the kernel takes 0.5 .. 32')
    a = _alpha(fn, alpha)
    E = torch.from_numpy(_matrices(fn, extrinsic, V, 'extrinsic').astype(np.float32)).to(dev)
    K = torch.from_numpy(_matrices(fn, intrinsic, V, 'intrinsic').astype(np.float32)).to(dev)
    b = boxes.float().contiguous()
    rec = torch.empty((V, max(n, 1), hip.CONSTS['ES_RENDER_REC']), dtype=torch.int32, device=dev)
    P, st = hip.P, hip.stream()
    hip.call('es_render_project', P(b), n, P(E), P(K), V, H, W, P(rec), st)
    hip.call('es_render_boxes', P(frames), int(chw), V, H, W, P(rec), P(colors), n, radius_q, a, P(out), st)
    return out


def camera_rays(extrinsic, intrinsic):
    """(V, 4, 4) host matrices -> (V, 12) f64: the 3 x 3 R^T K^-1 (row-major) and the camera centre -R^T t, in numpy f64"""
    E, K = np.asarray(extrinsic, np.float64), np.asarray(intrinsic, np.float64)
    out = np.zeros((len(E), 12), np.float64)
    for v in range(len(E)):
        Rt = E[v, :3, :3].T
        out[v, :9] = (Rt @ np.linalg.inv(K[v, :3, :3])).reshape(-1)
        out[v, 9:] = -(Rt @ E[v, :3, 3])
    return out


def render_occupancy(frames, extrinsic, intrinsic, occ, point_cloud_range, palette, alpha=0.5, out=None, layout=None):
    """occ: (X, Y, Z) integer labels on the frames' device (pred_occupancy); point_cloud_range (x0, y0, z0, x1, y1, z1) of the volume;
    palette (C, 3) u8, C <= 256 -> (V, H, W, 3) u8: every pixel whose ray meets a voxel with 1 <= label < C is blended with that class's
    colour, shaded by the face the ray entered through.  Label 0, labels >= C and labels outside 0 .. 255 are transparent.
    ValueError before any launch: as render_boxes; occ not a 3-d integer tensor on the frames' device, a palette of more than 256 rows
    (labels that do not fit u8), an empty range."""
    fn = 'render_occupancy'
    chw, V, H, W, out = _frames(fn, frames, layout, out)
    dev = frames.device
    if not isinstance(occ, torch.Tensor) or occ.dim() != 3 or occ.dtype.is_floating_point or occ.dtype == torch.bool or min(occ.shape) < 1:
        raise ValueError(f'{fn}: occ is a non-empty 3-d integer tensor, got {getattr(occ, "dtype", type(occ))} {tuple(getattr(occ, "shape", ()))}')
    if occ.device != dev:
        raise ValueError(f'{fn}: occ on {occ.device}, frames on {dev}')
    palette = _u8_rows(fn, palette, dev, 'palette')
    C = int(palette.shape[0])
    if not 1 <= C <= 256:
        raise ValueError(f'{fn}: a palette of {C} rows: labels are stored as u8, 1 .. 256 classes')
    pr = np.asarray(point_cloud_range, np.float64).reshape(-1)
    if pr.shape != (6,) or not np.all(pr[3:] > pr[:3]):
        raise ValueError(f'{fn}: point_cloud_range = {point_cloud_range}')
    a = _alpha(fn, alpha)
    E, K = _matrices(fn, extrinsic, V, 'extrinsic'), _matrices(fn, intrinsic, V, 'intrinsic')
    X, Y, Z = (int(s) for s in occ.shape)
    if occ.dtype != torch.uint8:
        occ = torch.where((occ < 0) | (occ > 255), torch.zeros((), dtype=occ.dtype, device=dev), occ).to(torch.uint8)
    occ = occ.contiguous()
    size = (pr[3:] - pr[:3]) / np.array([X, Y, Z], np.float64)
    grid = (ctypes.c_double * 6)(*pr[:3].tolist(), *size.tolist())
    rays = torch.from_numpy(camera_rays(E, K)).to(dev)
    P = hip.P
    hip.call('es_render_occupancy', P(frames), int(chw), V, H, W, P(rays), P(occ), X, Y, Z, ctypes.cast(grid, ctypes.c_void_p), P(palette), C, a,
             P(out), hip.stream())
    return out


def save_frames(dir, frames_hwc, stem='frame', start=0):
    """(V, H, W, 3) u8 (tensor on any device, or numpy) -> dir/<stem>_0000.png ... (numbered from `start`) through PIL; returns the paths"""
    from PIL import Image
    a = frames_hwc.detach().cpu().numpy() if isinstance(frames_hwc, torch.Tensor) else np.asarray(frames_hwc)
    if a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] != 3:
        raise ValueError(f'save_frames: (V, H, W, 3) uint8, got {a.dtype} {a.shape}')
    os.makedirs(dir, exist_ok=True)
    paths = []
    for i in range(a.shape[0]):
        paths.append(os.path.join(dir, f'{stem}_{start + i:04d}.png'))
        Image.fromarray(np.ascontiguousarray(a[i]), 'RGB').save(paths[-1])
    return paths
