"""The scene seen from above, on the device: a bird's-eye map of the aligned frame that shows the recording's own depth
pixels, coloured by its frames and z-buffered from above under a ceiling cut, with box footprints, the camera trail and the top
surface of an occupancy volume drawn over it.  Four launches of csrc/predict.hip plus the existing es_render_boxes:

    MapGrid     the rectangle, the cell size and the z cut; .around(camera centres) picks one for a recording
    SceneMap    add(depth, frames, extrinsic, intrinsic) any number of views at any time (es_map_splat: an integer max per cell, so the
                map does not depend on the order or grouping of the views), image() / height() (es_map_resolve), draw_boxes / draw_trail
                (es_map_project + es_render_boxes), draw_occupancy (es_map_occupancy)

extrinsic / intrinsic are the (V, 4, 4) matrices of the fusion AT THE RESOLUTION OF THE DEPTH MAPS (inference.depth_matrices); the frames
may have any other size (the nearest frame pixel colours a depth pixel).  Images are (Hm, Wm, 3) u8 on the device, +y up; nothing here
synchronises with the host: render.save_frames writes the files."""
import ctypes
import math

import numpy as np
import torch

from . import hip
from . import render as RD

Z_STEPS = 1024                     # height quantisation of the z-buffer: steps per metre
MAX_Z_RANGE = 4096.0
TRAIL_COLOR = (255, 255, 255)


class MapGrid:
    """width x height cells of `cell` metres, lower-left corner (x0, y0) of the aligned frame; points with z_min <= z < z_max are shown.
    Cell (ix, iy) is image row height - 1 - iy, column ix."""

    def __init__(self, x0, y0, cell, width, height, z_min=-1.0, z_max=2.0):
        self.x0, self.y0, self.cell, self.z_min, self.z_max = float(x0), float(y0), float(cell), float(z_min), float(z_max)
        self.width, self.height = int(width), int(height)
        if not (1 <= self.width <= RD.MAX_SIDE and 1 <= self.height <= RD.MAX_SIDE):
            raise ValueError(f'MapGrid: {self.width} x {self.height} cells, the kernels take 1 .. {RD.MAX_SIDE} per side')
        if not self.cell > 0 or not math.isfinite(self.cell) or not (math.isfinite(self.x0) and math.isfinite(self.y0)):
            raise ValueError(f'MapGrid: cell = {cell} at ({x0}, {y0})')
        if not self.z_max > self.z_min or not self.z_max - self.z_min <= MAX_Z_RANGE:
            raise ValueError(f'MapGrid: z cut [{z_min}, {z_max}): a non-empty range of at most {MAX_Z_RANGE:.0f} m')

    @classmethod
    def covering(cls, lo_xy, hi_xy, cell=0.02, z_min=-1.0, z_max=2.0):
        """the rectangle [lo, hi] snapped outward to whole cells (of the lattice through the origin)"""
        cell = float(cell)
        if not cell > 0 or not math.isfinite(cell):
            raise ValueError(f'MapGrid: cell = {cell}')
        lo, hi = np.asarray(lo_xy, np.float64).reshape(2), np.asarray(hi_xy, np.float64).reshape(2)
        if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(hi >= lo)):
            raise ValueError(f'MapGrid: the rectangle {lo.tolist()} .. {hi.tolist()}')
        i0, i1 = np.floor(lo / cell), np.ceil(hi / cell)
        n = np.maximum(i1 - i0, 1.0)
        if n.max() > RD.MAX_SIDE:
            fit = float((hi - lo).max()) / (RD.MAX_SIDE - 2)
            raise ValueError(f'MapGrid: {int(n[0])} x {int(n[1])} cells of {cell} m, the kernels take {RD.MAX_SIDE} per side: '
                             f'a cell of {fit:.4g} m or more fits')
        return cls(i0[0] * cell, i0[1] * cell, cell, int(n[0]), int(n[1]), z_min, z_max)

    @classmethod
    def around(cls, centres_xy, reach=8.0, cell=0.02, z_min=-1.0, z_max=2.0):
        """the rectangle of the camera centres (n, 2+) grown by `reach` metres -- what a depth camera of that range can have seen --
        snapped outward to whole cells.  ValueError when a side would pass 4096 cells; the message names the cell size that fits."""
        c = np.asarray(centres_xy, np.float64)
        if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 2 or not float(reach) >= 0:
            raise ValueError(f'MapGrid.around: centres (n >= 1, 2) and reach >= 0, got {c.shape}, {reach}')
        return cls.covering(c[:, :2].min(0) - float(reach), c[:, :2].max(0) + float(reach), cell, z_min, z_max)

    def to_json(self):
        return dict(x0=self.x0, y0=self.y0, cell=self.cell, width=self.width, height=self.height, z_min=self.z_min, z_max=self.z_max)

    @classmethod
    def from_json(cls, d):
        return cls(d['x0'], d['y0'], d['cell'], d['width'], d['height'], d['z_min'], d['z_max'])

    def to_pixels(self, xy):
        """(..., 2) metres of the aligned frame -> (..., 2) continuous image coordinates (column, row): pixel (c, r) covers [c, c+1) x [r, r+1)"""
        xy = np.asarray(xy, np.float64)
        return np.stack([(xy[..., 0] - self.x0) / self.cell, self.height - (xy[..., 1] - self.y0) / self.cell], -1)

    def to_metres(self, px):
        """the inverse of to_pixels; the centre of pixel (c, r) is to_metres((c + 0.5, r + 0.5))"""
        px = np.asarray(px, np.float64)
        return np.stack([self.x0 + px[..., 0] * self.cell, self.y0 + (self.height - px[..., 1]) * self.cell], -1)

    def host(self, max_depth):
        """the six f64 the launches read on the host: x0, y0, cell, z_min, z_max, max_depth"""
        return (ctypes.c_double * 6)(self.x0, self.y0, self.cell, self.z_min, self.z_max, float(max_depth))


def _image(fn, grid, image, dev):
    if (not isinstance(image, torch.Tensor) or image.dtype != torch.uint8 or tuple(image.shape) != (grid.height, grid.width, 3)
            or not image.is_contiguous() or image.device != dev):
        raise ValueError(f'{fn}: the map image is a contiguous uint8 ({grid.height}, {grid.width}, 3) tensor on {dev}, got '
                         f'{getattr(image, "dtype", type(image))} {tuple(getattr(image, "shape", ()))} on {getattr(image, "device", None)}')
    return image


def check_views(fn, device, depth, frames, extrinsic, intrinsic, layout=None, what='map'):
    """the argument checks of SceneMap.add (scene_cloud.SceneCloud.add takes the same views) -> (V, H, W, chw, h, w, E, K)"""
    if not isinstance(depth, torch.Tensor) or depth.dtype != torch.float32 or depth.dim() != 3 or not depth.is_contiguous():
        raise ValueError(f'{fn}: depth is a contiguous float32 (V, H, W) tensor, got {getattr(depth, "dtype", type(depth))} '
                         f'{tuple(getattr(depth, "shape", ()))}')
    if depth.device != device:
        raise ValueError(f'{fn}: depth on {depth.device}, the {what} on {device}')
    V, H, W = (int(s) for s in depth.shape)
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or not frames.is_contiguous():
        raise ValueError(f'{fn}: frames are a contiguous 4-d uint8 tensor, got {getattr(frames, "dtype", type(frames))} '
                         f'{tuple(getattr(frames, "shape", ()))}')
    if frames.device != device:
        raise ValueError(f'{fn}: frames on {frames.device}, the {what} on {device}')
    first, last = frames.shape[1] == 3, frames.shape[3] == 3
    if layout is None:
        if first == last:
            raise ValueError(f'{fn}: frames of shape {tuple(frames.shape)} are neither clearly (V, 3, h, w) nor (V, h, w, 3): pass layout=')
        layout = 'chw' if first else 'hwc'
    if layout not in ('chw', 'hwc') or not (first if layout == 'chw' else last):
        raise ValueError(f'{fn}: layout {layout!r} does not fit frames of shape {tuple(frames.shape)}')
    chw = layout == 'chw'
    h, w = (int(frames.shape[2]), int(frames.shape[3])) if chw else (int(frames.shape[1]), int(frames.shape[2]))
    if int(frames.shape[0]) != V:
        raise ValueError(f'{fn}: {int(frames.shape[0])} frames for {V} depth maps')
    if V > 65535:
        raise ValueError(f'{fn}: {V} views, one launch takes 65535')
    for name, a, b in (('depth maps', H, W), ('frames', h, w)):
        if not (1 <= a <= RD.MAX_SIDE and 1 <= b <= RD.MAX_SIDE):
            raise ValueError(f'{fn}: {name} of {a} x {b} pixels, the kernel takes 1 .. {RD.MAX_SIDE} per side')
    E, K = RD._matrices(fn, extrinsic, V, 'extrinsic'), RD._matrices(fn, intrinsic, V, 'intrinsic')
    return V, H, W, chw, h, w, E, K


class SceneMap:
    """the z-buffer of one map: (height, width) int64 keys on `device`, 0 = empty.  Depth pixels beyond max_depth metres are ignored."""

    def __init__(self, grid, device, max_depth=8.0):
        if not isinstance(grid, MapGrid):
            raise ValueError(f'SceneMap: grid is a MapGrid, got {type(grid).__name__}')
        if not float(max_depth) > 0:
            raise ValueError(f'SceneMap: max_depth = {max_depth}')
        self.grid, self.device, self.max_depth = grid, torch.device(device), float(max_depth)
        self._g = grid.host(max_depth)
        self.keys = torch.zeros((grid.height, grid.width), dtype=torch.int64, device=self.device)

    def _gp(self):
        return ctypes.cast(self._g, ctypes.c_void_p)

    def state_bytes(self):
        return self.keys.numel() * self.keys.element_size()

    def clear(self):
        self.keys.zero_()

    def to_pixels(self, xy):
        return self.grid.to_pixels(xy)

    def to_metres(self, px):
        return self.grid.to_metres(px)

    def add(self, depth, frames, extrinsic, intrinsic, layout=None):
        """depth (V, H, W) f32 metres, frames u8 (V, 3, h, w) or (V, h, w, 3) of any size, both on the map's device; extrinsic / intrinsic
        (V, 4, 4) at the DEPTH maps' resolution.  Any number of views, any number of times, in any order: the map is the same.
        ValueError before any launch: a wrong dtype, shape, device or count, a side outside 1 .. 4096, more than 65535 views."""
        V, H, W, chw, h, w, E, K = check_views('SceneMap.add', self.device, depth, frames, extrinsic, intrinsic, layout)
        if V == 0:
            return self
        rays = torch.from_numpy(RD.camera_rays(E, K)).to(self.device)
        P = hip.P
        hip.call('es_map_splat', P(depth), V, H, W, P(frames), int(chw), h, w, P(rays), self._gp(), self.grid.width, self.grid.height,
                 P(self.keys), hip.stream())
        return self

    def image(self, background=(0, 0, 0), shade=True, out=None):
        """-> (height, width, 3) u8: every seen cell in the colour of its highest point (shade: brighter with height), the others `background`"""
        bg = [int(c) for c in background]
        if len(bg) != 3 or not all(0 <= c <= 255 for c in bg):
            raise ValueError(f'SceneMap.image: background = {background}, three bytes')
        g = self.grid
        if out is None:
            out = torch.empty((g.height, g.width, 3), dtype=torch.uint8, device=self.device)
        _image('SceneMap.image', g, out, self.device)
        P = hip.P
        hip.call('es_map_resolve', P(self.keys), g.width, g.height, self._gp(), (bg[0] << 16) | (bg[1] << 8) | bg[2], int(bool(shade)), P(out),
                 0, hip.stream())
        return out

    def height(self):
        """-> (height, width) f32: the height in metres of every cell's highest point (the middle of its 1/1024 m step), NaN where empty"""
        g = self.grid
        hz = torch.empty((g.height, g.width), dtype=torch.float32, device=self.device)
        hip.call('es_map_resolve', hip.P(self.keys), g.width, g.height, self._gp(), 0, 0, 0, hip.P(hz), hip.stream())
        return hz

    def draw_boxes(self, image, boxes, colors, thickness=2, alpha=0.75):
        """the footprints of 9-DoF boxes (n, 9) in colors (n, 3) u8 over `image`, in place: the twelve edges solid, the faces translucent
        (alpha = the image's weight), drawn by the rasteriser of render.render_boxes.  A zero-size box is a disc of diameter `thickness`."""
        fn = 'SceneMap.draw_boxes'
        g = self.grid
        _image(fn, g, image, self.device)
        boxes = getattr(boxes, 'tensor', boxes)
        if not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or boxes.shape[1] != 9:
            raise ValueError(f'{fn}: boxes (n, 9), got {tuple(getattr(boxes, "shape", ()))}')
        if boxes.device != self.device:
            raise ValueError(f'{fn}: boxes on {boxes.device}, the map on {self.device}')
        n = int(boxes.shape[0])
        colors = RD._u8_rows(fn, colors, self.device, 'colors', n)
        radius_q = int(round(float(thickness) * 2))
        if not 1 <= radius_q <= 64:
            raise ValueError(f'{fn}: thickness = {thickness} pixels, the kernel takes 0.5 .. 32')
        a = RD._alpha(fn, alpha)
        b = boxes.float().contiguous()
        rec = torch.empty((max(n, 1), hip.CONSTS['ES_RENDER_REC']), dtype=torch.int32, device=self.device)
        P, st = hip.P, hip.stream()
        hip.call('es_map_project', P(b), n, self._gp(), g.width, g.height, P(rec), st)
        hip.call('es_render_boxes', P(image), 0, 1, g.height, g.width, P(rec), P(colors), n, radius_q, a, P(image), st)
        return image

    def draw_trail(self, image, centres_xyz, color=TRAIL_COLOR, thickness=3):
        """one disc per camera centre (n, 2 or 3; host array or tensor), in place"""
        c = centres_xyz.detach().cpu().numpy() if isinstance(centres_xyz, torch.Tensor) else np.asarray(centres_xyz)
        c = np.asarray(c, np.float32)
        if c.ndim != 2 or c.shape[1] not in (2, 3):
            raise ValueError(f'SceneMap.draw_trail: centres (n, 2) or (n, 3), got {c.shape}')
        boxes = np.zeros((len(c), 9), np.float32)
        boxes[:, :c.shape[1]] = c
        col = np.asarray(color, np.uint8).reshape(1, 3).repeat(len(c), 0)
        return self.draw_boxes(image, torch.from_numpy(boxes).to(self.device), torch.from_numpy(col), thickness, 1.0)

    def draw_occupancy(self, image, occ, point_cloud_range, palette, alpha=0.5):
        """the top surface of occ (X, Y, Z) integer labels over point_cloud_range, in place: every map pixel whose centre lies over a column
        with a voxel 1 <= label < len(palette) is blended with the colour of the highest such voxel"""
        fn = 'SceneMap.draw_occupancy'
        g = self.grid
        _image(fn, g, image, self.device)
        if not isinstance(occ, torch.Tensor) or occ.dim() != 3 or occ.dtype.is_floating_point or occ.dtype == torch.bool or min(occ.shape) < 1:
            raise ValueError(f'{fn}: occ is a non-empty 3-d integer tensor, got {getattr(occ, "dtype", type(occ))} {tuple(getattr(occ, "shape", ()))}')
        if occ.device != self.device:
            raise ValueError(f'{fn}: occ on {occ.device}, the map on {self.device}')
        palette = RD._u8_rows(fn, palette, self.device, 'palette')
        C = int(palette.shape[0])
        if not 1 <= C <= 256:
            raise ValueError(f'{fn}: a palette of {C} rows: labels are stored as u8, 1 .. 256 classes')
        pr = np.asarray(point_cloud_range, np.float64).reshape(-1)
        if pr.shape != (6,) or not np.all(pr[3:] > pr[:3]):
            raise ValueError(f'{fn}: point_cloud_range = {point_cloud_range}')
        a = RD._alpha(fn, alpha)
        X, Y, Z = (int(s) for s in occ.shape)
        if occ.dtype != torch.uint8:
            occ = torch.where((occ < 0) | (occ > 255), torch.zeros((), dtype=occ.dtype, device=self.device), occ).to(torch.uint8)
        occ = occ.contiguous()
        size = (pr[3:] - pr[:3]) / np.array([X, Y, Z], np.float64)
        vol = (ctypes.c_double * 6)(*pr[:3].tolist(), *size.tolist())
        P = hip.P
        hip.call('es_map_occupancy', P(image), g.width, g.height, self._gp(), P(occ), X, Y, Z, ctypes.cast(vol, ctypes.c_void_p), P(palette), C, a,
                 hip.stream())
        return image
