"""The scene in three dimensions, as files a viewer opens: the recording's depth pixels fused on the device into one
de-duplicated coloured cloud, every point labelled with the detection that contains it, the occupancy prediction as a mesh of exposed voxel
faces, and binary PLY for all of it.  Six launches of csrc/predict.hip plus the existing es_compact_mask / es_sort_u64:

    SceneCloud      add(depth, frames, extrinsic, intrinsic) any number of views at any time (es_cloud_splat: a CAS that only fills an empty
                    slot, an integer max and integer adds, so the cloud does not depend on the order or grouping of the views),
                    points(min_hits) (es_cloud_mask, es_compact_mask, es_sort_u64, es_cloud_points: rows in ascending key order), label
    label           es_cloud_label: the first box that holds each point, and every box's number of points
    occupancy_mesh  es_occ_face_mask, es_compact_mask, es_occ_face_quads
    write_ply / read_ply / box_edges   plain numpy on the host

extrinsic / intrinsic are the (V, 4, 4) matrices of the fusion AT THE RESOLUTION OF THE DEPTH MAPS (inference.depth_matrices), as for
scene_map.SceneMap.  Only SceneCloud.points and occupancy_mesh synchronise with the host: they read a row count."""
import ctypes
import math

import numpy as np
import torch

from . import hip
from . import render as RD
from .scene_map import check_views

MAX_CAPACITY = 1 << 30
MAX_DEPTH = 4096.0
SLOT_BYTES = 20                    # int64 key + u64 value + u32 hits


class CloudFull(RuntimeError):
    """the table dropped pixels: no cloud is returned.  .dropped, .capacity, .fit_capacity, .fit_cell"""

    def __init__(self, dropped, capacity, occupied, cell):
        self.dropped, self.capacity, self.occupied, self.cell = int(dropped), int(capacity), int(occupied), float(cell)
        need = 2 * (self.occupied + self.dropped) + 2            # at most occupied + dropped distinct voxels, in a table at most half full
        self.fit_capacity = 2
        while self.fit_capacity < need and self.fit_capacity < MAX_CAPACITY:
            self.fit_capacity *= 2
        # a surface of area A fills about A / cell^2 voxels: the cell that brings `need` down to this table
        self.fit_cell = float(f'{self.cell * math.sqrt(max(need / self.capacity, 1.0)) * 1.05:.2g}')
        super().__init__(f'SceneCloud: {self.dropped} depth pixels found no slot within {hip.CONSTS["ES_CLOUD_PROBES"]} probes of a table of '
                         f'{self.capacity} slots ({self.occupied} taken): capacity={self.fit_capacity} fits this recording at cell={self.cell:g}, '
                         f'or cell={self.fit_cell:g} at capacity={self.capacity}')


def _dptr(arr):
    return ctypes.cast(arr, ctypes.c_void_p)


def _boxes(fn, boxes, dev):
    boxes = getattr(boxes, 'tensor', boxes)
    if not isinstance(boxes, torch.Tensor) or boxes.dim() != 2 or boxes.shape[1] != 9:
        raise ValueError(f'{fn}: boxes (m, 9), got {tuple(getattr(boxes, "shape", ()))}')
    if boxes.device != dev:
        raise ValueError(f'{fn}: boxes on {boxes.device}, the points on {dev}')
    if boxes.shape[0] > 65535:
        raise ValueError(f'{fn}: {boxes.shape[0]} boxes, one launch takes 65535')
    return boxes.float().contiguous()


def label(xyz, boxes, grow=0.0):
    """xyz (n, 3) f32 and boxes (m, 9) (tensor or EulerDepthInstance3DBoxes) on one device -> (label (n,) int32: the smallest row of `boxes`
    whose box, grown by `grow` metres on every side, holds the point -- lists are in score order, so the best-scoring one -- or -1;
    support (m,) int32: the number of points labelled with each box).  Stream-ordered."""
    fn = 'scene_cloud.label'
    if not isinstance(xyz, torch.Tensor) or xyz.dtype != torch.float32 or xyz.dim() != 2 or xyz.shape[1] != 3 or not xyz.is_contiguous():
        raise ValueError(f'{fn}: xyz is a contiguous float32 (n, 3) tensor, got {getattr(xyz, "dtype", type(xyz))} {tuple(getattr(xyz, "shape", ()))}')
    b = _boxes(fn, boxes, xyz.device)
    grow = float(grow)
    if not (grow >= 0.0 and math.isfinite(grow)):
        raise ValueError(f'{fn}: grow = {grow} metres: finite and not negative')
    n, m = int(xyz.shape[0]), int(b.shape[0])
    lab = torch.empty(n, dtype=torch.int32, device=xyz.device)
    support = torch.empty(m, dtype=torch.int32, device=xyz.device)
    P = hip.P
    hip.call('es_cloud_label', P(xyz), n, P(b), m, grow, P(lab), P(support), hip.stream())
    return lab, support


class SceneCloud:
    """one voxel per `cell` metres of the aligned frame, in a table of `capacity` slots (a power of two) on `device`: the nearest depth
    measurement of a voxel gives its colour, hits counts its pixels.  Points with z[0] <= z < z[1] and a depth of at most max_depth metres."""

    def __init__(self, device, cell=0.02, capacity=1 << 22, z=(-math.inf, math.inf), max_depth=8.0):
        self.device, self.cell, self.capacity, self.max_depth = torch.device(device), float(cell), int(capacity), float(max_depth)
        self.z_min, self.z_max = (float(v) for v in z)
        if not (2 <= self.capacity <= MAX_CAPACITY) or self.capacity & (self.capacity - 1):
            raise ValueError(f'SceneCloud: capacity = {capacity}: a power of two in 2 .. 2^30')
        if not self.cell > 0 or not math.isfinite(self.cell):
            raise ValueError(f'SceneCloud: cell = {cell}')
        if not 0 < self.max_depth <= MAX_DEPTH:
            raise ValueError(f'SceneCloud: max_depth = {max_depth}: in (0, {MAX_DEPTH:.0f}] metres')
        if not self.z_max > self.z_min:
            raise ValueError(f'SceneCloud: z cut [{self.z_min}, {self.z_max}) is empty')
        self._g = (ctypes.c_double * 4)(self.cell, self.z_min, self.z_max, self.max_depth)
        self.tkeys = torch.full((self.capacity,), -1, dtype=torch.int64, device=self.device)
        self.tvals = torch.zeros(self.capacity, dtype=torch.int64, device=self.device)          # (u64 bits)
        self.thits = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)          # (u32 bits)
        self.counters = torch.zeros(2, dtype=torch.int32, device=self.device)                   # (u32 bits: accepted, dropped)
        self.keys = None                                                                        # the sorted keys of the last points()

    def state_bytes(self):
        return self.capacity * SLOT_BYTES + 8

    def clear(self):
        self.tkeys.fill_(-1)
        self.tvals.zero_()
        self.thits.zero_()
        self.counters.zero_()
        self.keys = None

    def add(self, depth, frames, extrinsic, intrinsic, layout=None):
        """the arguments (and the ValueErrors, before any launch) of SceneMap.add.  Any number of views, any number of times, in any order:
        the cloud is the same."""
        V, H, W, chw, h, w, E, K = check_views('SceneCloud.add', self.device, depth, frames, extrinsic, intrinsic, layout, what='cloud')
        if V == 0:
            return self
        rays = torch.from_numpy(RD.camera_rays(E, K)).to(self.device)
        P = hip.P
        hip.call('es_cloud_splat', P(depth), V, H, W, P(frames), int(chw), h, w, P(rays), _dptr(self._g), P(self.tkeys), P(self.tvals),
                 P(self.thits), self.capacity, P(self.counters), hip.stream())
        return self

    def pixel_counts(self):
        """-> (accepted, dropped) depth pixels so far; synchronises"""
        a, d = (int(v) & 0xffffffff for v in self.counters.tolist())
        return a, d

    def points(self, min_hits=1):
        """-> (xyz (n, 3) f32 voxel centres, rgb (n, 3) u8, hits (n,) int32) on the device, the voxels that at least min_hits pixels fell
        into, in ascending key order (x-major, then y, then z): the order depends neither on the table nor on the order of the views.
        Synchronises (the row count).  CloudFull, and no partial cloud, when a pixel was dropped."""
        min_hits = int(min_hits)
        if not 0 <= min_hits < 2 ** 31:
            raise ValueError(f'SceneCloud.points: min_hits = {min_hits}')
        accepted, dropped = self.pixel_counts()
        if dropped:
            raise CloudFull(dropped, self.capacity, int((self.tkeys != -1).sum()), self.cell)
        dev, cap = self.device, self.capacity
        i32, i64 = torch.int32, torch.int64
        room = max(min(cap, accepted), 1)
        mask = torch.empty(cap, dtype=i32, device=dev)
        scratch = torch.empty(cap + cap // 2048 + 8, dtype=i32, device=dev)
        sel, src = torch.empty(room, dtype=i64, device=dev), torch.empty(room, dtype=i32, device=dev)
        cnt = ctypes.c_int(0)
        P, st = hip.P, hip.stream()
        hip.call('es_cloud_mask', P(self.tkeys), P(self.thits), cap, min_hits, P(mask), st)
        hip.call('es_compact_mask', P(self.tkeys), cap, P(mask), P(scratch), P(sel), P(src), ctypes.addressof(cnt), st)
        n = int(cnt.value)
        keys, rows = torch.empty(n, dtype=i64, device=dev), torch.empty(n, dtype=i32, device=dev)
        xyz = torch.empty((n, 3), dtype=torch.float32, device=dev)
        rgb = torch.empty((n, 3), dtype=torch.uint8, device=dev)
        hits = torch.empty(n, dtype=i32, device=dev)
        if n:
            nb = int(hip.raw('es_sort_scratch_bytes')(n))
            sc = torch.empty(nb, dtype=torch.uint8, device=dev)
            hip.call('es_sort_u64', P(sel), P(src), n, P(sc), nb, P(keys), P(rows), st)
            hip.call('es_cloud_points', P(keys), P(rows), n, P(self.tvals), P(self.thits), self.cell, P(xyz), P(rgb), P(hits), st)
        self.keys = keys
        return xyz, rgb, hits

    def label(self, xyz, boxes, grow=0.0):
        return label(xyz, boxes, grow)


def occupancy_mesh(occ, point_cloud_range, palette):
    """occ (X, Y, Z) integer labels on a device (pred_occupancy), point_cloud_range (x0, y0, z0, x1, y1, z1) of the volume, palette (C, 3) u8
    -> (verts (4F, 3) f32, quads (F, 4) int32, face_label (F,) u8, colors (4F, 3) u8) on that device: one quad, counter-clockwise seen from
    outside, per face of a voxel with 1 <= label < C whose neighbour is outside the volume or holds no such label; faces in ascending
    (voxel, face) order, faces -x, +x, -y, +y, -z, +z.  Synchronises (the face count)."""
    fn = 'scene_cloud.occupancy_mesh'
    if not isinstance(occ, torch.Tensor) or occ.dim() != 3 or occ.dtype.is_floating_point or occ.dtype == torch.bool or min(occ.shape) < 1:
        raise ValueError(f'{fn}: occ is a non-empty 3-d integer tensor, got {getattr(occ, "dtype", type(occ))} {tuple(getattr(occ, "shape", ()))}')
    dev = occ.device
    palette = RD._u8_rows(fn, palette, dev, 'palette')
    C = int(palette.shape[0])
    if not 1 <= C <= 256:
        raise ValueError(f'{fn}: a palette of {C} rows: labels are stored as u8, 1 .. 256 classes')
    pr = np.asarray(point_cloud_range, np.float64).reshape(-1)
    if pr.shape != (6,) or not np.all(pr[3:] > pr[:3]):
        raise ValueError(f'{fn}: point_cloud_range = {point_cloud_range}')
    X, Y, Z = (int(s) for s in occ.shape)
    ne = 6 * X * Y * Z
    if ne > 1 << 30:
        raise ValueError(f'{fn}: a volume of {X} x {Y} x {Z} voxels: 6 X Y Z is at most 2^30')
    if occ.dtype != torch.uint8:
        occ = torch.where((occ < 0) | (occ > 255), torch.zeros((), dtype=occ.dtype, device=dev), occ).to(torch.uint8)
    occ = occ.contiguous()
    size = (pr[3:] - pr[:3]) / np.array([X, Y, Z], np.float64)
    vol = (ctypes.c_double * 6)(*pr[:3].tolist(), *size.tolist())
    i32 = torch.int32
    mask = torch.empty(ne, dtype=i32, device=dev)
    scratch = torch.empty(ne + ne // 2048 + 8, dtype=i32, device=dev)
    ids = torch.zeros(ne, dtype=torch.int64, device=dev)          # (es_compact_mask moves keys along with the rows: none are needed here)
    sel, src = torch.empty(ne, dtype=torch.int64, device=dev), torch.empty(ne, dtype=i32, device=dev)
    cnt = ctypes.c_int(0)
    P, st = hip.P, hip.stream()
    hip.call('es_occ_face_mask', P(occ), X, Y, Z, C, P(mask), st)
    hip.call('es_compact_mask', P(ids), ne, P(mask), P(scratch), P(sel), P(src), ctypes.addressof(cnt), st)
    F = int(cnt.value)
    verts = torch.empty((4 * F, 3), dtype=torch.float32, device=dev)
    face_label = torch.empty(F, dtype=torch.uint8, device=dev)
    hip.call('es_occ_face_quads', P(occ), X, Y, Z, _dptr(vol), P(src), F, P(verts), P(face_label), st)
    quads = torch.arange(4 * F, dtype=i32, device=dev).reshape(F, 4)
    colors = palette[face_label.long()].repeat_interleave(4, 0)
    return verts, quads, face_label, colors


# ------------------------------------------------------------------------------------------------------------------ host: boxes and PLY
BOX_EDGES = [(lo, lo | (1 << a)) for a in range(3) for lo in range(8) if not lo & (1 << a)]     # the edge order of the overlays


def box_edges(boxes, colors):
    """boxes (n, 9) and colors (n, 3) u8 on the host -> (verts (8n, 3) f64, edges (12n, 2) int32, edge_colors (12n, 3) u8): corner c of a box
    = centre + R_ZXY (+-l/2, +-w/2, +-h/2) with the sign of axis a positive iff bit a of c, the twelve edges in the overlays' order"""
    b = np.asarray(boxes.detach().cpu() if isinstance(boxes, torch.Tensor) else boxes, np.float32).reshape(-1, 9)
    col = np.asarray(colors.detach().cpu() if isinstance(colors, torch.Tensor) else colors)
    n = len(b)
    if col.dtype != np.uint8 or col.shape != (n, 3):
        raise ValueError(f'scene_cloud.box_edges: colors are uint8 ({n}, 3), got {col.dtype} {col.shape}')
    verts = np.zeros((n, 8, 3), np.float64)
    for i in range(n):
        c, h = b[i, :3].astype(np.float64), b[i, 3:6].astype(np.float64) * 0.5
        a, be, g = (np.float64(x) for x in b[i, 6:9])
        ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(be), np.sin(be), np.cos(g), np.sin(g)
        Rm = np.array([[ca * cc - sa * sb * sc, -(sa * cb), ca * sc + sa * sb * cc],
                       [sa * cc + ca * sb * sc, ca * cb, sa * sc - ca * sb * cc],
                       [-(cb * sc), sb, cb * cc]])
        for k in range(8):
            l = [h[ax] if k & (1 << ax) else -h[ax] for ax in range(3)]
            verts[i, k] = [c[r] + ((Rm[r, 0] * l[0] + Rm[r, 1] * l[1]) + Rm[r, 2] * l[2]) for r in range(3)]
    edges = (np.asarray(BOX_EDGES, np.int32)[None] + 8 * np.arange(n, dtype=np.int32)[:, None, None]).reshape(-1, 2)
    return verts.reshape(-1, 3), edges, np.repeat(col, 12, 0)


_PLY_TYPES = {'int8': 'char', 'uint8': 'uchar', 'int16': 'short', 'uint16': 'ushort', 'int32': 'int', 'uint32': 'uint', 'float32': 'float',
              'float64': 'double'}
_PLY_DTYPES = {v: '<' + np.dtype(k).str[1:] for k, v in _PLY_TYPES.items()}


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def vertex_columns(xyz, rgb=None, **extra):
    """(n, 3) positions (+ (n, 3) u8 colours, + named 1-d columns) -> the `vertex` dict of write_ply: x y z [red green blue] ..."""
    xyz = _host(xyz)
    out = dict(x=xyz[:, 0], y=xyz[:, 1], z=xyz[:, 2])
    if rgb is not None:
        rgb = _host(rgb)
        out.update(red=rgb[:, 0], green=rgb[:, 1], blue=rgb[:, 2])
    out.update({k: _host(v) for k, v in extra.items()})
    return out


def write_ply(path, vertex, face=None, edge=None):
    """binary_little_endian 1.0.  vertex: dict name -> 1-d array (properties in the dict's order, typed by the arrays' dtypes); face: (F, k)
    integer array written as `list uchar int vertex_indices`; edge: (pairs (E, 2) integer, colors (E, 3) u8) written as vertex1 vertex2 red
    green blue.  Arrays or tensors."""
    cols = {k: np.ascontiguousarray(_host(v)) for k, v in vertex.items()}
    n = len(next(iter(cols.values()))) if cols else 0
    head = ['ply', 'format binary_little_endian 1.0', f'element vertex {n}']
    fields = []
    for k, v in cols.items():
        if v.ndim != 1 or len(v) != n or v.dtype.name not in _PLY_TYPES:
            raise ValueError(f'write_ply: vertex property {k!r}: a 1-d array of {n} values of a PLY scalar type, got {v.dtype} {v.shape}')
        head.append(f'property {_PLY_TYPES[v.dtype.name]} {k}')
        fields.append((k, _PLY_DTYPES[_PLY_TYPES[v.dtype.name]]))
    body = []
    rec = np.empty(n, dtype=fields) if fields else np.empty(0, dtype=np.uint8)
    for k, v in cols.items():
        rec[k] = v
    body.append(rec.tobytes())
    if face is not None:
        f = np.ascontiguousarray(_host(face))
        if f.ndim != 2 or not 1 <= f.shape[1] <= 255 or f.dtype.kind not in 'iu':
            raise ValueError(f'write_ply: face is an (F, k) integer array, got {f.dtype} {f.shape}')
        head += [f'element face {len(f)}', 'property list uchar int vertex_indices']
        frec = np.empty(len(f), dtype=[('n', 'u1'), ('v', '<i4', (f.shape[1],))])
        frec['n'], frec['v'] = f.shape[1], f
        body.append(frec.tobytes())
    if edge is not None:
        pairs, ecol = (np.ascontiguousarray(_host(a)) for a in edge)
        if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype.kind not in 'iu' or ecol.dtype != np.uint8 or ecol.shape != (len(pairs), 3):
            raise ValueError(f'write_ply: edge is (pairs (E, 2) integer, colors (E, 3) uint8), got {pairs.dtype} {pairs.shape}, {ecol.dtype} {ecol.shape}')
        head += [f'element edge {len(pairs)}', 'property int vertex1', 'property int vertex2', 'property uchar red', 'property uchar green',
                 'property uchar blue']
        erec = np.empty(len(pairs), dtype=[('a', '<i4'), ('b', '<i4'), ('c', 'u1', (3,))])
        erec['a'], erec['b'], erec['c'] = pairs[:, 0], pairs[:, 1], ecol
        body.append(erec.tobytes())
    head.append('end_header')
    with open(path, 'wb') as fh:
        fh.write(('\n'.join(head) + '\n').encode('ascii'))
        for b in body:
            fh.write(b)
    return path


def read_ply(path):
    """what write_ply wrote -> dict(vertex = dict name -> array, face = (F, k) int32 or None, edge = (pairs (E, 2) int32, colors (E, 3) u8) or
    None).  Binary little-endian files with scalar vertex properties, one list property per face (every face of one length) and scalar edge
    properties."""
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.index(b'end_header\n') + len(b'end_header\n')
    lines = data[:end].decode('ascii').split('\n')
    if lines[0] != 'ply' or lines[1] != 'format binary_little_endian 1.0':
        raise ValueError(f'read_ply: {path}: not a binary little-endian PLY file')
    elements = []
    for ln in lines[2:]:
        tok = ln.split()
        if tok[:1] == ['element']:
            elements.append((tok[1], int(tok[2]), []))
        elif tok[:1] == ['property']:
            elements[-1][2].append(tok[1:])
    out, pos = dict(vertex={}, face=None, edge=None), end
    for name, count, props in elements:
        if any(p[0] == 'list' for p in props):
            if len(props) != 1 or props[0][1:3] != ['uchar', 'int']:
                raise ValueError(f'read_ply: {path}: element {name}: one `list uchar int` property')
            k = data[pos] if count else 0
            rec = np.frombuffer(data, dtype=[('n', 'u1'), ('v', '<i4', (k,))], count=count, offset=pos)
            if count and not (rec['n'] == k).all():
                raise ValueError(f'read_ply: {path}: faces of different lengths')
            pos += rec.nbytes
            out[name] = rec['v'].reshape(count, k).copy()
            continue
        rec = np.frombuffer(data, dtype=[(p[1], _PLY_DTYPES[p[0]]) for p in props], count=count, offset=pos)
        pos += rec.nbytes
        cols = {p[1]: rec[p[1]].copy() for p in props}
        if name == 'edge':
            out['edge'] = (np.stack([cols['vertex1'], cols['vertex2']], -1), np.stack([cols['red'], cols['green'], cols['blue']], -1))
        else:
            out[name] = cols
    if pos != len(data):
        raise ValueError(f'read_ply: {path}: {len(data) - pos} bytes after the last element')
    return out
