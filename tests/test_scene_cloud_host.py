"""The host side of embodiedscan_amd.scene_cloud, without a device: a PLY round trip of every element kind with the header checked byte
for byte, box_edges against the render spec's corners and edge order, CloudFull's message, and every ValueError of add / label /
occupancy_mesh that is raised before a launch.  Also the spec's own arithmetic: es_hash against Python integers, longest_run on a table
worked by hand."""
import numpy as np
import pytest
import torch

import render_spec as RS
import scene_cloud_spec as S
from embodiedscan_amd import scene_cloud as SC


def test_ply_round_trip_of_every_element_kind(tmp_path):
    rng = np.random.default_rng(1)
    n = 7
    vertex = dict(x=rng.normal(size=n).astype(np.float32), y=rng.normal(size=n).astype(np.float32), z=rng.normal(size=n).astype(np.float32),
                  red=rng.integers(0, 256, n, dtype=np.uint8), green=rng.integers(0, 256, n, dtype=np.uint8), blue=rng.integers(0, 256, n, dtype=np.uint8),
                  hits=rng.integers(0, 2 ** 31 - 1, n).astype(np.int32), label=np.arange(n, dtype=np.int32) - 1, instance=-np.arange(n, dtype=np.int32))
    face = np.array([[0, 1, 2, 3], [3, 4, 5, 6]], np.int32)
    pairs, ecol = np.array([[0, 1], [1, 6], [2, 5]], np.int32), rng.integers(0, 256, (3, 3), dtype=np.uint8)
    path = str(tmp_path / 'all.ply')
    assert SC.write_ply(path, vertex, face=face, edge=(pairs, ecol)) == path
    head = ('ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n'
            'property uchar green\nproperty uchar blue\nproperty int hits\nproperty int label\nproperty int instance\nelement face 2\n'
            'property list uchar int vertex_indices\nelement edge 3\nproperty int vertex1\nproperty int vertex2\nproperty uchar red\n'
            'property uchar green\nproperty uchar blue\nend_header\n').encode('ascii')
    raw = open(path, 'rb').read()
    assert raw[:len(head)] == head
    assert len(raw) == len(head) + n * (3 * 4 + 3 + 3 * 4) + 2 * (1 + 4 * 4) + 3 * (2 * 4 + 3)
    body = raw[len(head):]
    assert np.frombuffer(body[:4], '<f4')[0] == vertex['x'][0] and body[12:15] == bytes([vertex['red'][0], vertex['green'][0], vertex['blue'][0]])
    back = SC.read_ply(path)
    assert list(back['vertex']) == list(vertex)
    for k, v in vertex.items():
        assert back['vertex'][k].dtype == v.dtype and np.array_equal(back['vertex'][k], v), k
    assert np.array_equal(back['face'], face) and back['face'].dtype == np.int32
    assert np.array_equal(back['edge'][0], pairs) and np.array_equal(back['edge'][1], ecol)
    # vertices alone, tensors, other scalar types, no rows
    cols = SC.vertex_columns(torch.arange(6, dtype=torch.float32).reshape(2, 3), torch.tensor([[1, 2, 3], [4, 5, 6]], dtype=torch.uint8),
                             w=np.array([0.5, 1.5]), s=np.array([-3, 4], np.int16))
    back = SC.read_ply(SC.write_ply(str(tmp_path / 'v.ply'), cols))
    assert list(back['vertex']) == ['x', 'y', 'z', 'red', 'green', 'blue', 'w', 's'] and back['face'] is None and back['edge'] is None
    assert back['vertex']['w'].dtype == np.float64 and back['vertex']['s'].tolist() == [-3, 4] and back['vertex']['blue'].tolist() == [3, 6]
    none = SC.read_ply(SC.write_ply(str(tmp_path / 'e.ply'), SC.vertex_columns(np.zeros((0, 3), np.float32)), face=np.zeros((0, 4), np.int32),
                                    edge=(np.zeros((0, 2), np.int32), np.zeros((0, 3), np.uint8))))
    assert none['vertex']['x'].shape == (0,) and none['face'].shape[0] == 0 and none['edge'][0].shape == (0, 2)
    for bad, msg in ((lambda: SC.write_ply(path, dict(x=np.zeros((2, 2), np.float32))), 'vertex property'),
                     (lambda: SC.write_ply(path, dict(x=np.zeros(2, np.float32), y=np.zeros(3, np.float32))), 'vertex property'),
                     (lambda: SC.write_ply(path, dict(x=np.zeros(2, np.int64))), 'vertex property'),
                     (lambda: SC.write_ply(path, dict(x=np.zeros(2, np.float32)), face=np.zeros((2, 3), np.float32)), 'face'),
                     (lambda: SC.write_ply(path, dict(x=np.zeros(2, np.float32)), edge=(np.zeros((2, 2), np.int32), np.zeros((2, 3), np.int32))), 'edge')):
        with pytest.raises(ValueError, match=msg):
            bad()
    with open(str(tmp_path / 'ascii.ply'), 'w') as f:
        f.write('ply\nformat ascii 1.0\nelement vertex 0\nend_header\n')
    with pytest.raises(ValueError, match='binary'):
        SC.read_ply(str(tmp_path / 'ascii.ply'))


def test_box_edges_against_the_render_spec():
    boxes = RS.population(9, 3)
    colors = RS.colours(9, 4)
    verts, edges, ecol = SC.box_edges(boxes, colors)
    assert verts.shape == (72, 3) and verts.dtype == np.float64 and edges.shape == (108, 2) and edges.dtype == np.int32 and ecol.shape == (108, 3)
    for i, b in enumerate(boxes):
        Rm, c, h = RS.rotation(b[6:9]), b[:3].astype(np.float64), b[3:6].astype(np.float64) * 0.5
        for k in range(8):
            l = np.array([h[a] if k & (1 << a) else -h[a] for a in range(3)])
            want = [c[r] + ((Rm[r, 0] * l[0] + Rm[r, 1] * l[1]) + Rm[r, 2] * l[2]) for r in range(3)]
            assert verts[8 * i + k].tolist() == want
        assert (edges[12 * i:12 * i + 12] - 8 * i).tolist() == [list(e) for e in RS.EDGES]
        assert (ecol[12 * i:12 * i + 12] == colors[i]).all()
    assert SC.box_edges(np.zeros((0, 9)), np.zeros((0, 3), np.uint8))[0].shape == (0, 3)
    same = SC.box_edges(torch.from_numpy(boxes), torch.from_numpy(colors))
    assert np.array_equal(same[0], verts)
    with pytest.raises(ValueError, match='colors'):
        SC.box_edges(boxes, colors[:3])


def test_cloud_full_names_what_fits():
    e = SC.CloudFull(dropped=1234, capacity=128, occupied=128, cell=0.02)
    assert (e.dropped, e.capacity, e.occupied) == (1234, 128, 128)
    assert e.fit_capacity == 4096 and e.fit_capacity & (e.fit_capacity - 1) == 0 and e.fit_capacity >= 2 * (1234 + 128)
    assert e.fit_cell > 0.02 * (2 * 1362 / 128) ** 0.5
    msg = str(e)
    assert '1234 depth pixels' in msg and '128 slots' in msg and 'capacity=4096' in msg and f'cell={e.fit_cell:g}' in msg and '64 probes' in msg
    assert isinstance(e, RuntimeError)
    assert SC.CloudFull(1, 1 << 30, 1 << 30, 0.02).fit_capacity == 1 << 30


def test_value_errors_before_any_launch():
    """on host tensors: every refusal comes before the first launch, so none of this needs a device"""
    cpu = torch.device('cpu')
    for bad, msg in ((lambda: SC.SceneCloud(cpu, cell=0.0), 'cell'), (lambda: SC.SceneCloud(cpu, cell=float('inf')), 'cell'),
                     (lambda: SC.SceneCloud(cpu, capacity=1000), 'capacity'), (lambda: SC.SceneCloud(cpu, capacity=1), 'capacity'),
                     (lambda: SC.SceneCloud(cpu, capacity=1 << 31), 'capacity'), (lambda: SC.SceneCloud(cpu, capacity=8, z=(1.0, 1.0)), 'z cut'),
                     (lambda: SC.SceneCloud(cpu, capacity=8, z=(float('nan'), 1.0)), 'z cut'), (lambda: SC.SceneCloud(cpu, capacity=8, max_depth=0.0), 'max_depth'),
                     (lambda: SC.SceneCloud(cpu, capacity=8, max_depth=4097.0), 'max_depth')):
        with pytest.raises(ValueError, match=msg):
            bad()
    cl = SC.SceneCloud(cpu, capacity=8, z=(-float('inf'), float('inf')))
    assert cl.state_bytes() == 8 * 20 + 8 and bool((cl.tkeys == -1).all())
    d, f = torch.zeros((2, 4, 5)), torch.zeros((2, 3, 4, 5), dtype=torch.uint8)
    E = np.stack([np.eye(4)] * 2)
    for bad, msg in ((lambda: cl.add(d.double(), f, E, E), 'float32'), (lambda: cl.add(d[0], f, E, E), 'float32'), (lambda: cl.add(d, f.float(), E, E), 'uint8'),
                     (lambda: cl.add(d, f[:1], E, E), '1 frames'), (lambda: cl.add(d, f, E[:1], E), 'extrinsic'), (lambda: cl.add(d, f, E, E[:1]), 'intrinsic'),
                     (lambda: cl.add(d, f, E, E, layout='hwc'), 'layout'), (lambda: cl.add(d, torch.zeros((2, 3, 4, 3), dtype=torch.uint8), E, E), 'layout='),
                     (lambda: cl.add(torch.zeros((2, 4, 4097)), f, E, E), '4097'), (lambda: cl.add(d.transpose(1, 2), f, E, E), 'contiguous'),
                     (lambda: cl.points(min_hits=-1), 'min_hits')):
        with pytest.raises(ValueError, match=msg):
            bad()
    xyz, z9 = torch.zeros((3, 3)), torch.zeros((2, 9))
    for bad, msg in ((lambda: SC.label(xyz.double(), z9), 'float32'), (lambda: SC.label(xyz[:, :2], z9), 'float32'), (lambda: SC.label(xyz, z9[:, :8]), r'\(m, 9\)'),
                     (lambda: SC.label(xyz, z9, grow=-0.1), 'grow'), (lambda: SC.label(xyz, z9, grow=float('nan')), 'grow'), (lambda: SC.label(xyz, z9, grow=float('inf')), 'grow'),
                     (lambda: SC.label(xyz, torch.zeros((65536, 9))), '65535'), (lambda: cl.label(np.zeros((3, 3), np.float32), z9), 'float32')):
        with pytest.raises(ValueError, match=msg):
            bad()
    occ, pr, pal = torch.zeros((2, 2, 2), dtype=torch.int64), (0, 0, 0, 1, 1, 1), np.zeros((3, 3), np.uint8)
    for bad, msg in ((lambda: SC.occupancy_mesh(occ.float(), pr, pal), 'integer'), (lambda: SC.occupancy_mesh(occ[0], pr, pal), '3-d'),
                     (lambda: SC.occupancy_mesh(occ[:0], pr, pal), 'non-empty'), (lambda: SC.occupancy_mesh(occ, (0, 0, 0, 1, 1, 0), pal), 'point_cloud_range'),
                     (lambda: SC.occupancy_mesh(occ, pr[:5], pal), 'point_cloud_range'), (lambda: SC.occupancy_mesh(occ, pr, np.zeros((0, 3), np.uint8)), 'palette'),
                     (lambda: SC.occupancy_mesh(occ, pr, np.zeros((257, 3), np.uint8)), 'palette'), (lambda: SC.occupancy_mesh(occ, pr, pal.astype(np.int32)), 'palette'),
                     (lambda: SC.occupancy_mesh(occ == 1, pr, pal), 'integer')):
        with pytest.raises(ValueError, match=msg):
            bad()


def test_the_spec_hash_and_longest_run():
    def mix(k, mask):
        x = k & (2 ** 64 - 1)
        x = ((x ^ (x >> 30)) * 0xbf58476d1ce4e5b9) & (2 ** 64 - 1)
        x = ((x ^ (x >> 27)) * 0x94d049bb133111eb) & (2 ** 64 - 1)
        x ^= x >> 31
        return (x & 0xffffffff) & mask
    keys = np.array([0, 1, 2 ** 53 + 17, int(S.pack(np.array([-2 ** 17, 2 ** 17 - 1, 5]))), 123456789012345], np.int64)
    for mask in (1, 63, 2 ** 30 - 1):
        assert S.es_hash(keys, mask).tolist() == [mix(int(k), mask) for k in keys]
    assert S.unpack(S.pack(np.array([[-2 ** 17, 2 ** 17 - 1, 5], [0, -1, 1]]))).tolist() == [[-2 ** 17, 2 ** 17 - 1, 5], [0, -1, 1]]
    cap = 16
    full = np.zeros(cap, bool)
    keys = np.arange(1000, 1009)
    for k in keys:
        s = mix(int(k), cap - 1)
        while full[s]:
            s = (s + 1) % cap
        full[s] = True
    best = max(len(run) for run in ''.join('x' if b else ' ' for b in np.roll(full, -int(np.flatnonzero(~full)[0]))).split())
    assert S.longest_run(keys, cap) == best and S.longest_run(keys[::-1], cap) == best and S.longest_run(keys[:0], cap) == 0
    assert S.capacity(0) == 2 and S.capacity(1) == 8 and S.capacity(8941) == 65536
    m = S.face_mask(np.array([[[1]]], np.uint8), 2)
    assert m.tolist() == [1] * 6 and S.face_mask(np.array([[[2]]], np.uint8), 2).tolist() == [0] * 6
