"""The host side of embodiedscan_amd.inference (no GPU): synth.write_demo_scene -> scene_info round trip of the pose convention, the
skipped first pose line, the quaternion reading against scipy (when it imports) and against quarter turns in closed form, and the
errors of malformed folders."""
import math
import os

import numpy as np
import pytest

from embodiedscan_amd import inference as I
from embodiedscan_amd.synth import write_demo_scene


@pytest.fixture(scope='module')
def scene(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('demo'))
    return root, write_demo_scene(root, 'room', n_frames=4, height=60, width=80, seed=3)


def test_round_trip_of_the_pose_convention(scene):
    root, w = scene
    info = I.scene_info(os.path.join(root, 'room'))
    assert info['scan_id'] == info['sample_idx'] == 'demo/room'
    assert len(info['img_path']) == len(info['depth_img_path']) == len(info['images']) == 4
    assert [os.path.basename(p) for p in info['img_path']] == [s + '.jpg' for s in w['timestamps']]
    assert [os.path.basename(p) for p in info['depth_img_path']] == [s + '.png' for s in w['timestamps']]
    for v in range(4):
        want = np.linalg.inv(w['axis_align'] @ w['cam2global'][v])
        got = info['depth2img']['extrinsic'][v]
        assert got.dtype == np.float32 and got.shape == (4, 4)
        err = float(np.abs(got.astype(np.float64) - want).max())
        assert err < 1e-6, f'frame {v}: extrinsic off by {err:.2e}'
        # ... which is the scan's own world -> camera matrix (the axis alignment cancels)
        assert float(np.abs(got - w['scan']['extrinsic'][v]).max()) < 1e-5
        # (the written rotation is the inverse of an f32 matrix, orthonormal to f32 rounding only; the quaternion holds the nearest rotation)
        assert float(np.abs(info['images'][v]['cam2global'] - w['cam2global'][v]).max()) < 1e-6
    K = w['scan']['intrinsic'][0]
    for k in ('depth_cam2img', 'cam2img'):
        assert info[k].dtype == np.float32 and np.array_equal(info[k], K)
    assert np.array_equal(info['depth2img']['intrinsic'], K) and np.array_equal(info['depth2img']['origin'], np.float32([0, 0, .5]))
    assert np.allclose(info['axis_align_matrix'], w['axis_align'], atol=0, rtol=0) and info['depth_shift'] == 1000.0
    ann = info['ann_info']
    assert ann['gt_bboxes_3d'].shape == (0, 9) and ann['gt_labels_3d'].shape == (0,) and ann['gt_occupancy'].shape == (0, 4)
    assert len(ann['visible_instance_masks']) == 4
    assert np.array_equal(I.scene_info(os.path.join(root, 'room'), origin=(1, 2, 3), depth_shift=500.)['depth2img']['origin'], np.float32([1, 2, 3]))


def test_line_zero_is_skipped_by_default(scene):
    root, w = scene
    every = I.scene_info(os.path.join(root, 'room'), skip_first=False)
    assert len(every['img_path']) == 5 and os.path.basename(every['img_path'][0]) == '00000.jpg'
    first = np.identity(4)
    first[:3, :3] = I.CAM_AXES                                          # the identity pose of line 0
    assert np.allclose(every['depth2img']['extrinsic'][0], np.linalg.inv(w['axis_align'] @ first), atol=1e-6)
    default = I.scene_info(os.path.join(root, 'room'))
    assert every['img_path'][1:] == default['img_path']
    assert all(np.array_equal(a, b) for a, b in zip(every['depth2img']['extrinsic'][1:], default['depth2img']['extrinsic']))


def test_the_pipeline_reads_the_folder(scene):
    """scene_info is what ScanPipeline.__call__ consumes: the decoded depth is the written scan's, to the millimetre"""
    from embodiedscan_amd.datasets.loading import ScanPipeline
    root, w = scene
    sp = ScanPipeline(n_images=4, ordered=True, n_points=500, view_points=200, img_scale=(80, 60))
    scan = sp(I.scene_info(os.path.join(root, 'room')), np.random.RandomState(0))
    assert scan['depth'].shape == (4, 60, 80) and scan['img_raw'].shape == (4, 60, 80, 3)
    assert float(np.abs(scan['depth'] - w['scan']['depth']).max()) <= 0.5e-3 + 1e-6
    assert scan['meta']['sample_idx'] == 'demo/room' and scan['gt_boxes'].shape == (0, 9)
    assert float(np.abs(scan['extrinsic'] - w['scan']['extrinsic']).max()) < 1e-5


def test_quaternions():
    """scalar last; unnormalised quaternions are normalised; quarter turns in closed form; scipy's Rotation when it imports"""
    h = math.sqrt(0.5)
    cases = {(0, 0, 0, 1): np.eye(3),
             (0, 0, h, h): [[0, -1, 0], [1, 0, 0], [0, 0, 1]],            # +90 degrees about z
             (h, 0, 0, h): [[1, 0, 0], [0, 0, -1], [0, 1, 0]],            # about x
             (0, h, 0, h): [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],            # about y
             (0, 0, 1, 0): [[-1, 0, 0], [0, -1, 0], [0, 0, 1]],           # 180 degrees about z
             (0, 0, 3, 3): [[0, -1, 0], [1, 0, 0], [0, 0, 1]],            # not normalised
             (0, 0, -h, -h): [[0, -1, 0], [1, 0, 0], [0, 0, 1]]}          # q and -q are one rotation
    for q, want in cases.items():
        assert np.allclose(I.quat_to_matrix(q), np.asarray(want, float), atol=1e-15), q
    rng = np.random.default_rng(5)
    qs = rng.normal(size=(50, 4)) * rng.uniform(0.1, 10, (50, 1))
    for q in qs:
        m = I.quat_to_matrix(q)
        assert np.allclose(m @ m.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(m) - 1) < 1e-14
    try:
        from scipy.spatial.transform import Rotation
    except ImportError:
        Rotation = None
    if Rotation is not None:
        for q in qs:
            assert np.allclose(I.quat_to_matrix(q), Rotation.from_quat(q).as_matrix(), atol=1e-14)
    with pytest.raises(ValueError, match='quaternion'):
        I.quat_to_matrix([0, 0, 0, 0])
    from embodiedscan_amd.synth import _matrix_to_quat
    for q in qs:                                                          # the writer's inverse, on every branch
        m = I.quat_to_matrix(q)
        assert np.allclose(I.quat_to_matrix(_matrix_to_quat(m)), m, atol=1e-14)
    for q in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (h, h, 0, 0)):
        m = I.quat_to_matrix(q)
        assert np.allclose(I.quat_to_matrix(_matrix_to_quat(m)), m, atol=1e-14)


def test_malformed_folders(tmp_path):
    import shutil
    root = str(tmp_path)
    write_demo_scene(root, 'bad', n_frames=2, height=12, width=16, seed=1)
    d = os.path.join(root, 'bad')
    keep = {n: open(os.path.join(d, n)).read() for n in ('intrinsic.txt', 'axis_align_matrix.txt', 'poses.txt')}
    for name in ('intrinsic.txt', 'axis_align_matrix.txt'):
        np.savetxt(os.path.join(d, name), np.eye(3))
        with pytest.raises(ValueError, match='4 x 4'):
            I.scene_info(d)
        open(os.path.join(d, name), 'w').write(keep[name])
    open(os.path.join(d, 'poses.txt'), 'w').write(keep['poses.txt'] + '00009 1 2 3 0 0 0\n')
    with pytest.raises(ValueError, match='line 3'):
        I.scene_info(d)
    open(os.path.join(d, 'poses.txt'), 'w').write(keep['poses.txt'])
    assert len(I.scene_info(d)['img_path']) == 2
    os.remove(os.path.join(d, 'depth', '00002.png'))
    with pytest.raises(FileNotFoundError, match='00002.png'):
        I.scene_info(d)
    shutil.rmtree(os.path.join(d, 'rgb'))
    with pytest.raises(FileNotFoundError, match='00001.jpg'):
        I.scene_info(d)
