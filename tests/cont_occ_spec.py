"""Specification of EmbodiedOccPredictor (embodiedscan/models/detectors/embodied_occ.py:118-273 of the reference), composed from
the oracle's functions without editing them: resnet50_w16 + fpn on the V frames once; batch_point_sample on views 0 .. t for every
prefix t (:165-203); voxelize_range over the T cumulative clouds as batch entries 0 .. T-1; mink_resnet34 on SpT(.., n_batch=T);
its last level scattered densely per batch entry; imvoxel_neck on the (T, C2 + 512, X, Y, Z) volume; the 1x1x1 head convolutions and
head_loss over the T-fold batch.  Used by tests/test_gpu_cont_occ.py.  TEST ORACLE."""
import numpy as np
import torch

from oracle import model as M
from oracle import occ as OO
from oracle import sparse as S


def voxel_coords(points, n_voxels, point_cloud_range, prior_range, stride=64):
    """(coords (N, 4) int32 batch-major, index of each voxel's first point in the concatenated clouds)"""
    vs = [(prior_range[3 + a] - prior_range[a]) / n_voxels[a] / stride for a in range(3)]
    cmax = [n * stride - 1 for n in n_voxels]
    return OO.voxelize_range([p.detach().numpy() for p in points], point_cloud_range[:3], vs, cmax)


def detector_forward(sd, points, imgs, meta, n_voxels, point_cloud_range, prior_range, n_blocks=(1, 1, 1), training=True):
    """points: the T cumulative clouds; imgs (1, V, 3, H, W) preprocessed; -> list of (T, C, Xi, Yi, Zi) logits, fine -> coarse"""
    B, V = imgs.shape[:2]
    T = len(points)
    assert B == 1 and T == V
    x = OO.fpn(M.resnet50_w16(imgs.reshape((-1,) + imgs.shape[2:]), sd), sd)[0]          # (V, C2, Hf, Wf)
    prior = OO.prior_points(list(n_voxels), prior_range)
    if 'origin' in meta['depth2img']:
        prior = prior + torch.as_tensor(meta['depth2img']['origin'], dtype=prior.dtype)
    sf = torch.tensor(meta['scale_factor'][:2], dtype=torch.float32) if 'scale_factor' in meta else 1
    off = torch.tensor(meta['img_crop_offset'], dtype=torch.float32) if 'img_crop_offset' in meta else 0
    proj = M.projection_matrices(meta)
    vols = []
    for t in range(T):
        vol = M.batch_point_sample(meta, x[:t + 1], prior.to(x.dtype), proj[:t + 1], sf, off, meta.get('flip', False), imgs.shape[-2:],
                                   meta['img_shape'][:2])
        vols.append(vol.reshape(list(n_voxels[::-1]) + [-1]).permute(3, 2, 1, 0))
    img_volume = torch.stack(vols)                                                       # (T, C2, X, Y, Z)
    stride = 64
    coords, src = voxel_coords(points, n_voxels, point_cloud_range, prior_range, stride)
    f = torch.cat([p[:, :3] for p in points])[torch.from_numpy(src)].to(x.dtype)
    last = M.mink_resnet34(S.SpT(coords, f, 1, T, {}), sd, training=training)[-1]
    X, Y, Z = n_voxels
    dense = f.new_zeros((T * X * Y * Z, last.feats.shape[1]))
    c = torch.from_numpy(last.coords.astype(np.int64))
    cc = c[:, 1:] // stride
    dense = dense.index_copy(0, ((c[:, 0] * X + cc[:, 0]) * Y + cc[:, 1]) * Z + cc[:, 2], last.feats)
    point_volume = dense.reshape(T, X, Y, Z, -1).permute(0, 4, 1, 2, 3)
    x3 = OO.imvoxel_neck(torch.cat([img_volume, point_volume], 1), sd, n_blocks=n_blocks, training=training)
    return [OO._conv3d(l, sd[f'bbox_head.occ.{i}.weight'], 1, 0) for i, l in enumerate(x3)]


def detector_loss(sd, points, imgs, meta, gt_occupancy, gt_masks, n_voxels, point_cloud_range, prior_range, n_blocks=(1, 1, 1)):
    """gt_occupancy (N, 4) shared by the T samples, gt_masks: the T per-prefix masks -> ({'loss_occ_i'}, dict(preds, parts))"""
    preds = detector_forward(sd, points, imgs, meta, n_voxels, point_cloud_range, prior_range, n_blocks)
    losses, parts = OO.head_loss(preds, [gt_occupancy] * len(points), gt_masks, return_parts=True)
    return losses, dict(preds=preds, parts=parts)
