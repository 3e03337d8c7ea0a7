"""Specification of Embodied3DDetector (embodiedscan/models/detectors/embodied_det3d.py:90-266 of the reference), composed from the
oracle's functions without editing them: resnet50_w16 once on the V frames; voxelize over the T cumulative clouds as batch entries
0 .. T-1; mink_resnet34 on SpT(.., n_batch=T); per level and prefix t, batch_point_sample on views 0 .. t (:170-185:
`img_features[level][0][:idx + 1]`, `proj_mat[:idx + 1]`); head_forward and loss_single per prefix, the means as in
oracle.model.detector_loss.  Used by tests/test_gpu_cont_det.py.  TEST ORACLE."""
import torch

from oracle import coords as C
from oracle import model as M
from oracle import sparse as S


def extract_feat(sd, points, imgs, meta, voxel_size=0.01, training=True, trace=None):
    """points: the T cumulative clouds; imgs (1, V, 3, H, W) preprocessed; meta: the one meta the T samples share"""
    B, V = imgs.shape[:2]
    T = len(points)
    assert B == 1 and T == V
    coords, src = C.voxelize([p.detach().numpy() for p in points], voxel_size)
    feats = torch.cat([p[:, :3] for p in points])[torch.from_numpy(src)]
    xs = M.mink_resnet34(S.SpT(coords, feats, 1, T, {}), sd, training=training, trace=trace)
    img_feats = M.resnet50_w16(imgs.reshape((-1,) + imgs.shape[2:]), sd)                 # per level (V, C, Hf, Wf)
    proj = M.projection_matrices(meta)
    sf = torch.tensor(meta['scale_factor'][:2], dtype=torch.float32) if 'scale_factor' in meta else 1
    off = torch.tensor(meta['img_crop_offset'], dtype=torch.float32) if 'img_crop_offset' in meta else 0
    outs = []
    for lvl, xl in enumerate(xs):
        per_prefix = []
        for t in range(T):
            rows = xl.batch_rows(t)
            pts = (torch.from_numpy(xl.coords[rows, 1:]).float() * voxel_size).to(xl.feats.dtype)
            per_prefix.append(M.batch_point_sample(meta, img_feats[lvl][:t + 1], pts, proj[:t + 1], sf, off, meta.get('flip', False),
                                                   imgs.shape[-2:], meta['img_shape'][:2]))
        outs.append(xl.new(torch.cat([xl.feats, torch.cat(per_prefix)], 1)))
    return outs


def detector_loss(sd, points, imgs, meta, gt_boxes, gt_labels, voxel_size=0.01, thr=100000, training=True, return_aux=False,
                  targets_override=None, trace=None):
    """gt_boxes / gt_labels: the T per-prefix lists -> dict(loss_center, loss_bbox, loss_cls) (means over the prefixes)"""
    xs = extract_feat(sd, points, imgs, meta, voxel_size, training, trace)
    outs = M.head_forward(xs, sd, voxel_size=voxel_size, thr=thr, training=training, trace=trace)
    cl, bl, kl, aux = [], [], [], []
    for t in range(len(points)):
        c, bb, k, tg = M.loss_single([outs[l][t] for l in range(len(outs))], gt_boxes[t], gt_labels[t],
                                     targets_override=None if targets_override is None else targets_override[t])
        cl.append(c), bl.append(bb), kl.append(k), aux.append(tg)
    losses = dict(loss_center=torch.stack(cl).mean(), loss_bbox=torch.stack(bl).mean(), loss_cls=torch.stack(kl).mean())
    if return_aux:
        return losses, dict(xs=xs, outs=outs, targets=aux)
    return losses
