"""DenseFusionOccPredictor (embodiedscan/models/detectors/dense_fusion_occ.py:26-330) on the MI355X kernels.

Same registry name, constructor arguments and `forward(inputs, data_samples, mode)` protocol.  Data flow (BASELINE
config 5): multi-view images -> mmdet.ResNet-50 -> mmdet.FPN level 0 -> projection of the 40x40x16 prior voxel centres
into every view (the A8 kernel with explicit float locations) -> image volume (25 600, 256); points -> range
voxelisation at 2.5 mm -> MinkResNet34 -> last level (stride 64 = one voxel of the volume) scattered densely
(25 600, 512); both written into ONE channels-last (25 600, 768) buffer (no cat) -> IndoorImVoxelNeck -> ImVoxelOccHead.
"""
import os

import torch
from ... import engine as E
from ... import hip
from ... import sparse
from ...hip import P, call
from ...params import occ_detector_specs
from ...registry import MODELS, TASK_UTILS
from ...sparse import SparseTensor
from ..layers.fusion_layers.point_fusion import build_fusion_meta
from .base import DetectorBase

C3 = 512                     # channels of MinkResNet34's last level: columns [C2, C2 + C3) of the volume buffer

@MODELS.register_module()
class DenseFusionOccPredictor(DetectorBase):
    task, continuous = 'occ', False

    def __init__(self, backbone, backbone_3d, neck, neck_3d, bbox_head, prior_generator, n_voxels, coord_type,
                 use_valid_mask=True, use_xyz_feat=False, point_cloud_range=None, train_cfg=None, test_cfg=None,
                 data_preprocessor=None, init_cfg=None, seed=0, device='cuda:0'):
        from .. import task_modules  # noqa: F401  (registers the prior generator)
        assert use_xyz_feat, 'shipped config: use_xyz_feat=True (the other branch of the reference has a precedence bug, SURVEY Q15)'
        assert not use_valid_mask, 'use_valid_mask=True appends a 4th "level" the reference head cannot consume; shipped: False'
        self.backbone = MODELS.build(backbone)
        self.backbone.act16 = os.environ.get('ES_OCC_ACT16', '1') != '0'   # round 5: its feature maps only feed the FPN laterals (K = 1 row GEMMs that
                                                                              # read bf16 rows): bf16 activation storage as in the other two detectors
        self.backbone_3d = MODELS.build(backbone_3d)
        self.neck = MODELS.build(neck)
        self.neck_3d = MODELS.build(neck_3d)
        bbox_head = dict(bbox_head)
        bbox_head.update(train_cfg=train_cfg, test_cfg=test_cfg)
        self.bbox_head = MODELS.build(bbox_head)
        self.n_voxels = list(n_voxels)
        self.point_cloud_range = list(point_cloud_range)
        pr = prior_generator['ranges'][0]
        self.voxel_stride = 2 ** 6 if backbone_3d['type'] == 'MinkResNet' else 1
        self.voxel_size = [(pr[3] - pr[0]) / self.n_voxels[0] / self.voxel_stride,
                           (pr[4] - pr[1]) / self.n_voxels[1] / self.voxel_stride,
                           (pr[5] - pr[2]) / self.n_voxels[2] / self.voxel_stride]
        self.prior_generator = TASK_UTILS.build(prior_generator)
        self.coord_type = coord_type
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.use_valid_mask, self.use_xyz_feat = use_valid_mask, use_xyz_feat
        specs = occ_detector_specs(base_channels=self.backbone.base, fpn_out=self.neck.out_channels,
                                   neck_in=self.neck_3d.in_channels, neck_out=self.neck_3d.out_channels,
                                   n_blocks=self.neck_3d.n_blocks, num_classes=self.bbox_head.num_classes,
                                   head_in=self.bbox_head.in_channels)
        self._init_base(specs, device, seed, data_preprocessor)
        self._bucket_groups = self.bucket_groups_for(self.neck_3d.n_scales)
        self._prior = None

    # gradient buckets: part 0 = the image branch (ResNet-50 + FPN: complete last), 1 = MinkResNet34, 2 = the fine half of
    # the dense neck (down_layer_0/1: 0.3 GB), implicit part 3 = the coarse half + head (down_layer_2, up / out blocks: 2.6 GB of
    # the 2.9 GB of gradients) -- its all-reduce starts when the reverse replay leaves down_layer_2, in 256 MB chunks, under
    # the backward of the fine neck levels and both backbones instead of as one 2.9 GB call at the end
    # Part 2 must be exactly the down layers recorded BEFORE the neck's tape mark (imvoxel_neck.forward places it in front of
    # down_layer_{n_scales - 1}): derived from the neck's depth, not hard-coded (round-3 advisor: with n_blocks of another
    # length a down layer behind the mark would have been all-reduced before its gradient was complete).
    @staticmethod
    def bucket_groups_for(n_scales):
        return (('backbone.', 'neck.'), ('backbone_3d.',), tuple(f'neck_3d.down_layer_{i}.' for i in range(n_scales - 1)))

    _bucket_groups = (('backbone.', 'neck.'), ('backbone_3d.',), ('neck_3d.down_layer_0.', 'neck_3d.down_layer_1.'))   # n_scales = 3

    def _children(self):
        return [(self.backbone, 'backbone.'), (self.neck, 'neck.'), (self.backbone_3d, 'backbone_3d.'),
                (self.neck_3d, 'neck_3d.'), (self.bbox_head, 'bbox_head.')]

    def prior_points(self, origin=None):
        """(X*Y*Z, 3) f32 prior voxel centres in VOLUME row order ((x*Y + y)*Z + z), + the scan origin
        (dense_fusion_occ.py:156-162); the reference's list is z-major, re-ordered exactly like its volume reshape/permute
        (:216-217)."""
        if self._prior is None:
            X, Y, Z = self.n_voxels
            a = self.prior_generator.grid_anchors([self.n_voxels[::-1]], device='cpu')[0][:, :3]
            self._prior = a.reshape(Z, Y, X, 3).permute(2, 1, 0, 3).reshape(-1, 3).contiguous()
        p = self._prior
        if origin is not None:
            p = p + torch.as_tensor(origin, dtype=torch.float32)
        return p

    def _batch_rule(self, B, V, points, batch_data_samples):
        """refuses a batch this class cannot take (before anything is launched) -> (volumes the neck sees, the metas of the image samples)"""
        assert B == 1, 'only support batch_size=1 here (dense_fusion_occ.py:160,251)'
        return B, [ds.metainfo for ds in batch_data_samples]

    def _project(self, f2d, Hf, Wf, prior, meta_dev, V, vol):
        """the prior voxel centres into every view: the mean of the views' features into columns [0, C2) of `vol`.  Returns
        bwd(g, acc): the gradient rows `g` of `vol` gathered back into f2d.g (acc 0: the gather overwrites it)."""
        nvox, C2, ld = prior.shape[0], f2d.d.shape[1], vol.shape[1]
        bidx = torch.zeros((nvox, 4), dtype=torch.int32, device=self.device)            # column 0 = sample index (0: B == 1)
        pix = torch.empty((nvox, V), dtype=torch.int32, device=self.device)
        cnt = torch.empty(nvox, dtype=torch.int32, device=self.device)
        call('es_point_sample_fwd_pts', P(bidx), P(prior), nvox, P(meta_dev), meta_dev.shape[1], V, P(f2d.d), Hf, Wf, C2,
             P(vol), ld, P(pix), P(cnt), hip.stream())
        E.mark('image volume (projection)')

        def bwd(g, acc):
            head = torch.empty(f2d.d.shape[0], dtype=torch.int32, device=self.device)
            nxt = torch.empty(nvox * V, dtype=torch.int32, device=self.device)
            call('es_point_sample_bwd', P(bidx), nvox, V, P(g), ld, P(pix), P(cnt), Hf, Wf, C2, P(f2d.g), V, P(head), P(nxt), acc,
                 hip.stream())
        return bwd

    def image_maps(self, img):
        """(B, V, 3, H, W) frames -> FPN level 0 of the B V views: (Var (B V Hf Wf, C2), Hf, Wf).  A frame block that already lies
        channels-last in memory (a walk's staged frame) is taken as it is."""
        B, V = img.shape[:2]
        H, W = img.shape[-2:]
        if img.stride(2) != 1:
            img = img.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
        nhwc = img.permute(0, 1, 3, 4, 2).reshape(B * V, H, W, 3)
        E.refresh_weight_copies()
        return self.neck(self.backbone(nhwc), B * V, levels=[0])[0]

    def point_branch(self, clouds, vol, C2, rows=None, on_backbone=None):
        """voxelise `clouds` (one batch entry each), MinkResNet on the xyz rows, its last level (stride 64 = one voxel of the volume)
        scattered into columns [C2, C2 + C3) of `vol` (SparseTensor.dense()) -> (x3, didx = the volume row of every x3 row).  `rows`:
        the clouds' rows in batch order as ONE tensor, from which the xyz features are gathered by its own row stride -- a walk passes
        the buffer that holds its one cloud; None: a packed (n, 3) copy is made here.  on_backbone: called right behind the 3-D
        backbone (the tape mark of a loss forward)."""
        X, Y, Z = self.n_voxels
        rmin = self.point_cloud_range[:3]
        cmax = [n * self.voxel_stride - 1 for n in self.n_voxels]
        cs, src = sparse.voxelize_range(clouds, rmin, self.voxel_size, cmax)
        if rows is None:
            rows = torch.cat([p[:, :3] for p in clouds]) if len(clouds) > 1 else clouds[0][:, :3].contiguous()
        feats = torch.empty((cs.n, 3), dtype=torch.float32, device=self.device)
        call('es_row_move', P(feats), 3, P(rows), rows.stride(0), P(src), cs.n, 3, 0, hip.stream())
        x3 = self.backbone_3d(SparseTensor(cs, E.Var(feats, rg=False)))[-1]
        if on_backbone is not None:
            on_backbone()
        assert x3.F.d.shape[1] == C3 and x3.cs.ts == self.voxel_stride
        didx = torch.empty(x3.cs.n, dtype=torch.int32, device=self.device)
        call('es_dense_index', P(x3.cs.coords), x3.cs.n, x3.cs.ts, X, Y, Z, P(didx), hip.stream())
        call('es_row_move', vol.data_ptr() + 4 * C2, C2 + C3, P(x3.F.d), C3, P(didx), x3.cs.n, C3, 2, hip.stream())
        return x3, didx

    def extract_feat(self, batch_inputs_dict, batch_data_samples):
        """dense_fusion_occ.py:120-259 (EmbodiedOccPredictor: embodied_occ.py:118-247, n = T prefix-major volumes).
        Returns [(Var (n*X_i*Y_i*Z_i, 128), (X_i, Y_i, Z_i))] fine -> coarse."""
        self._bind()
        self.start_tape_parts()
        img = batch_inputs_dict['imgs']
        B, V = img.shape[:2]
        H, W = img.shape[-2:]
        n, metas = self._batch_rule(B, V, batch_inputs_dict['points'], batch_data_samples)
        f2d, Hf, Wf = self.image_maps(img)
        E.mark('2-D backbone + FPN')
        self.tape_part(1)                       # behind this point: 3-D backbone, then the neck parts
        X, Y, Z = self.n_voxels
        origin = metas[0]['depth2img'].get('origin') if isinstance(metas[0].get('depth2img'), dict) else None
        prior = self.prior_points(origin).to(self.device, non_blocking=True)
        meta_dev = build_fusion_meta(metas, self.coord_type, (H, W), V).to(self.device, non_blocking=True)
        C2 = f2d.d.shape[1]
        vol = torch.zeros((n * X * Y * Z, C2 + C3), dtype=torch.float32, device=self.device)
        project_bwd = self._project(f2d, Hf, Wf, prior, meta_dev, V, vol)
        pts = [p if (p.dtype == torch.float32 and p.stride(-1) == 1) else p.float().contiguous() for p in batch_inputs_dict['points']]
        x3, didx = self.point_branch(pts, vol, C2, on_backbone=lambda: self.tape_part(2))
        E.mark('point branch (voxelise + MinkResNet + dense)')
        v = E.Var(vol)

        def bwd(v=v, x3=x3, f2d=f2d):
            if v.g is None:
                return
            g3 = torch.empty_like(x3.F.d)
            call('es_row_move', P(g3), C3, v.g.data_ptr() + 4 * C2, C2 + C3, P(didx), x3.cs.n, C3, 0, hip.stream())
            if x3.F.g is None:
                x3.F.g = g3
            else:
                E.add_into(x3.F.g, g3)
            if f2d.rg:
                acc = 1
                if f2d.g is None:
                    f2d.g, acc = torch.empty_like(f2d.d), 0         # the gather writes every pixel
                project_bwd(v.g, acc)
        E.TAPE.add(bwd)
        outs = self.neck_3d(v, (X, Y, Z), n, on_coarse=lambda: self.tape_part(3))
        E.mark('IndoorImVoxelNeck')
        return outs

    def loss(self, batch_inputs_dict, batch_data_samples, **kwargs):
        x = self.extract_feat(batch_inputs_dict, batch_data_samples)
        return self.bbox_head.loss(x, batch_data_samples, **kwargs)

    def predict(self, batch_inputs_dict, batch_data_samples, **kwargs):
        with self._predict_guard():
            x = self.extract_feat(batch_inputs_dict, batch_data_samples)
            pred = self.bbox_head.predict(x, batch_data_samples)
        for i, ds in enumerate(batch_data_samples):
            ds.pred_occupancy = pred[i]
        return batch_data_samples
