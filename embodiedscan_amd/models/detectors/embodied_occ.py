"""EmbodiedOccPredictor (embodiedscan/models/detectors/embodied_occ.py:25-345) on the MI355X kernels: continuous occupancy.

Frames 1 .. T of a walk-through arrive and one prediction is made per prefix.  The reference calls batch_point_sample on views
0 .. t for every t (:165-203) and runs the 3-D branch on the T cumulative clouds as a batch of T (:206-246).  Here the image volumes of
ALL prefixes come out of one pass over the views (es_point_sample_prefix_fwd_pts: a running sum, bit-identical to the T separate
calls) straight into columns [0, C2) of one (T nvox, C2 + 512) buffer whose frame-major rows are the batch-major rows of the dense
neck with B = T; the T cumulative clouds are voxelised as batch entries 0 .. T-1, MinkResNet34's last level is scattered into
columns [C2, C2 + 512), and IndoorImVoxelNeck / ImVoxelOccHead run on the T-fold batch exactly as they do on one sample.
Parameters, gradient buckets and the predict guard are DenseFusionOccPredictor's."""
import torch
from ... import engine as E
from ... import hip
from ... import sparse
from ...hip import P, call
from ...registry import MODELS
from ...sparse import SparseTensor
from ..layers.fusion_layers.point_fusion import build_fusion_meta
from .dense_fusion_occ import DenseFusionOccPredictor


@MODELS.register_module()
class EmbodiedOccPredictor(DenseFusionOccPredictor):
    def open_walk(self, metainfo):
        """a session that takes the walk one frame at a time: walk.observe(img, points, depth2img) -> the pred_occupancy of the prefix
        so far (walk.py).  metainfo: what is constant over the walk -- image shape, augmentation keys, depth2img['origin']"""
        from .walk import OccWalk
        return OccWalk(self, metainfo)

    def extract_feat(self, batch_inputs_dict, batch_data_samples):
        """embodied_occ.py:118-247.  Returns [(Var (T*X_i*Y_i*Z_i, 128), (X_i, Y_i, Z_i))] fine -> coarse, prefix-major rows."""
        self._bind()
        self.start_tape_parts()
        img = batch_inputs_dict['imgs']
        B, V = img.shape[:2]
        H, W = img.shape[-2:]
        T = len(batch_data_samples)
        assert B == 1, 'the image batch of the continuous detector is 1 (embodied_occ.py:189 "batch_size=1")'
        assert T == V, f'one data sample per prefix: {T} samples for {V} views (Det3DDataPreprocessor(batchwise_inputs=True))'
        assert len(batch_inputs_dict['points']) == T, 'one cumulative cloud per prefix (pipeline.make_cont_occ_batch)'
        if img.stride(2) != 1:
            img = img.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
        nhwc = img.permute(0, 1, 3, 4, 2).reshape(V, H, W, 3)
        E.refresh_weight_copies()
        f2d, Hf, Wf = self.neck(self.backbone(nhwc), V, levels=[0])[0]
        E.mark('2-D backbone + FPN')
        self.tape_part(1)                       # behind this point: 3-D backbone, then the neck parts
        meta0 = batch_data_samples[0].metainfo  # the T copies share their meta (data_preprocessor.py:192 of the reference)
        X, Y, Z = self.n_voxels
        nvox = X * Y * Z
        origin = meta0['depth2img'].get('origin') if isinstance(meta0.get('depth2img'), dict) else None
        prior = self.prior_points(origin).to(self.device, non_blocking=True)
        meta_dev = build_fusion_meta([meta0], self.coord_type, (H, W), V).to(self.device, non_blocking=True)
        C2 = f2d.d.shape[1]
        C3 = 512
        vol = torch.zeros((T * nvox, C2 + C3), dtype=torch.float32, device=self.device)
        bidx = torch.zeros((nvox, 4), dtype=torch.int32, device=self.device)           # column 0 = image sample index (0)
        pix = torch.empty((nvox, V), dtype=torch.int32, device=self.device)
        cnt = torch.empty((V, nvox), dtype=torch.int32, device=self.device)
        call('es_point_sample_prefix_fwd_pts', P(bidx), P(prior), nvox, P(meta_dev), meta_dev.shape[1], V, P(f2d.d), Hf, Wf, C2,
             P(vol), C2 + C3, P(pix), P(cnt), hip.stream())
        E.mark('image volumes of every prefix (projection)')
        # sparse branch: the T cumulative clouds are batch entries 0 .. T-1 (embodied_occ.py:206-235)
        pts = [p if (p.dtype == torch.float32 and p.stride(-1) == 1) else p.float().contiguous() for p in batch_inputs_dict['points']]
        rmin = self.point_cloud_range[:3]
        cmax = [n * self.voxel_stride - 1 for n in self.n_voxels]
        cs, src = sparse.voxelize_range(pts, rmin, self.voxel_size, cmax)
        allp = torch.cat([p[:, :3] for p in pts]) if len(pts) > 1 else pts[0][:, :3].contiguous()
        feats = torch.empty((cs.n, 3), dtype=torch.float32, device=self.device)
        call('es_row_move', P(feats), 3, P(allp), allp.stride(0), P(src), cs.n, 3, 0, hip.stream())
        x3 = self.backbone_3d(SparseTensor(cs, E.Var(feats, rg=False)))[-1]
        self.tape_part(2)
        assert x3.F.d.shape[1] == C3 and x3.cs.ts == self.voxel_stride
        didx = torch.empty(x3.cs.n, dtype=torch.int32, device=self.device)
        call('es_dense_index', P(x3.cs.coords), x3.cs.n, x3.cs.ts, X, Y, Z, P(didx), hip.stream())
        call('es_row_move', vol.data_ptr() + 4 * C2, C2 + C3, P(x3.F.d), C3, P(didx), x3.cs.n, C3, 2, hip.stream())
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
                head = torch.empty(f2d.d.shape[0], dtype=torch.int32, device=self.device)
                nxt = torch.empty(nvox * V, dtype=torch.int32, device=self.device)
                call('es_point_sample_prefix_bwd', P(bidx), nvox, V, P(v.g), C2 + C3, P(pix), P(cnt), Hf, Wf, C2, P(f2d.g), V, P(head),
                     P(nxt), acc, hip.stream())
        E.TAPE.add(bwd)
        outs = self.neck_3d(v, (X, Y, Z), T, on_coarse=lambda: self.tape_part(3))
        E.mark('IndoorImVoxelNeck')
        return outs
