"""EmbodiedOccPredictor (embodiedscan/models/detectors/embodied_occ.py:25-345) on the MI355X kernels: continuous occupancy.

Frames 1 .. T of a walk-through arrive and one prediction is made per prefix.  The reference calls batch_point_sample on views
0 .. t for every t (:165-203) and runs the 3-D branch on the T cumulative clouds as a batch of T (:206-246).  Here the image volumes of
ALL prefixes come out of one pass over the views (es_point_sample_prefix_fwd_pts: a running sum, bit-identical to the T separate
calls) straight into columns [0, C2) of one (T nvox, C2 + 512) buffer whose frame-major rows are the batch-major rows of the dense
neck with B = T; the T cumulative clouds are voxelised as batch entries 0 .. T-1, MinkResNet34's last level is scattered into
columns [C2, C2 + 512), and IndoorImVoxelNeck / ImVoxelOccHead run on the T-fold batch exactly as they do on one sample.
Parameters, gradient buckets, the predict guard and extract_feat are DenseFusionOccPredictor's: this class states what a batch of
prefixes must look like (_batch_rule) and how the image volumes are projected (_project)."""
import torch
from ... import engine as E
from ... import hip
from ...hip import P, call
from ...registry import MODELS
from .dense_fusion_occ import DenseFusionOccPredictor


@MODELS.register_module()
class EmbodiedOccPredictor(DenseFusionOccPredictor):
    continuous = True

    def open_walk(self, metainfo):
        """a session that takes the walk one frame at a time: walk.observe(img, points, depth2img) -> the pred_occupancy of the prefix
        so far (walk.py).  metainfo: what is constant over the walk -- image shape, augmentation keys, depth2img['origin']"""
        from .walk import OccWalk
        return OccWalk(self, metainfo)

    def _batch_rule(self, B, V, points, batch_data_samples):
        T = len(batch_data_samples)
        assert B == 1, 'the image batch of the continuous detector is 1 (embodied_occ.py:189 "batch_size=1")'
        assert T == V, f'one data sample per prefix: {T} samples for {V} views (Det3DDataPreprocessor(batchwise_inputs=True))'
        assert len(points) == T, 'one cumulative cloud per prefix (pipeline.make_cont_occ_batch)'
        return T, [batch_data_samples[0].metainfo]      # the T copies share their meta (data_preprocessor.py:192 of the reference)

    def _project(self, f2d, Hf, Wf, prior, meta_dev, V, vol):
        """the image volumes of ALL prefixes in one pass over the views: row block t of `vol` = the running mean over views 0 .. t
        (embodied_occ.py:165-203 calls batch_point_sample once per t); bwd(g, acc) as in the base class"""
        nvox, C2, ld = prior.shape[0], f2d.d.shape[1], vol.shape[1]
        bidx = torch.zeros((nvox, 4), dtype=torch.int32, device=self.device)            # column 0 = image sample index (0)
        pix = torch.empty((nvox, V), dtype=torch.int32, device=self.device)
        cnt = torch.empty((V, nvox), dtype=torch.int32, device=self.device)
        call('es_point_sample_prefix_fwd_pts', P(bidx), P(prior), nvox, P(meta_dev), meta_dev.shape[1], V, P(f2d.d), Hf, Wf, C2,
             P(vol), ld, P(pix), P(cnt), hip.stream())
        E.mark('image volumes of every prefix (projection)')

        def bwd(g, acc):
            head = torch.empty(f2d.d.shape[0], dtype=torch.int32, device=self.device)
            nxt = torch.empty(nvox * V, dtype=torch.int32, device=self.device)
            call('es_point_sample_prefix_bwd', P(bidx), nvox, V, P(g), ld, P(pix), P(cnt), Hf, Wf, C2, P(f2d.g), V, P(head), P(nxt),
                 acc, hip.stream())
        return bwd
