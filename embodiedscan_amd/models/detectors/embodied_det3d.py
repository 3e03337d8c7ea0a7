"""Embodied3DDetector (embodiedscan/models/detectors/embodied_det3d.py:27-300) on the MI355X kernels: continuous 3-D detection.

Frames 1 .. T of a walk-through arrive and one set of detections is made per prefix.  The reference runs the 2-D backbone once on the
V = T frames (:113-128), voxelises the T cumulative clouds as batch entries 0 .. T-1 (:132-142) and fuses entry t with the image
features of views 0 .. t only (:147-191: `img_features[level][0][:idx + 1]`, `proj_mat[:idx + 1]`); head, target assignment and NMS
then run per sample as they do for mv-3ddet.  Here that is SparseFeatureFusionSingleStage3DDetector with ONE thing changed: the
per-level fusion launches the view-window kernels (es_point_sample_win_fwd / _bwd) with the table win[t] = (image set 0, t + 1
views) instead of giving every sample all V views -- 4 forward and 12 backward launches per step whatever T is.  Parameters,
state-dict names, gradient buckets, prefetch, loss / forward / train_step are the parent's.

predict: a test walk-through has 50 frames, and the 50 cumulative clouds as one batch are 6.4 M points.  `predict_chunk` (an
attribute, not a config key: the reference configuration builds unchanged) is the number of prefixes whose 3-D branch and head run
together; the 2-D features are computed once.  In eval mode every norm is per sample or folded, so the chunk size does not change
the result."""
import torch
from ... import hip
from ...hip import P, call
from ...registry import MODELS
from .sparse_featfusion_single_stage import SparseFeatureFusionSingleStage3DDetector


@MODELS.register_module()
class Embodied3DDetector(SparseFeatureFusionSingleStage3DDetector):
    continuous = True

    predict_chunk = 8

    def open_walk(self, metainfo, max_frames=50):
        """a session that takes the walk one frame at a time: walk.observe(img, points, depth2img) -> the detections of the prefix so
        far (walk.py).  The feature maps of up to max_frames <= 64 frames stay on the device; ValueError above that"""
        from .walk import DetWalk
        return DetWalk(self, metainfo, max_frames)

    def _check(self, batch_inputs_dict, batch_data_samples):
        B, V = batch_inputs_dict['imgs'].shape[:2]
        T = len(batch_data_samples)
        assert B == 1, 'the image batch of the continuous detector is 1 (embodied_det3d.py:109 "only support batch_size=1")'
        assert T == V, f'one data sample per prefix: {T} samples for {V} views (Det3DDataPreprocessor(batchwise_inputs=True))'
        assert len(batch_inputs_dict['points']) == T, 'one cumulative cloud per prefix (pipeline.make_cont_det_batch)'
        return T

    def _window(self, t0, k):
        """(k, 2) int32 device table: batch entry j of the launch is prefix t0 + j -> image set 0, its first t0 + j + 1 views"""
        cache = self.__dict__.setdefault('_win_cache', {})
        key = (t0, k, str(self.device))
        if key not in cache:
            if len(cache) > 64:
                cache.clear()
            cache[key] = torch.tensor([[0, t0 + j + 1] for j in range(k)], dtype=torch.int32).to(self.device)
        return cache[key]

    def extract_feat(self, batch_inputs_dict, batch_data_samples):
        """embodied_det3d.py:90-207.  Returns 4 SparseTensors (batch entry t = prefix t) with [3-D | image] channels."""
        self._check(batch_inputs_dict, batch_data_samples)
        self._win_t0 = 0
        return super().extract_feat(batch_inputs_dict, batch_data_samples)

    def _fuse_level(self, cs, meta_dev, V, f2d, Hf, Wf, cat, C3):
        C = f2d.d.shape[1]
        n = cs.n
        win = self._window(self._win_t0, meta_dev.shape[0])
        assert int(f2d.d.shape[0]) == V * Hf * Wf, 'one image set: the V frames of the walk-through'
        pix = torch.empty((n, V), dtype=torch.int32, device=cat.device)       # (the kernel writes every entry: -1 beyond the window)
        cnt = torch.empty(n, dtype=torch.int32, device=cat.device)
        call('es_point_sample_win_fwd_h' if f2d.d.dtype == torch.bfloat16 else 'es_point_sample_win_fwd', P(cs.coords), n,
             float(self.voxel_size), P(meta_dev), meta_dev.shape[1], V, P(win), P(f2d.d), Hf, Wf, C, cat.data_ptr() + 4 * C3, cat.stride(0),
             P(pix), P(cnt), hip.stream())
        return pix, cnt, win

    def _fuse_level_bwd(self, cs, V, dout, C3, saved, f2d, Hf, Wf):
        if not f2d.rg:
            return
        pix, cnt, win = saved
        C = f2d.d.shape[1]
        acc = 1
        if f2d.g is None:
            f2d.g, acc = torch.empty(f2d.d.shape, dtype=torch.float32, device=f2d.d.device), 0   # the gather writes every pixel
        n_pix = f2d.d.shape[0]
        head = torch.empty(n_pix, dtype=torch.int32, device=f2d.d.device)
        nxt = torch.empty(max(cs.n * V, 1), dtype=torch.int32, device=f2d.d.device)
        call('es_point_sample_win_bwd', P(cs.coords), cs.n, V, P(win), dout.data_ptr() + 4 * C3, dout.stride(0), P(pix), P(cnt), Hf, Wf, C,
             P(f2d.g), n_pix // (Hf * Wf), P(head), P(nxt), acc, hip.stream())

    def predict(self, batch_inputs_dict, batch_data_samples, **kwargs):
        """embodied_det3d.py:231-266: `pred_instances_3d` on each of the T samples.  The 3-D branch and the head run over groups of
        `predict_chunk` prefixes; the image backbone runs once."""
        T = self._check(batch_inputs_dict, batch_data_samples)
        chunk = max(1, int(self.predict_chunk))
        results = []
        with self._predict_guard():
            try:
                self._bind()
                img_feats, V, hw, forked = self._image_feats(batch_inputs_dict['imgs'])
                points = batch_inputs_dict['points']
                for t0 in range(0, T, chunk):
                    t1 = min(T, t0 + chunk)
                    self._win_t0 = t0
                    x = self._fuse_points({'points': points[t0:t1]}, batch_data_samples[t0:t1], (img_feats, V, hw, forked and t0 == 0))
                    results += self.bbox_head.predict(x, batch_data_samples[t0:t1], **kwargs)
            finally:
                self._win_t0 = 0
        for ds, r in zip(batch_data_samples, results):
            ds.pred_instances_3d = r
        return batch_data_samples
