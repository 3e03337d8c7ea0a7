"""Walk sessions of the continuous models and of the grounder: frame in, prediction (or answers to prompts) out.

EmbodiedOccPredictor.predict / Embodied3DDetector.predict take the whole walk (T frames, T cumulative clouds) and return T results.
An agent that is walking has frame t only; a session (`detector.open_walk(metainfo)`) holds what frames 0 .. t-1 left behind and
`observe(img, points, depth2img)` returns the prediction of the prefix 0 .. t:

OccWalk   the image volume of prefix t is a running sum over the views, so the state is an (nvox, C) sum and an (nvox) count advanced by
          ONE launch per frame (es_point_sample_step_fwd_pts, bit-identical to row block t of the prefix kernel) -- no feature map of an
          earlier frame, no limit on the walk length -- plus the cloud so far.
DetWalk   the fusion of prefix t gathers every earlier view at the CURRENT voxel set, so the four levels' feature maps of all frames are
          kept (preallocated for `max_frames` <= 64, the view limit of the window kernels) and the existing per-level window fusion runs
          on their first t + 1 views.

GroundWalk (SparseFeatureFusion3DGrounder.open_walk) keeps the maps as DetWalk does, but its observe() does no 3-D work and returns the frame
          count: scene() encodes the prefix so far (all t + 1 views, cached until the next observe) and ask(prompts) grounds on it.

All re-voxelise the cloud so far and run the 3-D branch on it: those are exact, an incremental 3-D backbone is not.  Conventions follow
the grounder's SceneEncoding: a session records engine.PRECISION[0] / engine.WEIGHT_VERSION[0] when it is opened and observe() raises
ValueError once either has moved (the state was computed with other weights) or the device differs.  Every observe runs in eval mode
with the tape off; the detector's `training` flag and engine.TAPE.enabled are restored afterwards and nothing is recorded.

Failure: every refusal (stale weights, device, argument shapes, max_frames) comes before anything is launched and leaves the session as
it was.  DetWalk commits a frame only when its prediction is made, GroundWalk when its observe has succeeded.  OccWalk commits it
with the step launch, which moves the sum in place: an error raised behind that launch (3-D branch, neck, head) leaves the frame
counted with no prediction returned -- reset() the walk then."""
import torch
from ... import engine as E
from ... import hip
from ...hip import P, call
from ...structures import Det3DDataSample
from ..layers.fusion_layers.point_fusion import build_fusion_meta
from .base import predict_guard
from .dense_fusion_occ import C3

MAX_DET_FRAMES = 64          # es_point_sample_win_fwd returns -9 above that


class WalkMeta:
    """Host side of a session: the walk's constant meta (image shape, augmentation keys, the projection entry's `origin`) and the
    per-frame matrices collected so far.  one_view(): the ES_FUSE_* row of ONE frame (what the step kernel reads); metainfo(): the
    meta dict of the prefix so far, from which build_fusion_meta makes the row of all its views (what the window kernels read)."""

    def __init__(self, metainfo, coord_type):
        self.coord_type = coord_type
        self.key = {'LIDAR': 'lidar2img', 'DEPTH': 'depth2img', 'CAMERA': 'cam2img'}[coord_type.upper()]
        self.base = dict(metainfo or {})
        pm = self.base.get(self.key)
        self.const = {k: v for k, v in pm.items() if k not in ('extrinsic', 'intrinsic')} if isinstance(pm, dict) else {}
        self.origin = self.const.get('origin')
        self.extrinsic, self.intrinsic = [], []

    def __len__(self):
        return len(self.extrinsic)

    def clear(self):
        self.extrinsic, self.intrinsic = [], []

    @staticmethod
    def _frame(frame):
        e, i = frame['extrinsic'], frame['intrinsic']
        assert not isinstance(e, (list, tuple)) or len(e) == 4, 'one frame: a 4 x 4 extrinsic, not a list of views'
        return e, i

    def add(self, frame):
        e, i = self._frame(frame)
        self.extrinsic.append(e)
        self.intrinsic.append(i)

    def pop(self):
        self.extrinsic.pop()
        self.intrinsic.pop()

    def one_view(self, frame, hw):
        """(1, 32 + 16) f32 host row: build_fusion_meta(..., n_views=1) on this frame's matrices"""
        e, i = self._frame(frame)
        m = dict(self.base)
        m[self.key] = dict(self.const, extrinsic=[e], intrinsic=[i])
        return build_fusion_meta([m], self.coord_type, hw, 1)

    def metainfo(self):
        m = dict(self.base)
        m[self.key] = dict(self.const, extrinsic=list(self.extrinsic), intrinsic=list(self.intrinsic))
        return m


class _Cloud:
    """the rows of the cloud so far in one device buffer that grows by doubling (a view of its first n rows is the prefix's cloud)"""

    def __init__(self, device):
        self.device, self.buf, self.n = device, None, 0

    def append(self, rows):
        """-> the number of rows after the append; `n` itself moves only when the caller commits (rows copied behind n by a call that
        then fails are simply overwritten by the next one)"""
        rows = rows if rows.dtype == torch.float32 else rows.float()
        k, cols = int(rows.shape[0]), int(rows.shape[1])
        if self.buf is not None and self.buf.shape[1] != cols:
            if self.n:
                raise ValueError(f'points has {cols} columns, the cloud so far {self.buf.shape[1]}')
            self.buf = None                              # an empty cloud (a new or reset walk) takes whatever columns come
        if self.buf is None or self.n + k > self.buf.shape[0]:
            cap = max(2 * (self.n + k), 1 << 16)
            new = torch.empty((cap, cols), dtype=torch.float32, device=self.device)
            if self.n:
                new[:self.n].copy_(self.buf[:self.n])
            self.buf = new
        if k:
            self.buf[self.n:self.n + k].copy_(rows)
        return self.n + k


def _device(d):
    """torch.device with the index filled in ('cuda' -> the current device), so that two spellings of one device compare equal"""
    d = torch.device(d)
    return torch.device(d.type, torch.cuda.current_device()) if d.type == 'cuda' and d.index is None else d


class _Walk:
    def __init__(self, det, metainfo):
        self.det = det
        self.device = _device(det.device)
        self.precision, self.weight_version = E.PRECISION[0], E.WEIGHT_VERSION[0]
        self.meta = WalkMeta(metainfo, det.coord_type)
        self.cloud = _Cloud(self.device)
        self.t = 0                       # frames observed so far
        self._frame = None               # (1, H, W, 3) f32: the image backbone's input, one stable address per session

    def _check_state(self):
        if self.precision != E.PRECISION[0] or self.weight_version != E.WEIGHT_VERSION[0]:
            raise ValueError(f'the walk was opened under precision {self.precision!r} / weight version {self.weight_version}, now '
                             f'{E.PRECISION[0]!r} / {E.WEIGHT_VERSION[0]}: its state is stale, open a new walk')
        if _device(self.det.device) != self.device:
            raise ValueError(f'the walk was opened on {self.device}, the detector now is on {self.det.device}')

    def _check(self, img, points):
        self._check_state()
        for name, t in (('img', img), ('points', points)):
            if _device(t.device) != self.device:
                raise ValueError(f'{name} is on {t.device}, the walk on {self.device}')
        if img.dim() != 3 or img.shape[0] != 3 or img.dtype != torch.float32:
            raise ValueError('img: one preprocessed frame (3, H, W) f32, as inputs["imgs"][0, t] after the data preprocessor')
        if points.dim() != 2 or points.shape[1] < 3:
            raise ValueError('points: the (k, >= 3) rows of the cloud this frame adds')

    def _stage_frame(self, img):
        H, W = int(img.shape[1]), int(img.shape[2])
        if self._frame is None or tuple(self._frame.shape[1:3]) != (H, W):
            self._frame = torch.empty((1, H, W, 3), dtype=torch.float32, device=self.device)
        self._frame[0].copy_(img.permute(1, 2, 0))
        return H, W

    def _frame5(self, H, W):
        """the staged frame as the (1, 1, 3, H, W) block a detector's image branch takes (a view: channels stay innermost)"""
        return self._frame.view(1, 1, H, W, 3).permute(0, 1, 4, 2, 3)

    def _guard(self):
        """eval mode + tape off, both restored on exit"""
        return predict_guard(self.det)

    def state_bytes(self):
        raise NotImplementedError


class OccWalk(_Walk):
    """EmbodiedOccPredictor.open_walk(metainfo).  observe() -> (X, Y, Z) int64 pred_occupancy of the prefix so far; `logits` is the
    finest level's head output of the last observe."""

    def __init__(self, det, metainfo):
        super().__init__(det, metainfo)
        self.sum = self.nvalid = self.pix = None
        self.logits = None
        X, Y, Z = det.n_voxels
        self.nvox = X * Y * Z
        self.prior = det.prior_points(self.meta.origin).to(self.device)
        self.bidx = torch.zeros((self.nvox, 4), dtype=torch.int32, device=self.device)         # column 0 = image sample index (0)

    def reset(self):
        """back to the state of open_walk: the next observe is frame 0 (weights / precision are still those of the opening)"""
        if self.sum is not None:
            self.sum.zero_()
            self.nvalid.zero_()
        self.meta.clear()
        self.cloud.n = 0
        self.t = 0
        self.logits = None

    def state_bytes(self):
        own = [self.sum, self.nvalid, self.cloud.buf]
        return sum(t.numel() * t.element_size() for t in own if t is not None)

    def observe(self, img, points, depth2img):
        self._check(img, points)
        det, dev = self.det, self.device
        with self._guard():
            hip.refresh_stream()
            det._bind()
            H, W = self._stage_frame(img)
            f2d, Hf, Wf = det.image_maps(self._frame5(H, W))
            meta_dev = self.meta.one_view(depth2img, (H, W)).to(dev, non_blocking=True)
            assert f2d.d.dtype == torch.float32, 'the step kernel reads f32 feature maps (the FPN emits f32)'
            C2 = int(f2d.d.shape[1])
            nvox = self.nvox
            if self.sum is None or self.sum.shape[1] != C2:
                assert self.t == 0, 'the width of the image volume changed during the walk'
                self.sum = torch.zeros((nvox, C2), dtype=torch.float32, device=dev)
                self.nvalid = torch.zeros(nvox, dtype=torch.int32, device=dev)
                self.pix = torch.empty(nvox, dtype=torch.int32, device=dev)
            n = self.cloud.append(points)                # (before the state moves: a refused cloud leaves the walk where it was)
            vol = torch.zeros((nvox, C2 + C3), dtype=torch.float32, device=dev)
            call('es_point_sample_step_fwd_pts', P(self.bidx), P(self.prior), nvox, P(meta_dev), meta_dev.shape[1], P(f2d.d), Hf, Wf, C2,
                 P(self.sum), P(self.nvalid), P(vol), C2 + C3, P(self.pix), hip.stream())
            self.meta.add(depth2img)
            self.cloud.n = n
            self.t += 1
            cloud = self.cloud.buf[:n]                   # the cloud so far, its xyz read in place: no packed copy
            det.point_branch([cloud], vol, C2, rows=cloud)
            outs = det.neck_3d(E.Var(vol), tuple(det.n_voxels), 1)
            logits, dims = det.bbox_head.forward(outs[:1])[0]
            self.logits = logits.d
            return det.bbox_head.argmax(logits, dims)[0]


class _MapWalk(_Walk):
    """a session that keeps the four levels' feature maps of every observed frame on the device: per level one (max_frames Hf Wf, C)
    buffer in the dtype the backbone emits (allocated at the first observe, when the map sizes are known)"""

    def __init__(self, det, metainfo, max_frames=50):
        max_frames = int(max_frames)
        if not 1 <= max_frames <= MAX_DET_FRAMES:
            raise ValueError(f'max_frames = {max_frames}: the view-window kernels take 1 .. {MAX_DET_FRAMES} views')
        super().__init__(det, metainfo)
        self.max_frames = max_frames
        self.maps = None                 # [(buffer (max_frames Hf Wf, C), Hf, Wf)] per level

    def reset(self):
        self.meta.clear()
        self.cloud.n = 0
        self.t = 0

    def state_bytes(self):
        own = [self.cloud.buf] + [m for m, _, _ in (self.maps or [])]
        return sum(t.numel() * t.element_size() for t in own if t is not None)

    def _refuse_full(self):
        if self.t >= self.max_frames:
            raise ValueError(f'the walk was opened for max_frames = {self.max_frames} frames and has seen them all')

    def _intake(self, img, join=False):
        """the frame through the image branch, its four maps into row block t of the kept ones -> (hw, forked) as _image_feats gives
        them.  Forked: the copies ride behind the image backbone on its stream; join=True makes whatever the caller queues next see
        the maps, join=False leaves that to the caller (_fuse_points joins).  Commits nothing: `t` does not move."""
        H, W = self._stage_frame(img)
        img_feats, _, hw, forked = self.det._image_feats(self._frame5(H, W))
        self._alloc_maps(img_feats)                      # (on the main stream: the buffers outlive every side-stream segment)
        if forked:
            with E.side_stream(fork=False):
                self._keep_maps(img_feats)
            if join:
                E.join_side()
        else:
            self._keep_maps(img_feats)
        return hw, forked

    def _alloc_maps(self, img_feats):
        if self.maps is None or any(m.dtype != f.d.dtype or m.shape[1] != f.d.shape[1] or (h, w) != (Hf, Wf)
                                    for (m, h, w), (f, Hf, Wf) in zip(self.maps, img_feats)):
            assert self.t == 0, 'the feature maps changed their shape or dtype during the walk'
            self.maps = [(torch.empty((self.max_frames * Hf * Wf, int(f.d.shape[1])), dtype=f.d.dtype, device=self.device), Hf, Wf)
                         for f, Hf, Wf in img_feats]

    def _keep_maps(self, img_feats):
        t = self.t
        for (m, Hf, Wf), (f, _, _) in zip(self.maps, img_feats):
            m[t * Hf * Wf:(t + 1) * Hf * Wf].copy_(f.d)

    def _views(self, k):
        """the maps of the first k frames, as the fusion takes them"""
        return [(E.Var(m[:k * Hf * Wf], rg=False), Hf, Wf) for m, Hf, Wf in self.maps]


class DetWalk(_MapWalk):
    """Embodied3DDetector.open_walk(metainfo, max_frames).  observe() -> InstanceData(bboxes_3d, scores_3d, labels_3d) of the prefix so
    far.  The feature maps of every observed frame stay on the device (_MapWalk)."""

    def observe(self, img, points, depth2img):
        self._check(img, points)
        self._refuse_full()
        det = self.det
        t = self.t
        with self._guard():
            hip.refresh_stream()
            det._bind()
            self.meta.add(depth2img)
            try:
                hw, forked = self._intake(img)
                n = self.cloud.append(points)
                views = self._views(t + 1)
                sample = Det3DDataSample(self.meta.metainfo())
                det._win_t0 = t                          # the one batch entry of the launch is prefix t: window = views 0 .. t
                x = det._fuse_points({'points': [self.cloud.buf[:n]]}, [sample], (views, t + 1, hw, forked))
                res = det.bbox_head.predict(x, [sample])[0]
            except BaseException:
                self.meta.pop()
                raise
            finally:
                det._win_t0 = 0
            self.cloud.n = n
            self.t = t + 1
            return res


class GroundWalk(_MapWalk):
    """SparseFeatureFusion3DGrounder.open_walk(metainfo, max_frames): ask a recording in words while it is being walked.

    observe() runs the 2-D backbone on the one frame, keeps its four maps and appends the frame's rows to the cloud -- no 3-D work -- and
    returns the number of frames seen.  scene() is the SceneEncoding of the prefix so far: the fusion of the cloud so far with views
    0 .. t (all V = t + 1 of them, the base _fuse_level), MinkNeck and scene_from_tokens; it is cached until the next observe, so
    any number of ask() calls between two frames pay for the 3-D branch once.  ask(prompts) = det.ground(scene(), prompts); with any of
    iou_thr / score_thr / topk the result goes through inference.select_answers.

    Failure: as on the siblings every refusal comes before anything is launched and leaves the session as it was; a frame is committed
    only when its observe has succeeded (the map rows and cloud rows an interrupted observe wrote lie behind the committed ones and
    are overwritten by the next)."""

    def __init__(self, det, metainfo, max_frames=50):
        super().__init__(det, metainfo, max_frames)
        self._scene = None               # SceneEncoding of the prefix 0 .. t-1, None: not built since the last observe
        self._hw = None

    def reset(self):
        super().reset()
        self._scene = None

    def observe(self, img, points, depth2img):
        self._check(img, points)
        self._refuse_full()
        WalkMeta._frame(depth2img)
        det = self.det
        n = self.cloud.append(points)                    # (a cloud with other columns is refused here, before the backbone runs)
        with self._guard():
            hip.refresh_stream()
            det._bind()
            hw, _ = self._intake(img, join=True)
        self.meta.add(depth2img)
        self.cloud.n = n
        self._hw = hw
        self._scene = None
        self.t += 1
        return self.t

    def scene(self):
        """the SceneEncoding of the frames observed so far (the same object until the next observe)"""
        self._check_state()
        if self.t == 0:
            raise ValueError('the walk has not observed a frame yet: nothing to encode')
        if self._scene is not None:
            return self._scene
        det, t = self.det, self.t
        with self._guard():
            hip.refresh_stream()
            det._bind()
            sample = Det3DDataSample(self.meta.metainfo())
            det.start_tape_parts()                       # (what _image_feats leaves behind for _fuse_points; nothing is recorded here)
            det._branch_ends = [len(E.TAPE.fns), None]
            x = det._fuse_points({'points': [self.cloud.buf[:self.cloud.n]]}, [sample], (self._views(t), t, self._hw, False))
            det.neck_3d(x, 1)
            nk = det.neck_3d.last
            L = nk['lens'][0]
            feats, points = nk['feats'].d[:L].clone(), nk['points'][:L].clone()
        self._scene = det.scene_from_tokens(feats, points)
        return self._scene

    def ask(self, prompts, tokens_positive=None, **select):
        """InstanceData per prompt for the prefix so far: what det.ground returns (Q rows each), or -- with iou_thr / score_thr / topk --
        the answers inference.select_answers makes of it"""
        res = self.det.ground(self.scene(), prompts, tokens_positive)
        if select:
            from ...inference import select_answers
            res = select_answers(res, **select)
        return res
