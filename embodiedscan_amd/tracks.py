"""Object tracks over a walk: stable identities for the scene inventory (the definition is include/es_hip.h's, at
es_track_assign; the reference has no tracker).

A walk session answers after every frame with a fresh object list.  A TrackTable connects the lists: every detection of a frame either
continues a track -- the greedy one-to-one matching on the exact 9-DoF IoU -- or is born as a new one, and a track nobody has matched
for more than max_age frames dies.  A slot of the table is an identity: it is never reused, a dead track keeps its row.

    table = TrackTable(device)
    for t, frame in ...:
        inst = filter_instances(walk.observe(*frame))
        ids = table.update(inst)                  # (n,) int64 on the device: the track of every row (-1: the table was full)
    table.inventory(min_hits=2)                   # every object seen at least twice, with its id

update is two launches -- es_box3d_iou into a cached workspace (all CUs), then es_track_assign (one workgroup: matching in rounds of
mutual-best pairs, births by a prefix sum, ageing) -- and NO host synchronisation: the host only keeps an upper bound on the number of
tracks (it grows by n per update), the kernel reads the true count on the device and ignores the columns above it.  inventory is the
one read-back; it also makes the host's bound exact again."""
import torch

from . import hip
from .structures import EulerDepthInstance3DBoxes, InstanceData

MAX_DETECTIONS, MAX_CAPACITY = 2048, 4096          # limits of es_track_assign
LABEL, FIRST_SEEN, LAST_SEEN, HITS, ALIVE = range(5)


class TrackTable:
    """capacity: slots (1 .. 4096; a birth beyond it is dropped and counted); iou_thr: a detection continues a track only when their
    IoU exceeds it; same_class: ... and only when its label equals the track's; max_age: a track unmatched for more than max_age frames
    dies (None: never).  ValueError: capacity out of range, iou_thr negative or NaN."""

    def __init__(self, device, capacity=1024, iou_thr=0.25, same_class=False, max_age=None):
        capacity = int(capacity)
        if not 1 <= capacity <= MAX_CAPACITY:
            raise ValueError(f'TrackTable: capacity = {capacity}, the table covers 1 .. {MAX_CAPACITY} slots')
        if not float(iou_thr) >= 0.0:
            raise ValueError(f'TrackTable: iou_thr = {iou_thr}')
        self.capacity, self.iou_thr, self.same_class = capacity, float(iou_thr), bool(same_class)
        self.max_age = -1 if max_age is None else int(max_age)
        self.device = torch.empty(0, device=device).device
        self.boxes = torch.zeros((capacity, 9), dtype=torch.float32, device=self.device)
        self.f = torch.zeros((capacity, 2), dtype=torch.float32, device=self.device)            # score, label_score
        self.i = torch.zeros((capacity, 5), dtype=torch.int32, device=self.device)              # label, first_seen, last_seen, hits, alive
        self.counts = torch.zeros(2, dtype=torch.int32, device=self.device)                     # n_tracks, dropped
        self._iou = None                                                                        # workspace of es_box3d_iou, grows
        self._bound, self.t = 0, None                                                           # host: n_tracks <= _bound; the last t

    def reset(self):
        for buf in (self.boxes, self.f, self.i, self.counts):
            buf.zero_()
        self._bound, self.t = 0, None

    def state_bytes(self):
        """device bytes the table holds: its rows, the counters and the IoU workspace"""
        bufs = [self.boxes, self.f, self.i, self.counts] + ([self._iou] if self._iou is not None else [])
        return sum(b.numel() * b.element_size() for b in bufs)

    def update(self, instances, t=None):
        """the object list of frame t (InstanceData with bboxes_3d, scores_3d, labels_3d) -> (n,) int64 ids on the device, -1 for a
        detection that found the table full.  t: default the previous t + 1 (0 at the start); it must increase.  ValueError before any
        launch: t not above the previous one, inputs on another device or of the wrong shape, more than 2048 rows."""
        boxes = getattr(instances.bboxes_3d, 'tensor', instances.bboxes_3d)
        scores, labels = instances.scores_3d, instances.labels_3d
        for name, x in (('boxes', boxes), ('scores', scores), ('labels', labels)):
            if x.device != self.device:
                raise ValueError(f'TrackTable.update: {name} on {x.device}, the table lives on {self.device}')
        n = int(boxes.shape[0])
        if boxes.dim() != 2 or boxes.shape[1] != 9 or tuple(scores.shape) != (n,) or tuple(labels.shape) != (n,):
            raise ValueError(f'TrackTable.update: boxes (n, 9), scores (n), labels (n); got {tuple(boxes.shape)}, {tuple(scores.shape)}, '
                             f'{tuple(labels.shape)}')
        if n > MAX_DETECTIONS:
            raise ValueError(f'TrackTable.update: {n} detections, one update covers {MAX_DETECTIONS} (filter the list first)')
        t = (0 if self.t is None else self.t + 1) if t is None else int(t)
        if self.t is not None and t <= self.t:
            raise ValueError(f'TrackTable.update: t = {t} after t = {self.t}: the frame index must increase')
        P, st, m = hip.P, hip.stream(), self._bound
        b, s, l = boxes.float().contiguous(), scores.float().contiguous(), labels.to(torch.int32).contiguous()
        if n * m and (self._iou is None or self._iou.numel() < n * m):
            self._iou = torch.empty(max(n * m, 2 * (0 if self._iou is None else self._iou.numel())), dtype=torch.float32, device=self.device)
        ids = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
        if n * m:
            hip.call('es_box3d_iou', P(b), n, P(self.boxes), m, P(self._iou), st)
        hip.call('es_track_assign', P(self._iou), n, m, m, P(b), P(s), P(l), P(self.boxes), P(self.f), P(self.i), P(self.counts),
                 self.capacity, t, self.iou_thr, int(self.same_class), self.max_age, P(ids), st)
        self._bound, self.t = min(self.capacity, m + n), t
        return ids[:n].long()

    def lookup(self, ids):
        """(n,) ids from update -> (hits, first_seen), (n,) int64 each on the device (0 and -1 for an id of -1); no synchronisation"""
        ok = ids >= 0
        rows = self.i[ids.clamp(min=0)].long()
        return torch.where(ok, rows[:, HITS], torch.zeros_like(ids)), torch.where(ok, rows[:, FIRST_SEEN], torch.full_like(ids, -1))

    def inventory(self, min_hits=1, alive_only=True):
        """-> InstanceData(bboxes_3d, scores_3d, labels_3d, track_ids, hits, first_seen, last_seen): the tracks with at least min_hits
        matched frames (alive_only: that have not died), by ascending id; labels_3d = the label of the track's highest-scoring
        detection so far, scores_3d = its latest score.  The one read-back: the integer columns and the counters come to the host in one
        copy, the rows are selected there and gathered on the device."""
        host = torch.cat([self.counts, self.i.reshape(-1)]).cpu()
        nt = int(host[0])
        self._bound = nt
        rows = host[2:].reshape(-1, 5)[:nt]
        keep = rows[:, HITS] >= int(min_hits)
        if alive_only:
            keep &= rows[:, ALIVE] != 0
        ids = torch.nonzero(keep).reshape(-1).to(self.device)
        sel = self.i[ids].long()
        return InstanceData(bboxes_3d=EulerDepthInstance3DBoxes(self.boxes[ids]), scores_3d=self.f[ids, 0], labels_3d=sel[:, LABEL], track_ids=ids,
                            hits=sel[:, HITS], first_seen=sel[:, FIRST_SEEN], last_seen=sel[:, LAST_SEEN])

    @property
    def dropped(self):
        """detections that found the table full so far (a read-back)"""
        return int(self.counts[1])
