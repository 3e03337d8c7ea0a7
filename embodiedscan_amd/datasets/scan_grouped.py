"""Scan-grouped view of the visual-grounding dataset: items are (scan, P prompts) instead of (scan, prompt), so that a loader decodes a
scan's frames once per P prompts and SparseFeatureFusion3DGrounder.train_step_shared encodes the scan once for all of them.

Grouping rule.  Scans in order of first appearance in the dataset's `data_list`; each scan's prompts in a seeded per-epoch order
(`set_epoch`), cut into chunks of P; a last chunk that is short is filled with prompts of the same scan from the start of that order (a
scan with fewer than P prompts repeats its own: DefaultSampler's round-up, applied per scan).  So every prompt of the dataset appears at
least once per epoch, no item mixes scans and P is constant.

The view exposes what datasets.ScanLoader uses of a dataset (`__len__`, `pipeline`, `load_scan(idx, rng, alloc)`, `get_data_info`); the
raw scan it returns is the one the grounding reader returns for the item's first prompt plus `prompts`: per prompt the text, the positive
spans, the target boxes (through the SAME augmentation draw as the scan's points), labels and the three eval flags."""
import numpy as np

_FLAGS = ('is_view_dep', 'is_hard', 'is_unique')


class ScanGroupedGrounding:
    def __init__(self, dataset, prompts_per_scan, seed=0):
        if int(prompts_per_scan) < 1:
            raise ValueError('prompts_per_scan must be positive')
        self.dataset, self.prompts_per_scan, self.seed, self.epoch = dataset, int(prompts_per_scan), int(seed), 0
        self.pipeline = dataset.pipeline
        self.metainfo = getattr(dataset, 'metainfo', None)
        groups = {}
        for i, info in enumerate(dataset.data_list):
            groups.setdefault(info['scan_id'], []).append(i)
        self.scan_ids = list(groups)                       # (dicts keep insertion order: first appearance)
        self.groups = [groups[k] for k in self.scan_ids]
        self._build()

    def set_epoch(self, epoch):
        self.epoch = int(epoch)
        self._build()

    def prompt_order(self, g):
        """the indices (into dataset.data_list) of scan g's prompts in this epoch's order"""
        idxs = self.groups[g]
        rng = np.random.RandomState([self.seed & 0xffffffff, self.epoch & 0xffffffff, g])
        return [idxs[j] for j in rng.permutation(len(idxs))]

    def _build(self):
        P = self.prompts_per_scan
        items = []
        for g in range(len(self.groups)):
            order = self.prompt_order(g)
            for c in range(0, len(order), P):
                chunk = order[c:c + P]
                j = 0
                while len(chunk) < P:
                    chunk.append(order[j % len(order)])
                    j += 1
                items.append(chunk)
        self.items = items

    def __len__(self):
        return len(self.items)

    def get_data_info(self, idx):
        return self.dataset.get_data_info(self.items[idx][0])

    def load_scan(self, idx, rng=None, alloc=None):
        from ..pipeline import augment_gt_boxes
        chunk = self.items[idx]
        scan = self.dataset.load_scan(chunk[0], rng, alloc)          # frames decoded once for the P prompts
        prompts = []
        for i in chunk:
            info = self.dataset.data_list[i]
            ann = info.get('ann_info') or info.get('eval_ann_info') or {}
            boxes = np.asarray(ann.get('gt_bboxes_3d', np.zeros((0, 9), np.float32)), np.float32)
            rec = dict(text=info['text'], tokens_positive=info.get('tokens_positive'),
                       gt_boxes=augment_gt_boxes(boxes, scan['aug']).numpy(),
                       gt_labels=np.asarray(ann.get('gt_labels_3d', np.zeros((0,), np.int64)), np.int64))
            for k in _FLAGS:
                rec[k] = ann.get(k)
            prompts.append(rec)
        scan['prompts'] = prompts
        return scan
