"""GroundWalk (SparseFeatureFusion3DGrounder.open_walk: frame in, questions answered on the prefix so far) on the MI355X against the
batch path -- encode_scene + ground on views 0 .. t and the cloud prefix t -- on tests/test_gpu_grounding._small_grounder and a 4-frame
synthetic scan (test_gpu_cont_det._sweep_scan(44, 4): 128 x 128 images, 8000 points in frame order).

Per prefix t the token count is equal, and the tokens / answers differ from the batch path for the one reason of
test_gpu_shared_scene.test_encode_scene_and_ground_vs_predict_on_replicated_samples -- the image backbone ran on one frame at a time on
one side and on t + 1 frames at once on the other -- and are held to its bounds: tokens relative L2 < 1e-5; ask against ground on the
batch encoding, teacher-forced to the same query indices, boxes < 1e-4 and scores < 1e-3.  Prefixes differ from each other, scene() is
cached (the same object, no launch in between), reset() + the same walk is bit-equal, every refusal of the protocol leaves the frame
count, the cloud length and the cached scene as they were.  The batch references are computed once per module."""
import pytest
import torch

import test_gpu_cont_det as CD
import test_gpu_grounding as TG

pytestmark = pytest.mark.gpu

PROMPTS = ['the chair next to the window', 'find the table that is closer to the door', 'the lamp']
T_FRAMES = 4


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def make_case(dev):
    """the grounder, the walk's inputs and per prefix the batch path's encoding and free answers (computed once, left unchanged)"""
    from embodiedscan_amd import engine as E, pipeline
    from embodiedscan_amd.structures import Det3DDataSample
    cfg, det, sd = TG._small_grounder(dev)
    E.TAPE.clear()
    dscan = pipeline.upload_scan(CD._sweep_scan(44, T_FRAMES), dev)
    batch = pipeline.make_batch([dscan])
    cloud = batch['inputs']['points'][0]
    data = det.data_preprocessor(batch, False)
    imgs = data['inputs']['imgs'].clone()                  # (the preprocessor's buffers are a ring)
    full = dict(data['data_samples'][0].metainfo)
    d2i = full['depth2img']
    meta = dict(full, depth2img={k: v for k, v in d2i.items() if k not in ('extrinsic', 'intrinsic')})
    frames = [(t, cloud[r0:r1], dict(extrinsic=e, intrinsic=i), r1) for t, (r0, r1), e, i in pipeline.walk_frames(dscan, cloud.shape[0])]
    assert len(frames) == T_FRAMES and frames[-1][3] == cloud.shape[0]
    ref = []
    for t, _, _, r1 in frames:
        m = dict(full, depth2img=dict(d2i, extrinsic=list(d2i['extrinsic'][:t + 1]), intrinsic=list(d2i['intrinsic'][:t + 1])))
        scene = det.encode_scene({'imgs': imgs[:, :t + 1].contiguous(), 'points': [cloud[:r1]]}, [Det3DDataSample(m)])[0]
        res = det.ground(scene, PROMPTS)
        ref.append(dict(scene=scene, forced=det.last_queries['idx'].clone(),
                        res=[(r.bboxes_3d.tensor.clone(), r.scores_3d.clone()) for r in res]))
    torch.cuda.synchronize()
    return dict(det=det, imgs=imgs, frames=frames, meta=meta, ref=ref)


@pytest.fixture(scope='module')
def case(dev):
    return make_case(dev)


class _Launches:
    """counts the kernel launches made through the binding layer while it is installed"""

    def __init__(self, monkeypatch):
        from embodiedscan_amd import hip
        self.n = 0
        orig = hip._launch

        def counted(name, args):
            self.n += 1
            return orig(name, args)
        monkeypatch.setattr(hip, '_launch', counted)


def _walk_pass(walk, c, ask=True):
    """-> per prefix (feats, points, [(boxes, scores)] of the free ask)"""
    out = []
    for t, rows, d2i, _ in c['frames']:
        assert walk.observe(c['imgs'][0, t], rows, d2i) == t + 1
        s = walk.scene()
        res = walk.ask(PROMPTS) if ask else []
        out.append((s.feats.clone(), s.points.clone(), [(r.bboxes_3d.tensor.clone(), r.scores_3d.clone()) for r in res]))
    torch.cuda.synchronize()
    return out


def walk_equals_batch(c, monkeypatch):
    from embodiedscan_amd import inference
    det = c['det']
    walk = det.open_walk(c['meta'], max_frames=T_FRAMES)
    with pytest.raises(ValueError, match='not observed'):
        walk.ask(PROMPTS)
    assert walk.t == 0 and walk.cloud.n == 0 and walk._scene is None
    feats = []
    for t, rows, d2i, r1 in c['frames']:
        assert walk.observe(c['imgs'][0, t], rows, d2i) == t + 1
        assert walk.t == t + 1 and walk.cloud.n == r1 and len(walk.meta) == t + 1 and walk._scene is None
        s = walk.scene()
        with monkeypatch.context() as mp:
            n = _Launches(mp)
            again = walk.scene()
            assert again is s and n.n == 0, f'scene() twice: another object or {n.n} launches'
        r = c['ref'][t]
        assert s.L == r['scene'].L, f'prefix {t}: {s.L} tokens, the batch path has {r["scene"].L}'
        assert torch.equal(s.points, r['scene'].points)
        ef = TG._rel(s.feats, r['scene'].feats)
        print(f'prefix {t}: {s.L} tokens, rel-L2 against encode_scene on views 0 .. {t}: {ef:.2e} (tol 1e-5)')
        assert ef < 1e-5
        feats.append(s.feats.clone())
        det.force_queries = r['forced']
        try:
            res = walk.ask(PROMPTS)
        finally:
            det.force_queries = None
        assert walk.scene() is s, 'ask() rebuilt the scene'
        for p, (g, (wb, ws)) in enumerate(zip(res, r['res'])):
            eb, es = TG._rel(g.bboxes_3d.tensor, wb), float((g.scores_3d - ws).abs().max())
            print(f'  prompt {p}: boxes rel-L2 {eb:.2e} (tol 1e-4), scores max |err| {es:.2e} (tol 1e-3)')
            assert eb < 1e-4 and es < 1e-3
        sel = dict(iou_thr=0.25, topk=3)
        free = walk.ask(PROMPTS)
        got, want = walk.ask(PROMPTS, **sel), inference.select_answers(free, **sel)
        assert len(got) == len(PROMPTS)
        for g, w in zip(got, want):
            assert torch.equal(g.keep, w.keep) and torch.equal(g.bboxes_3d.tensor, w.bboxes_3d.tensor) and 1 <= len(g.keep) <= 3
    assert walk.state_bytes() > 0
    for a in range(T_FRAMES):
        for b in range(a + 1, T_FRAMES):
            assert feats[a].shape != feats[b].shape or not torch.equal(feats[a], feats[b]), f'prefixes {a} and {b} got the same encoding'
    with pytest.raises(TypeError, match='unexpected'):
        walk.ask(PROMPTS, topk_per_class=3)


def test_walk_equals_encode_scene_and_ground_per_prefix(case, monkeypatch):
    walk_equals_batch(case, monkeypatch)


def walk_protocol(c):
    from embodiedscan_amd import engine as E
    det = c['det']
    dev = det.device
    with pytest.raises(ValueError, match='max_frames'):
        det.open_walk(c['meta'], max_frames=65)
    walk = det.open_walk(c['meta'], max_frames=T_FRAMES)
    first = _walk_pass(walk, c)
    walk.reset()
    assert walk.t == 0 and walk.cloud.n == 0 and len(walk.meta) == 0 and walk._scene is None
    with pytest.raises(ValueError, match='not observed'):
        walk.scene()
    E.TAPE.clear()
    det.train(True)
    E.TAPE.enabled = True
    try:
        second = _walk_pass(walk, c)
        assert det.training and E.TAPE.enabled and len(E.TAPE.fns) == 0, 'training flag / tape not restored, or something was recorded'
    finally:
        det.train(False)
    for t, (a, b) in enumerate(zip(first, second)):
        same = torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for p, q in zip(a[2], b[2]) for x, y in zip(p, q))
        assert same, f'prefix {t}: the pass after reset() is not bit-equal to the first'
    # every refusal comes before a launch and leaves t, the cloud length and the cached scene as they were
    walk = det.open_walk(c['meta'], max_frames=2)
    for t, rows, d2i, _ in c['frames'][:2]:
        walk.observe(c['imgs'][0, t], rows, d2i)
    scene = walk.scene()
    state = (walk.t, walk.cloud.n, len(walk.meta))
    t, rows, d2i, _ = c['frames'][2]
    img = c['imgs'][0, t]

    def unchanged(what):
        assert (walk.t, walk.cloud.n, len(walk.meta)) == state and walk._scene is scene, f'{what}: the session moved'

    with pytest.raises(ValueError, match='max_frames'):
        walk.observe(img, rows, d2i)
    unchanged('a full walk')
    for key, bump in ((E.WEIGHT_VERSION, lambda v: v + 1), (E.PRECISION, lambda v: 'bf16' if v != 'bf16' else 'f32')):
        old = key[0]
        key[0] = bump(old)
        try:
            for call in (lambda: walk.observe(img, rows, d2i), walk.scene, lambda: walk.ask(PROMPTS)):
                with pytest.raises(ValueError, match='stale'):
                    call()
        finally:
            key[0] = old
        unchanged('stale weights / precision')
    walk2 = det.open_walk(c['meta'], max_frames=T_FRAMES)
    walk2.observe(c['imgs'][0, 0], c['frames'][0][1], c['frames'][0][2])
    scene2, state2 = walk2.scene(), (walk2.t, walk2.cloud.n, len(walk2.meta))
    bad = [(img.cpu(), rows, 'walk on')] if dev.type == 'cuda' else []
    bad += [(img[None], rows, r'\(3, H, W\)'), (img.double(), rows, r'\(3, H, W\)'), (img, rows[:, 0], r'\(k, >= 3\)'), (img, rows[:, :2], r'\(k, >= 3\)')]
    for im, pt, match in bad:
        with pytest.raises(ValueError, match=match):
            walk2.observe(im, pt, d2i)
        assert (walk2.t, walk2.cloud.n, len(walk2.meta)) == state2 and walk2._scene is scene2
    assert walk.scene() is scene and walk2.scene() is scene2


def test_walk_protocol(case):
    walk_protocol(case)
