"""Asking a recording in words (embodiedscan_amd.inference: ground_scene, ask_walk, --prompt) on the MI355X: the demo folder of
tests/test_gpu_inference.py (synth.write_demo_scene: 4 frames at 60 x 80) and the shipped grounding configuration with the small settings
of tests/test_gpu_grounding._small_grounder (text encoder TEXT_CFG, 32 queries, 2 decoder layers, FFN 128, pruning threshold 300)
written to a temporary config next to a checkpoint of the seeded weights; pipeline: 4 images resized to 128 x 128, 2000 points per frame.
ground_scene and ask_walk are held to the same steps done by hand -- encode_scene + ground + select_answers, a GroundWalk over the
frames --, --render to render_boxes with one colour per prompt, the command line to its JSON schema and its two usage errors.  The
score threshold is the median score of the run, so that rows fall on both sides of it.  Model and references are made once per module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_gpu_grounding as TG
import test_gpu_inference as TI

pytestmark = pytest.mark.gpu
ROOT = TI.ROOT
SEED = TI.SEED
PROMPTS = ['the chair next to the window', 'find the table that is closer to the door', 'the lamp']
T_FRAMES = 4

demo = TI.demo          # the module-scoped folder fixture


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def _same(a, b, what):
    assert torch.equal(a.keep, b.keep), f'{what}: chosen rows differ: {a.keep.tolist()} / {b.keep.tolist()}'
    assert torch.equal(a.bboxes_3d.tensor, b.bboxes_3d.tensor) and torch.equal(a.scores_3d, b.scores_3d), what


@pytest.fixture(scope='module')
def grounder(dev, demo, tmp_path_factory):
    """the grounder through a written config and a saved checkpoint, as the command line gets them; by hand: the whole folder encoded
    once and grounded, and a GroundWalk over its frames"""
    from embodiedscan_amd import inference as I, pipeline
    from embodiedscan_amd.checkpoint import save_checkpoint
    from embodiedscan_amd.config import load_config
    work = str(tmp_path_factory.mktemp('cfg'))
    shipped = os.path.join(ROOT, 'configs', 'mv_grounding.py')
    cfg_path = os.path.join(work, 'mv_grounding_small.py')
    with open(cfg_path, 'w') as f:
        f.write(f"_base_ = [{shipped!r}]\n"
                f"model = dict(num_queries=32, text_encoder_cfg=dict({', '.join(f'{k}={v!r}' for k, v in TG.TEXT_CFG.items())}),\n"
                f"             decoder=dict(num_layers=2, layer_cfg=dict(ffn_cfg=dict(feedforward_channels=128))),\n"
                f"             neck_3d=dict(pts_prune_threshold=300))\n"
                f"test_pipeline = {TI._small_pipeline(load_config(shipped))!r}\n")
    _, seeded, _ = TG._small_grounder(dev)
    ckpt = os.path.join(work, 'weights.pth')
    save_checkpoint(seeded, ckpt)
    del seeded
    det, cfg = I.init_model(cfg_path, ckpt, device=dev)
    assert not det.training and det.num_queries == 32 and det.decoder.num_layers == 2
    pipe = I.pipeline_of(cfg)
    dscan = TI._scan(det, demo, pipe)
    data = det.data_preprocessor(pipeline.make_batch([dscan]), False)
    scene = det.encode_scene(data['inputs'], data['data_samples'])[0]
    raw = det.ground(scene, PROMPTS)
    raw = [type(r)(bboxes_3d=r.bboxes_3d, scores_3d=r.scores_3d.clone()) for r in raw]
    thr = TI._split(torch.cat([r.scores_3d for r in raw]))
    # the walk by hand, on the frame-ordered form of the pipeline
    wscan = TI._scan(det, demo, I.sweeps_pipeline(pipe))
    batch = pipeline.make_batch([wscan])
    cloud = batch['inputs']['points'][0]
    wdata = det.data_preprocessor(batch, False)
    imgs = wdata['inputs']['imgs'].clone()
    meta = dict(wdata['data_samples'][0].metainfo)
    meta['depth2img'] = {k: v for k, v in meta['depth2img'].items() if k not in ('extrinsic', 'intrinsic')}
    walk = det.open_walk(meta, max_frames=T_FRAMES)
    walked = []
    for t, (r0, r1), e, i in pipeline.walk_frames(wscan, cloud.shape[0]):
        walk.observe(imgs[0, t], cloud[r0:r1], dict(extrinsic=e, intrinsic=i))
        walked.append([type(r)(bboxes_3d=r.bboxes_3d, scores_3d=r.scores_3d.clone()) for r in walk.ask(PROMPTS)])
    torch.cuda.synchronize()
    assert len(walked) == T_FRAMES
    return dict(det=det, cfg_path=cfg_path, ckpt=ckpt, pipe=pipe, dscan=dscan, wscan=wscan, raw=raw, walked=walked, thr=thr,
                sel=dict(iou_thr=0.25, score_thr=thr, topk=3))


def test_ground_scene_equals_encode_ground_select_by_hand(grounder, demo):
    from embodiedscan_amd import inference as I
    c, det = grounder, grounder['det']
    folder = os.path.join(demo, 'room')
    raw = I.ground_scene(det, folder, c['pipe'], PROMPTS, seed=SEED, select=None)
    assert len(raw) == len(PROMPTS)
    for r, w in zip(raw, c['raw']):
        assert torch.equal(r.bboxes_3d.tensor, w.bboxes_3d.tensor) and torch.equal(r.scores_3d, w.scores_3d) and len(r.scores_3d) == 32
    got = I.ground_scene(det, folder, c['pipe'], PROMPTS, seed=SEED, select=c['sel'])
    want = I.select_answers(c['raw'], **c['sel'])
    n = 0
    for p, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f'prompt {p}')
        assert bool((g.scores_3d >= c['thr']).all()) and len(g.keep) <= 3
        n += len(g.keep)
    print(f'ground_scene: {[len(g.keep) for g in got]} answers of 32 rows per prompt at score >= {c["thr"]:.4f}')
    assert 0 < n
    one = I.ground_scene(det, folder, c['pipe'], PROMPTS[:1], seed=SEED)                  # the defaults: "the" answer
    assert len(one) == 1 and one[0].keep.tolist() == [int(c['raw'][0].scores_3d.argmax())]
    other = I.ground_scene(det, folder, c['pipe'], PROMPTS, seed=SEED + 1, select=None)[0]
    assert not torch.equal(other.scores_3d, c['raw'][0].scores_3d), 'the seed does not reach the pipeline'
    with pytest.raises(ValueError, match='prompt'):
        I.ground_scene(det, folder, c['pipe'], [])
    # what was there before stays: the object-list entry points still refuse a grounder
    with pytest.raises(ValueError, match='a grounder needs a prompt'):
        I.run_scene(det, folder, c['pipe'])


def test_ask_walk_yields_the_answers_of_every_prefix(grounder, demo):
    from embodiedscan_amd import inference as I
    c, det = grounder, grounder['det']
    folder = os.path.join(demo, 'room')
    got = list(I.ask_walk(det, folder, c['pipe'], PROMPTS, seed=SEED, select=c['sel']))
    assert [t for t, _ in got] == list(range(T_FRAMES))
    for t, ans in got:
        for p, (g, w) in enumerate(zip(ans, I.select_answers(c['walked'][t], **c['sel']))):
            _same(g, w, f'prefix {t}, prompt {p}')
    last = got[-1][1]
    for t, ans in got[:-1]:
        assert any(a.bboxes_3d.tensor.shape != b.bboxes_3d.tensor.shape or not torch.equal(a.bboxes_3d.tensor, b.bboxes_3d.tensor)
                   for a, b in zip(ans, last)), f'prefix {t} answers like the whole walk'
    raw = list(I.ask_walk(det, folder, c['pipe'], PROMPTS, seed=SEED, select=None, every=2, max_frames=3))
    assert [t for t, _ in raw] == [1, 2], 'every = 2 over 3 frames: after frame 1 and behind the last'
    for t, ans in raw:
        assert all(torch.equal(a.scores_3d, w.scores_3d) for a, w in zip(ans, c['walked'][t]))
    with pytest.raises(ValueError, match='every'):
        next(I.ask_walk(det, folder, c['pipe'], PROMPTS, every=0))


def _load_frames(dir, n):
    from PIL import Image
    names = sorted(f for f in os.listdir(dir) if f.endswith('.png'))
    assert names == [f'frame_{k:04d}.png' for k in range(n)], names
    return np.stack([np.asarray(Image.open(os.path.join(dir, f))) for f in names])


def test_render_draws_every_prompt_in_its_colour(grounder, demo, tmp_path):
    from embodiedscan_amd import inference as I, render as RD
    c, det = grounder, grounder['det']
    folder = os.path.join(demo, 'room')
    pal = RD.class_palette(len(PROMPTS) + 1)[1:]
    pal_dev = torch.from_numpy(pal).to(det.device)

    def by_hand(dscan, answers, views):
        E, K = I.frame_matrices(dscan)
        boxes = torch.cat([a.bboxes_3d.tensor for a in answers])
        colors = torch.cat([pal_dev[p:p + 1].expand(len(a.keep), 3) for p, a in enumerate(answers)]).contiguous()
        return RD.render_boxes(dscan['img'][views], E[views], K[views], boxes, colors, layout='chw').cpu().numpy()

    out = str(tmp_path / 'whole')
    ans = I.ground_scene(det, folder, c['pipe'], PROMPTS, seed=SEED, select=c['sel'], render=out)
    with open(os.path.join(out, 'legend.json')) as f:
        legend = json.load(f)
    assert list(legend) == PROMPTS and [legend[p] for p in PROMPTS] == pal.tolist()
    frames = _load_frames(out, T_FRAMES)
    assert np.array_equal(frames, by_hand(c['dscan'], ans, slice(0, T_FRAMES)))
    plain = c['dscan']['img'].permute(0, 2, 3, 1).cpu().numpy()
    changed = (frames != plain).any(-1)
    print(f'ground_scene --render: {int(changed.sum())} of {changed.size} pixels drawn')
    assert changed.any() and not changed.all()
    out = str(tmp_path / 'walk')
    got = list(I.ask_walk(det, folder, c['pipe'], PROMPTS, seed=SEED, select=c['sel'], render=out))
    frames = _load_frames(out, T_FRAMES)
    for t, a in got:
        assert np.array_equal(frames[t], by_hand(c['wscan'], a, slice(t, t + 1))[0]), f'frame {t} is not drawn under the answers of prefix {t}'
    with open(os.path.join(out, 'legend.json')) as f:
        assert json.load(f) == legend


def _cli(args):
    return subprocess.run([sys.executable, '-m', 'embodiedscan_amd.inference'] + args, cwd=ROOT, capture_output=True, text=True, timeout=300)


def test_command_line_writes_the_answers_of_every_prefix(grounder, demo, tmp_path):
    from embodiedscan_amd import inference as I
    c = grounder
    out = str(tmp_path / 'answers.json')
    listed = str(tmp_path / 'prompts.txt')
    with open(listed, 'w') as f:
        f.write(PROMPTS[1] + '\n\n' + PROMPTS[2] + '\n')
    res = _cli([c['cfg_path'], c['ckpt'], '--root-dir', demo, '--scene', 'room', '--walk', '--seed', str(SEED), '--prompt', PROMPTS[0],
                '--prompts-file', listed, '--topk', '3', '--score-thr', repr(c['thr']), '--out', out])
    assert res.returncode == 0, res.stderr[-3000:]
    with open(out) as f:
        doc = json.load(f)
    assert doc['scene'] == 'demo/room' and doc['walk'] is True and doc['model'] == 'SparseFeatureFusion3DGrounder'
    assert doc['select'] == dict(iou_thr=0.25, score_thr=c['thr'], topk=3)
    assert len(doc['results']) == T_FRAMES * len(PROMPTS)
    for k, rec in enumerate(doc['results']):
        t, p = divmod(k, len(PROMPTS))
        want = I.select_answers(c['walked'][t], **c['sel'])[p]
        assert set(rec) == {'t', 'prompt', 'boxes', 'scores', 'keep'} and rec['t'] == t and rec['prompt'] == PROMPTS[p]
        assert rec['keep'] == want.keep.tolist() and len(rec['boxes']) == len(rec['scores']) == len(rec['keep']) and all(len(b) == 9 for b in rec['boxes'])


def test_command_line_usage_errors(grounder, demo):
    """a grounder without a prompt, a prompt without a grounder: a usage message and a non-zero exit, before any model is built"""
    c = grounder
    res = _cli([c['cfg_path'], c['ckpt'], '--root-dir', demo, '--scene', 'room'])
    assert res.returncode != 0 and 'usage:' in res.stderr and '--prompt' in res.stderr, res.stderr[-2000:]
    res = _cli([os.path.join(ROOT, 'configs', 'cont_det3d.py'), '--root-dir', demo, '--scene', 'room', '--prompt', PROMPTS[0]])
    assert res.returncode != 0 and 'usage:' in res.stderr and 'takes no prompt' in res.stderr, res.stderr[-2000:]
