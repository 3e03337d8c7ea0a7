"""The host side of asking a recording in words (embodiedscan_amd.inference), without a GPU: what select_answers refuses before any
launch, the frame-ordered form of a pipeline that ask_walk reads a folder through, the palette of the prompts, and the two usage
errors of the command line, which come before a model is built."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_select_answers_refuses_before_any_launch():
    from embodiedscan_amd import inference as I
    from embodiedscan_amd.structures import InstanceData
    ok = InstanceData(bboxes_3d=torch.zeros((4, 9)), scores_3d=torch.zeros(4))
    with pytest.raises(ValueError, match='different numbers of rows'):
        I.select_answers([ok, InstanceData(bboxes_3d=torch.zeros((3, 9)), scores_3d=torch.zeros(3))])
    with pytest.raises(ValueError, match='1024'):
        I.select_answers((torch.zeros((2, 1025, 9)), torch.zeros((2, 1025))))
    for topk in (0, -1, 5):
        with pytest.raises(ValueError, match='topk'):
            I.select_answers([ok], topk=topk)
    with pytest.raises(ValueError, match='topk'):
        I.select_answers((torch.zeros((2, 0, 9)), torch.zeros((2, 0))), topk=2)
    with pytest.raises(ValueError, match=r'\(P, Q, 9\)'):
        I.select_answers((torch.zeros((2, 4, 8)), torch.zeros((2, 4))))
    with pytest.raises(ValueError, match=r'\(Q, 9\)'):
        I.select_answers([InstanceData(bboxes_3d=torch.zeros((4, 9)), scores_3d=torch.zeros(5))])
    assert I.select_answers([]) == []


def test_sweeps_pipeline_is_the_frame_ordered_form():
    from embodiedscan_amd import inference as I
    from embodiedscan_amd.config import load_config
    from embodiedscan_amd.datasets.loading import ScanPipeline
    for name in ('mv_grounding.py', 'mv_grounding_fcaf.py'):
        pipe = I.pipeline_of(load_config(os.path.join(ROOT, 'configs', name)))
        plain = ScanPipeline.from_cfg(pipe)
        assert not plain.sweeps and plain.n_images == 50 and plain.ordered and not plain.aug['rst'] and not plain.aug['flip']
        sw = I.sweeps_pipeline(pipe)
        types = [t['type'] for t in sw]
        assert 'PointSample' not in types and types.index('ConstructMultiSweeps') == types.index('Pack3DDetInputs') - 1
        assert [t for t in pipe if t['type'] == 'AggregateMultiViewPoints'][0].get('save_slices') is None, 'the input list was edited'
        made = ScanPipeline.from_cfg(sw)
        assert made.sweeps and (made.n_images, made.ordered, made.view_points, made.img_scale) == (50, True, plain.view_points, plain.img_scale)
        assert I.sweeps_pipeline(sw) is sw and I.sweeps_pipeline(made) is made
    cont = I.pipeline_of(load_config(os.path.join(ROOT, 'configs', 'cont_det3d.py')))
    assert I.sweeps_pipeline(cont) is cont


def test_prompt_palette_skips_the_grey_row():
    from embodiedscan_amd import inference as I, render as RD
    pal = I.prompt_palette(5)
    assert pal.shape == (5, 3) and (pal == RD.class_palette(6)[1:]).all() and len({tuple(r) for r in pal.tolist()}) == 5


@pytest.mark.parametrize('config,extra,needle', [('mv_grounding.py', [], '--prompt'), ('cont_det3d.py', ['--prompt', 'the chair'], 'takes no prompt'),
                                                 ('mv_3ddet.py', ['--prompts-file', 'PROMPTS'], 'takes no prompt')])
def test_command_line_usage_errors(config, extra, needle, tmp_path, capsys):
    from embodiedscan_amd import inference as I
    listed = tmp_path / 'prompts.txt'
    listed.write_text('the lamp\n')
    extra = [str(listed) if e == 'PROMPTS' else e for e in extra]
    with pytest.raises(SystemExit) as exc:
        I.main([os.path.join(ROOT, 'configs', config), '--root-dir', str(tmp_path), '--scene', 'room'] + extra)
    err = capsys.readouterr().err
    assert exc.value.code == 2 and 'usage:' in err and needle in err, err
