"""Host side of the opt-in text encoder: the `text_encoder_impl` argument of SparseFeatureFusion3DGrounder and the ES_TEXT_ENCODER
default rule, the registry pass-through, HipTextEncoder.from_module's refusals, and the state-dict round trip under the transformers
module's own key names (Q / K / V split out of the fused kernel copy and fused again).  No GPU: everything stays on CPU tensors."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(vocab_size=100, hidden_size=128, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256, max_position_embeddings=40)


def _model_cfg(**extra):
    from embodiedscan_amd.config import load_config
    m = load_config(os.path.join(ROOT, 'configs', 'mv_grounding.py'))['model']
    m['text_encoder_cfg'] = TINY
    m.update(device='cpu', seed=0, **extra)
    return m


def _build(**extra):
    from embodiedscan_amd import models  # noqa: F401
    from embodiedscan_amd.registry import MODELS
    return MODELS.build(_model_cfg(**extra))


def test_argument_environment_default_and_registry(monkeypatch):
    from embodiedscan_amd.text import HipTextEncoder
    monkeypatch.delenv('ES_TEXT_ENCODER', raising=False)
    det = _build()
    assert det.text_encoder_impl == 'torch' and isinstance(det.text_encoder, torch.nn.Module)      # unset means torch
    det = _build(text_encoder_impl='hip')                                                         # through MODELS.build
    assert det.text_encoder_impl == 'hip' and isinstance(det.text_encoder, HipTextEncoder)
    assert det.text_dim == det.text_encoder.config.hidden_size == 128
    monkeypatch.setenv('ES_TEXT_ENCODER', 'hip')
    assert _build().text_encoder_impl == 'hip'
    assert _build(text_encoder_impl='torch').text_encoder_impl == 'torch'                         # the argument wins
    monkeypatch.setenv('ES_TEXT_ENCODER', 'cublas')
    with pytest.raises(ValueError, match='text_encoder_impl'):
        _build()


def test_both_builds_start_from_identical_weights(monkeypatch):
    monkeypatch.delenv('ES_TEXT_ENCODER', raising=False)
    a, b = _build().state_dict(), _build(text_encoder_impl='hip').state_dict()
    assert list(a) == list(b)
    assert all(torch.equal(a[k], b[k]) for k in a if k.startswith('text_encoder.'))


@pytest.mark.parametrize('change,word', [(dict(hidden_act='relu'), 'gelu'), (dict(num_attention_heads=4), 'head dimension 64'),
                                         (dict(position_embedding_type='relative_key'), 'absolute'),
                                         (dict(is_decoder=True, add_cross_attention=True), 'cross-attention')])
def test_from_module_refusals(change, word):
    from transformers import RobertaConfig
    from embodiedscan_amd.text import HipTextEncoder
    cfg = RobertaConfig(**TINY)
    for k, v in change.items():
        setattr(cfg, k, v)
    with pytest.raises(ValueError, match=word):
        HipTextEncoder(cfg, {})


def test_state_dict_round_trip_under_the_modules_key_names():
    from embodiedscan_amd.text import HipTextEncoder, build_text_encoder
    model = build_text_encoder(TINY, seed=2)
    enc = HipTextEncoder.from_module(model)
    want = model.state_dict()
    got = enc.state_dict()
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) and got[k].shape == want[k].shape for k in want)
    assert all(got[k].data_ptr() != want[k].data_ptr() for k in want), 'the module must not be kept'
    # the fused kernel copy is [q | k | v] along the output columns, in both layouts
    ly, p = enc._layers[1], 'encoder.layer.1.attention.self.'
    fused = torch.cat([want[p + n + '.weight'] for n in ('query', 'key', 'value')], 0)
    assert torch.equal(ly['wqkv'].d[0], fused.t()) and torch.equal(ly['wqkv'].t[0], fused.to(torch.bfloat16))
    assert torch.equal(ly['bqkv'].d, torch.cat([want[p + n + '.bias'] for n in ('query', 'key', 'value')]))
    # loading other weights refreshes the fused and the bf16 copies
    other = {k: v + 1 if v.is_floating_point() else v for k, v in build_text_encoder(TINY, seed=3).state_dict().items()}
    enc.load_state_dict(other)
    fused = torch.cat([other[p + n + '.weight'] for n in ('query', 'key', 'value')], 0)
    assert torch.equal(enc._layers[1]['wqkv'].d[0], fused.t()) and torch.equal(enc._layers[1]['wqkv'].t[0], fused.to(torch.bfloat16))
    assert all(torch.equal(enc.state_dict()[k], other[k]) for k in other)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        enc.load_state_dict({p + 'query.weight': torch.zeros(3, 3)}, strict=False)
