"""The flag names of include/es_hip.h as hip.CONSTS carries them and the statuses of hip.try_call (host only), then the bodies of
tests/test_gpu_engine_launch.py on the CPU emulator (tests/emu).  TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import pytest

from test_emu_product import emulated  # noqa: F401

# name -> the value the header documents next to the prototypes that accept it
FLAGS = dict(ES_ACC_ADD=1, ES_ACC_MIRROR=2, ES_ACC_ROWS_BF16=2, ES_ROWS_F32=0, ES_ROWS_BF16=1, ES_ROWS_PRE16=3, ES_ACT_NONE=0, ES_ACT_RELU=1,
             ES_ACT_ELU=2, ES_ACT_GATE=3, ES_DECLINED=-4, ES_GEN_DECLINED=1)
GEN = ('es_gen_transpose_fwd_bf16', 'es_gen_transpose_dgrad_bf16', 'es_gen_transpose_wgrad_bf16')


def test_flag_constants_are_parsed_from_the_header_signed_values_included():
    from embodiedscan_amd import hip
    assert {k: hip.CONSTS.get(k) for k in FLAGS} == FLAGS
    src = open(hip.HEADER_PATH).read()
    for k in FLAGS:                                  # each is one #define of its own: the same value under two names stays two names
        assert src.count(f'#define {k} ') == 1, k
    assert hip.CONSTS['ES_MAX_SEG'] == 32 and hip.CONSTS['ES_FUSE_PROJ'] == 32          # (the unsigned ones as before)


@pytest.mark.parametrize('name,declined', [('es_spconv_halo_bf16', -4), ('es_rows_wgrad1_bf16', -4), ('es_img_dgrad1_s2_bf16', -4),
                                           ('es_dconv_fwd_bf16', -4)] + [(n, 1) for n in GEN])
def test_try_call_knows_the_declined_status_of_its_entry(monkeypatch, name, declined):
    from embodiedscan_amd import hip
    status = [0]
    monkeypatch.setitem(hip._fn, name, lambda *a: status[0])
    assert hip.try_call(name, 0) is True
    status[0] = declined
    assert hip.try_call(name, 0) is False
    for bad in (-1, -3, -5, 2, 1 if declined == -4 else -4):
        status[0] = bad
        with pytest.raises(hip.HipError, match=f'{name} failed with status {bad}'):
            hip.try_call(name, 0)
        with pytest.raises(hip.HipError, match=f'{name} failed with status {bad}'):
            hip.call(name, 0)


@pytest.mark.parametrize('cin,cout,fwd_served,dgrad_served', [(32, 32, True, True), (16, 32, True, False), (8, 24, False, False)])
def test_gen_conv_transpose_asks_the_fused_entries_through_the_door(emulated, cin, cout, fwd_served, dgrad_served):  # noqa: F811
    import test_gpu_engine_launch as T
    T.gen_transpose_door_case(emulated, cin, cout, fwd_served, dgrad_served)


def test_a_failed_fused_launch_raises_and_queues_nothing_more(emulated, monkeypatch):  # noqa: F811
    import test_gpu_engine_launch as T
    T.gen_transpose_error_case(emulated, monkeypatch)


@pytest.mark.parametrize('name', ['add', 'concat_rows', 'union_add', 'layernorm', 'norm'])
def test_gradient_hand_over(emulated, name):  # noqa: F811
    import test_gpu_engine_launch as T
    T.handover_case(emulated, name)
