"""CPU: the sizes of the decoder forward's marked-plane region (persist.hip: vag_dec_fwd_planes_floats) and of the caller's plane
buffer that holds it (vag_handoff_planes_floats), and the option that selects the form.  Host arithmetic only: no device call."""
import pytest

# the shapes of tests/test_gpu_dec_fwd_planes.py and the headline workload (bench.py configs[1])
SHAPES = [(256, 3, 5, 3), (512, 17, 7, 3), (512, 64, 40, 2), (512, 112, 4, 3), (512, 5, 3, 1)]
CONFIGS_1 = (512, 64, 40, 40)
DEFAULT = 15


def _tiles(B):
    return (B + 15) // 16


def _block_floats(K):
    """one (step, row tile) block of rows of K values: K / 32 k-steps of three planes of 64 slots of 8 bf16"""
    return (K // 32) * 3 * 64 * 16 // 4


def _dec_fwd(H, B, Tt):
    return 2 * Tt * _tiles(B) * _block_floats(H)


def _enc_fwd(H, B, Ts):
    return 2 * Ts * _tiles(B) * _block_floats(H)


def _enc_bwd(H, B, Ts):
    return 2 * Ts * _tiles(B) * _block_floats(3 * H)


def _dec_bwd(H, B, Tt):
    """dq, dgh1 and dgh2 blocks and the W_hh2^T regions (8 x 3H values, 6 bytes each) of the workgroups of the widest launch a
    device of at most 256 CUs makes (tests/test_gpu_hidden_planes.py: _decoder_floats)"""
    RT, wgs = _tiles(B), H // 8
    return Tt * RT * (_block_floats(2 * H) + 2 * _block_floats(3 * H)) + min(RT, 256 // wgs) * wgs * 8 * 3 * H * 6 // 4


def _lib():
    from vagnmt_hip import _lib
    return _lib.lib()


@pytest.mark.parametrize("H,B,Ts,Tt", SHAPES + [CONFIGS_1])
def test_dec_fwd_planes_floats_is_two_blocks_per_step_and_row_tile(H, B, Ts, Tt):
    assert _lib().vag_dec_fwd_planes_floats(B, Tt, H) == _dec_fwd(H, B, Tt)


def test_the_headline_shape_needs_what_the_issue_states():
    H, B, Ts, Tt = CONFIGS_1
    assert _lib().vag_dec_fwd_planes_floats(B, Tt, H) == 3932160
    assert _lib().vag_handoff_planes_floats(B, Ts, Tt, H) == 20447232          # the decoder backward's need: unchanged


@pytest.mark.parametrize("H,B,Ts,Tt", SHAPES + [CONFIGS_1])
def test_handoff_planes_floats_is_the_largest_of_both_forwards_and_each_backward(H, B, Ts, Tt):
    want = max(_enc_fwd(H, B, Ts) + _dec_fwd(H, B, Tt), _enc_bwd(H, B, Ts), _dec_bwd(H, B, Tt))
    assert _lib().vag_handoff_planes_floats(B, Ts, Tt, H) == want
    assert want >= _enc_fwd(H, B, Ts) + _dec_fwd(H, B, Tt) > 0


@pytest.mark.parametrize("H,B,Tt", [(384, 16, 3), (1024, 16, 3), (512, 65, 3), (512, 0, 3), (512, 16, 0)])
def test_a_shape_without_a_one_launch_decoder_has_no_region(H, B, Tt):
    # H other than 256 and 512; a batch that no device takes in one launch or two full enough ones (B = 65 at H = 512); empty shapes
    assert _lib().vag_dec_fwd_planes_floats(B, Tt, H) == 0


def test_the_option_accepts_every_mask_of_five_bits():
    L = _lib()
    try:
        for mask in range(32):
            assert L.vag_set_option(b"handoff_planes", mask) == 0
    finally:
        L.vag_set_option(b"handoff_planes", DEFAULT)
