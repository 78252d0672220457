"""The 3x3 family's board sizes (csrc/gmz_conv.hip ConvSizes): an unsupported size is refused before any launch, and
the refusal names every supported size — forward family and weight gradient from the one list.  No GPU: fake
pointers, never dereferenced (the tests/test_abi.py pattern); no supported size is called with them.  And the
float32 restatement of the reference's loss on the CPU at 19x19 and 6x6 with the production width (128 filters)."""
import ctypes
import re

import pytest


def _lib():
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    return lib, ctypes.c_void_p(1 << 20), (lambda: lib.gmz_last_error().decode())


def _sizes(msg):
    assert "board size must be" in msg, msg
    return [int(v) for v in re.findall(r"\d+", msg.split("board size must be")[1])]


def test_forward_refuses_an_unsupported_size_with_the_list():
    lib, fake, err = _lib()
    assert lib.gmz_conv3x3_forward(1, 7, fake, fake, fake, 4, None) < 0
    assert _sizes(err()) == [6, 9, 15, 19], err()
    assert lib.gmz_conv3x3_forward_add(2, 12, fake, fake, fake, fake, 4, None) < 0
    assert _sizes(err()) == [6, 9, 15, 19], err()


def test_wgrad_refuses_an_unsupported_size_with_the_list():
    lib, fake, err = _lib()
    assert lib.gmz_conv3x3_wgrad(1, 7, fake, fake, 4, fake, 1, 1, 1, 1, 0, fake, 1 << 30, None) < 0
    assert _sizes(err()) == [6, 9, 15, 19], err()
    segs = (ctypes.c_void_p * 2)(1 << 20, 1 << 21)
    assert lib.gmz_conv3x3_wgrad_segments(2, 20, ctypes.cast(segs, ctypes.c_void_p), ctypes.cast(segs, ctypes.c_void_p), 2,
                                          4, fake, 1, 1, 1, 1, 1, fake, 1 << 30, None) < 0
    assert _sizes(err()) == [6, 9, 15, 19], err()


@pytest.fixture(scope="module")
def T():
    from datou_gomoku_muzero_amd import trainer
    return trainer


@pytest.mark.parametrize("fixture", ["train_loss_c19full.npz", "train_loss_c6w128full.npz"])
def test_loss_and_gradients_match_reference_at_the_new_sizes(T, fixture):
    """test_trainer.test_loss_and_gradients_match_reference_at_production_width (CPU, float32, its bounds) on the
    reference's calculate_loss at 19x19 and 6x6 with 128 filters (tests/golden/make_golden_trainer_sizes.py)."""
    import test_trainer as tt
    tt.test_loss_and_gradients_match_reference_at_production_width(T, fixture)
