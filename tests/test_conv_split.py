"""The split-f16 3x3 convolution (gmz_conv3x3_forward_split, trainer.TARGET_SPLIT) without a GPU: the operand split
itself (trainer.split_f16, the specification of the kernel's arithmetic), the C entry points' refusals with fake
pointers that are never dereferenced (the tests/test_conv_sizes.py pattern), and the Python path's fallbacks on the
CPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN


@pytest.fixture(scope="module")
def T():
    from datou_gomoku_muzero_amd import trainer
    return trainer


def bits22(rs, shape):
    """float32 values with at most 22 significant bits (the low 2 mantissa bits cleared), magnitudes in [0.125, 1),
    random signs: hi + lo * 2^-11 of their split is exact."""
    v = rs.uniform(0.125, 1.0, shape).astype(np.float32)
    v = (v.view(np.uint32) & np.uint32(0xFFFFFFFC)).view(np.float32)
    return v * rs.choice([-1.0, 1.0], shape).astype(np.float32)


def test_split_reconstructs_22_bit_values_exactly(T):
    v = torch.from_numpy(bits22(np.random.RandomState(0), (1 << 16,)))
    assert float(v.abs().min()) >= 0.125 and float(v.abs().max()) < 1.0
    hi, lo = T.split_f16(v)
    assert hi.dtype == torch.float16 and lo.dtype == torch.float16
    back = hi.float() + lo.float() * 2.0 ** -11
    assert torch.equal(back.view(torch.int32), v.view(torch.int32))
    nz = lo.float().abs()[lo != 0]
    assert float(nz.min()) >= 2.0 ** -14, float(nz.min())  # no lo in the f16 subnormals (measured: 1.2e-4)


def test_split_of_zero_is_zero(T):
    hi, lo = T.split_f16(torch.zeros(8))
    assert not hi.any() and not lo.any()


def test_split_of_general_values_is_within_the_stated_bound(T):
    rs = np.random.RandomState(1)
    v = (rs.randn(1 << 16) * 10.0 ** rs.uniform(-12, 4, 1 << 16)).astype(np.float32)
    v = v[np.abs(v) < 2.0 ** 15]
    hi, lo = T.split_f16(torch.from_numpy(v))
    back = hi.double().numpy() + lo.double().numpy() * 2.0 ** -11
    err = np.abs(back - v.astype(np.float64))
    lim = np.maximum(2.0 ** -22 * np.abs(v.astype(np.float64)), 2.0 ** -35)
    assert np.all(err <= lim), float((err / lim).max())


def _lib():
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    return lib, ctypes.c_void_p(1 << 20), (lambda: lib.gmz_last_error().decode())


@pytest.mark.parametrize("H", [7, 20])
def test_forward_split_refuses_an_unsupported_size_with_the_list(H):
    lib, fake, err = _lib()
    assert lib.gmz_conv3x3_forward_split(H, fake, fake, ctypes.c_void_p(1 << 21), 4, None, None, None, None, 0.0, None, 0,
                                         None) < 0
    msg = err()
    assert "board size must be" in msg, msg
    assert [int(v) for v in re.findall(r"\d+", msg.split("board size must be")[1])] == [6, 9, 15, 19], msg


def test_forward_split_refuses_epilogue_operands_without_gamma():
    lib, fake, err = _lib()
    y = ctypes.c_void_p(1 << 21)
    assert lib.gmz_conv3x3_forward_split(9, fake, fake, y, 4, None, None, None, None, 0.0, fake, 0, None) < 0
    assert "gamma" in err(), err()
    assert lib.gmz_conv3x3_forward_split(9, fake, fake, y, 4, None, None, None, None, 0.0, None, 1, None) < 0
    assert "gamma" in err(), err()
    assert lib.gmz_conv3x3_forward_split(9, fake, fake, y, 0, None, None, None, None, 0.0, None, 0, None) < 0
    assert lib.gmz_conv3x3_forward_split(9, None, fake, y, 4, None, None, None, None, 0.0, None, 0, None) < 0


def test_pack_split_many_refuses_no_jobs():
    lib, fake, err = _lib()
    assert lib.gmz_conv3x3_pack_split_many(fake, 0, None) < 0
    assert "n_jobs" in err(), err()
    assert lib.gmz_conv3x3_pack_split(None, 1, 1, 1, 1, 0, fake, None) < 0


def test_split_value_on_the_cpu_is_the_float32_forward(T):
    import test_trainer as tt
    torch.set_num_threads(4)
    d = np.load(os.path.join(GOLDEN, "train_loss_c6w128full.npz"))
    cfg, _, target = tt._nets(T, *tt._shape(d))
    obs = torch.from_numpy(d["obs"])[:, -1]
    v = target.initial_value(obs)
    vs = target.initial_value(obs, split=True)
    assert torch.equal(v.view(torch.int32), vs.view(torch.int32))
    with pytest.raises(ValueError):
        target.initial_value(obs, f16=True, split=True)


def test_target_split_is_off_by_default(T):
    assert T.TARGET_SPLIT is False
