"""decode_scaled: the numpy restatement of the PBA_RECORD_F16_SCALED layout (include/pba.h), on hand-built records."""
import numpy as np

from helpers import engine_module

E = engine_module()


def half_bits(x):
    return np.asarray(x, np.float16).view(np.uint16)


def test_decode_scaled_hand_built_record():
    P = 3  # odd: 45 halves per block
    r = [1.5, -255.0, 0.0]
    e = [1.0, 2.0, 8.0]
    jh = np.arange(18, dtype=np.float64).reshape(3, 6) * 1000.0 - 4000.0  # row k: 6 stored halves
    jt = -np.arange(18, dtype=np.float64).reshape(3, 6) * 0.25
    jr = [65504.0, -32768.0, 16384.0]
    block = np.concatenate([r, jh.ravel(), jt.ravel(), jr, e])
    raw = np.stack([half_bits(block), np.zeros(15 * P, np.uint16)])  # second block: an invalid block's zeros
    out = E.decode_scaled(raw, P)
    assert out.shape == (2, 14 * P) and out.dtype == np.float32
    sc = np.array(e)[:, None]
    expect = np.concatenate([r, (jh * sc).ravel(), (jt * sc).ravel(), np.array(jr) * np.array(e)])
    assert np.array_equal(out[0], expect.astype(np.float32))
    assert out[0, 13 * P + 1] == -65536.0 and out[0, 13 * P + 2] == 131072.0  # beyond the half range
    assert not out[1].any()


def test_decode_scaled_accepts_flat_input_and_even_patterns():
    P = 2
    block = np.array([3.0, 4.0] + [1.0] * 6 + [2.0] * 6 + [-1.0] * 6 + [-2.0] * 6 + [5.0, 6.0] + [4.0, 32768.0])
    out = E.decode_scaled(half_bits(block), P)  # one block, flat
    assert out.shape == (1, 28)
    assert np.array_equal(out[0], np.array([3.0, 4.0] + [4.0] * 6 + [65536.0] * 6 + [-4.0] * 6 + [-65536.0] * 6 +
                                           [20.0, 6.0 * 32768.0], np.float32))


def test_record_format_constants():
    assert (E.RECORD_F32, E.RECORD_F16, E.RECORD_F16_SCALED) == (0, 1, 2)
    src = open(E.HEADER).read()
    assert "#define PBA_RECORD_F16_SCALED 2" in src
    for name in ("pba_record_bytes", "pba_get_records_raw", "pba_decode_records_device"):
        assert name in E.header_functions()
