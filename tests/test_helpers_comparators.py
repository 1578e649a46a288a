"""The NaN-aware comparators of tests/helpers.py: identical bits pass, a NaN matches a NaN of any sign or payload, anything else fails
and the message names the count and the first indices.  And the guarded output buffers of tests/gpu_kit.py, run on the CPU: a clean
buffer passes, a byte written behind the words fails, a wrong word is named by its index."""
import numpy as np
import pytest
import torch

from gpu_kit import GUARD, POISON, check_words, poisoned, words_of, zeroed
from helpers import assert_f32_bits_equal, assert_rays_equal
from oracle.pyoracle import RAY_DT

X86_NAN, GFX_NAN = 0xFFC00000, 0x7FC00000


def f32(words):
    return np.array(words, np.uint32).view(np.float32)


def test_f32_bits():
    a = f32([[0x3F800000, X86_NAN, 0], [0x80000000, 0x7F800000, 0x7FC12345]])
    b = f32([[0x3F800000, GFX_NAN, 0], [0x80000000, 0x7F800000, X86_NAN]])
    assert_f32_bits_equal(a, b)
    for wrong in (f32([[0x3F800001, GFX_NAN, 0], [0x80000000, 0x7F800000, X86_NAN]]),   # one ulp
                  f32([[0x3F800000, GFX_NAN, 0x80000000], [0x80000000, 0x7F800000, X86_NAN]]),   # -0 for +0
                  f32([[0x3F800000, 0x7F800000, 0], [0x80000000, 0x7F800000, X86_NAN]])):        # Inf for NaN
        with pytest.raises(AssertionError, match=r"1 of 2 entries differ in their bits, first \[0\]"):
            assert_f32_bits_equal(a, wrong, "case")
    with pytest.raises(AssertionError, match="shape"):
        assert_f32_bits_equal(a, b[:1])


def test_rays():
    a = np.zeros(5, RAY_DT)
    a["o"], a["d"], a["tmax"] = (1, 2, 3), (0, 0, 1), np.inf
    b = a.copy()
    a["d"][3], b["d"][3] = f32([X86_NAN] * 3), f32([GFX_NAN] * 3)
    assert_rays_equal(a, b)
    for field, value in (("tmax", np.float32(3e38)), ("tmin", -0.0), ("o", (1, 2, np.nextafter(np.float32(3), np.float32(4))))):
        c = b.copy()
        c[field][[1, 4]] = value
        with pytest.raises(AssertionError, match=r"2 of 5 rays differ in their bits, first \[1 4\]"):
            assert_rays_equal(a, c, field)
    c = b.copy()
    c["d"][3] = 0   # a number where the other side has a NaN
    with pytest.raises(AssertionError, match=r"1 of 5 rays differ"):
        assert_rays_equal(a, c)
    with pytest.raises(AssertionError):
        assert_rays_equal(a, b[:4])


# ---- the guarded output buffers of tests/gpu_kit.py, on the CPU ------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint32, np.uint64])
def test_guarded_buffer_clean_passes(dtype):
    n, width = 37, np.dtype(dtype).itemsize
    out = zeroed(n, width, device="cpu")
    want = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(dtype)
    out[:n * width] = torch.from_numpy(want.view(np.uint8).copy())
    assert np.array_equal(words_of(out, n, dtype), want)
    check_words(out, want.reshape(1, n), dtype, "clean")


def test_guarded_buffer_zeroed_zeroes_exactly_the_words():
    raw = zeroed(5, 8, device="cpu").numpy()
    assert len(raw) == 40 + GUARD and not raw[:40].any() and (raw[40:] == POISON).all()
    raw = poisoned(40, device="cpu").numpy()
    assert len(raw) == 40 + GUARD and (raw == POISON).all()


@pytest.mark.parametrize("at", [0, 1, GUARD - 1])
def test_guarded_buffer_byte_behind_the_words_fails(at):
    n, width = 9, 4
    out = zeroed(n, width, device="cpu")
    out[n * width + at] = 0
    with pytest.raises(AssertionError, match="bytes behind an output were written"):
        words_of(out, n, np.uint32)
    with pytest.raises(AssertionError, match="behind"):
        check_words(out, np.zeros(n, np.uint32), np.uint32, "guard")


def test_guarded_buffer_wrong_word_is_named():
    n = 20
    out = zeroed(n, 4, device="cpu")
    want = np.zeros(n, np.uint32)
    want[[3, 17]] = (7, 1 << 31)
    with pytest.raises(AssertionError, match=r"case: 2 of 20 items differ, first items \[ 3 17\]: got \[0 0\] want \[ +7 2147483648\]"):
        check_words(out, want, np.uint32, "case")
    out[17 * 4 + 3] = 0x80  # little-endian: the top byte of word 17
    with pytest.raises(AssertionError, match=r"case: 1 of 20 items differ, first items \[3\]"):
        check_words(out, want, np.uint32, "case")
