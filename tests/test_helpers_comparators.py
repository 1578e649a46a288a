"""The NaN-aware comparators of tests/helpers.py: identical bits pass, a NaN matches a NaN of any sign or payload, anything else fails
and the message names the count and the first indices."""
import numpy as np
import pytest

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
