"""The shared 16-bit element helpers (csrc/s6d_bf16.h: bf16_bits, bf16_value, bf16_split, kswz) are plain C++ behind the HIP
qualifiers: compile the header for the host against the emulator's HIP header (tests/host_cc/bf16_host.cc) and compare with
torch's CPU float32 -> bfloat16 conversion bit for bit -- a logic check that needs no GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import hipemu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

# float32 bit patterns with a story, and the bf16 bits they must give (None: a NaN, payload not pinned)
FIXED = [
    (0x00000000, 0x0000), (0x80000000, 0x8000),                      # +-0
    (0x00000001, 0x0000), (0x80000001, 0x8000),                      # the smallest subnormal rounds to zero
    (0x007fffff, 0x0080), (0x807fffff, 0x8080),                      # the largest subnormal rounds to the smallest normal
    (0x3f808000, 0x3f80),                                            # an exact tie: to even, down
    (0x3f818000, 0x3f82),                                            # an exact tie: to even, up
    (0x7f7fffff, 0x7f80), (0xff7fffff, 0xff80),                      # the largest finite value overflows to infinity
    (0x7f800000, 0x7f80), (0xff800000, 0xff80),                      # +-inf
    (0x7fc00000, None), (0x7f800001, None), (0xffffffff, None), (0x7fff8000, None),   # quiet, signalling, all ones, a carry into the sign
]


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bf16") / "libbf16_host.so")
    subprocess.check_call([hipemu.CXX, "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-I", hipemu.EMU, "-I", hipemu.CSRC, "-I",
                           os.path.join(REPO, "include"), "-o", so, os.path.join(HERE, "host_cc", "bf16_host.cc")])
    lib = ctypes.CDLL(so)
    lib.bf16_bits_host.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    lib.bf16_value_host.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p]
    lib.bf16_split_host.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_void_p]
    lib.kswz_host.argtypes = [ctypes.c_int]
    return lib


def _bits(L, x):
    out = np.empty(len(x), np.uint16)
    L.bf16_bits_host(x.ctypes.data, len(x), out.ctypes.data)
    return out


def _value(L, h):
    out = np.empty(len(h), np.float32)
    L.bf16_value_host(h.ctypes.data, len(h), out.ctypes.data)
    return out


def _torch_bits(x):
    return torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def _is_nan16(h):
    return (h & 0x7fff) > 0x7f80


def _patterns():
    rng = np.random.default_rng(0)
    return np.concatenate([np.array([b for b, _ in FIXED], np.uint32), rng.integers(0, 2 ** 32, 2 ** 20, dtype=np.uint64).astype(np.uint32)])


def test_bf16_bits_equals_torch(L):
    u = _patterns()
    x = u.view(np.float32)
    got, want = _bits(L, x), _torch_bits(x)
    for (b, h), g in zip(FIXED, got):
        assert _is_nan16(g) if h is None else g == h, f"{b:#010x} -> {int(g):#06x}, expected {'a NaN' if h is None else hex(h)}"
    nan = np.isnan(x)
    assert nan.sum() > 1000                                             # the random patterns do hold NaNs of every payload
    assert _is_nan16(got[nan]).all() and _is_nan16(want[nan]).all()     # a NaN stays a NaN; the payload is not pinned
    np.testing.assert_array_equal(got[~nan], want[~nan])


def test_bf16_value_is_the_left_shift(L):
    h = np.arange(2 ** 16, dtype=np.uint32).astype(np.uint16)
    np.testing.assert_array_equal(_value(L, h).view(np.uint32), h.astype(np.uint32) << 16)


def test_bf16_split(L):
    u = _patterns()
    x = u.view(np.float32)
    x = np.ascontiguousarray(x[np.isfinite(x)])
    hi, lo = np.empty(len(x), np.uint16), np.empty(len(x), np.uint16)
    L.bf16_split_host(x.ctypes.data, len(x), hi.ctypes.data, lo.ctypes.data)
    # hi = bf16(x), lo = bf16(x - hi): the same two conversions by torch, the subtraction in float32
    t_hi = _torch_bits(x)
    with np.errstate(invalid="ignore"):
        rest = x - (t_hi.astype(np.uint32) << 16).view(np.float32)
    np.testing.assert_array_equal(hi, t_hi)
    np.testing.assert_array_equal(hi, _bits(L, x))
    np.testing.assert_array_equal(lo, _torch_bits(rest))
    np.testing.assert_array_equal(lo, _bits(L, x - _value(L, hi)))
    # two roundings of 2^-8 relative each: |x - (hi + lo)| <= 2^-16 |x| where neither rounding leaves the normal range: x normal,
    # hi finite (|x| below the overflow threshold of the first rounding), lo normal -- or zero because x - hi IS zero (a lo that
    # is zero because x - hi underflowed bf16's range belongs to the subnormal case: no relative bound there)
    normal_x = np.abs(x) >= np.float32(2.0 ** -126)
    finite_hi = (hi & 0x7f80) != 0x7f80
    lo_ok = ((lo & 0x7f80) != 0) | (rest == 0)
    m = normal_x & finite_hi & lo_ok
    assert m.sum() > 900000
    x64 = x[m].astype(np.float64)
    s = _value(L, hi[m]).astype(np.float64) + _value(L, lo[m]).astype(np.float64)
    assert (np.abs(x64 - s) <= 2.0 ** -16 * np.abs(x64)).all()


def test_kswz_is_the_chunk_swizzle_bit(L):
    """1 for rows 4-11 of every 16: the rows of a ds_read_b128 lane group that read the neighbouring chunk."""
    assert [L.kswz_host(r) for r in range(32)] == [0] * 4 + [1] * 8 + [0] * 4 + [0] * 4 + [1] * 8 + [0] * 4
