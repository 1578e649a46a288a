"""What the GPU tests share: the `rc` fixture, uploads, guarded output buffers and the word-for-word comparison.  Imported only by GPU
tests (and by tests/test_helpers_comparators.py, which runs the buffer helpers on the CPU); torch is imported where it is used."""
import ctypes

import numpy as np
import pytest

POISON = 0xAB
POISON_U32 = 0xABABABAB  # the same fill, for outputs that are compared as u32 words
GUARD = 256              # poisoned bytes behind every output: nothing may be written past it


@pytest.fixture(scope="module")
def rc():
    import raycore_jl_amd
    assert raycore_jl_amd.device_count() > 0, "no GPU visible: the product has no CPU fallback"
    return raycore_jl_amd


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def f32_tensor(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def dev_u32(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.uint32).view(np.int32)).cuda()


def dev_u64(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def u32_of(t):
    return t.cpu().numpy().view(np.uint32)


def u64_of(t):
    return t.cpu().numpy().view(np.uint64)


def read_device(ptr, dtype, count):
    out = np.zeros(count, dtype=dtype)
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(int(ptr)), out.nbytes, 2) == 0
    return out


def poisoned(nbytes, device="cuda"):
    import torch
    return torch.full((nbytes + GUARD,), POISON, dtype=torch.uint8, device=device)


def zeroed(n, width, device="cuda"):
    """n zeroed words of `width` bytes followed by the poisoned guard (the call accumulates: the caller zeroes)."""
    out = poisoned(n * width, device)
    out[:n * width] = 0
    return out


def words_of(out, n, dtype):
    """The first n words of a guarded buffer, after checking the guard behind them."""
    got = out.cpu().numpy()
    width = np.dtype(dtype).itemsize
    assert np.all(got[n * width:] == POISON), "bytes behind an output were written"
    return got[:n * width].view(dtype)


def check_words(out, want, dtype, what):
    """`out`: a guarded buffer; `want`: the expected words, any shape.  Every word is compared, after the guard."""
    flat = np.asarray(want, dtype).reshape(-1)
    got = words_of(out, flat.size, dtype)
    bad = np.nonzero(got != flat)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {flat.size} items differ, first items {bad[:8]}: got {got[bad[:8]]} want {flat[bad[:8]]}"


def finish(t):
    import torch
    torch.cuda.synchronize()
    t.wait_for_gpu()  # (a stack overflow would be reported here)
