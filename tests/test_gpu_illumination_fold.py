"""rc_get_illumination_device ACCUMULATES into the caller's f32 vector with the reference's arithmetic -- `counts[k] += 1f0` once per hit
(src/kernels.jl:119-121) --, also onto a vector that is not zero.  The suite only ever hands the call zeros; this pins the fold onto
whatever a caller left there: integer counts clamp at 2^24, where f32 stops moving under + 1; a word that is not a count (a fraction, a
negative, something beyond 2^24, inf) follows the same one-by-one sum; NaN stays NaN.

The scene: 9 triangles, one per cell of a 3 x 3 board, so the histogram's last row of eight is partial (n8 = 2); a 16 x 16 grid from a
direction in which, by the CPU oracle, every triangle takes at least one ray.  The expected vector is that sum in numpy float32, with
the oracle's hit counts, compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

from gpu_kit import rc  # noqa: F401
from helpers import build_oracle, build_product

pytestmark = pytest.mark.gpu

VIEWDIR = np.array([0.1, 0.2, -1.0], dtype=np.float32)
GRID = 16
PREFILL = np.array([0, 5, 16777215, 16777216, 0.5, -3, 3e7, np.inf, np.nan], dtype=np.float32)
DISTINCT = np.arange(1, 10, dtype=np.uint32)
REPEATING = np.array([3, 3, 7, 0, 12, 7, 1, 9, 3], dtype=np.uint32)  # 0 and 12 are outside 1..9: dropped; slots 2, 4, 5, 6, 8 take nothing


def board():
    """Nine triangles in the plane z = 0, triangle k in the unit cell (k % 3, k // 3)."""
    tris = [[(x + 0.05, y + 0.05, 0.0), (x + 0.95, y + 0.05, 0.0), (x + 0.05, y + 0.95, 0.0)] for y in range(3) for x in range(3)]
    return np.ascontiguousarray(np.array(tris, dtype=np.float32).reshape(9, 9))


def reference_sum(start, hits):
    """counts[k] += 1f0, hits[k] times, in float32; a value that no longer moves ends its slot early (it would not move again)."""
    out = start.copy()
    for k, n in enumerate(hits):
        for _ in range(int(n)):
            nv = np.float32(out[k] + np.float32(1.0))
            if nv == out[k]:
                break
            out[k] = nv
    return out


@pytest.mark.parametrize("meta", [DISTINCT, REPEATING], ids=["distinct", "repeating"])
def test_fold_onto_a_vector_that_is_not_zero(rc, oracle, meta):
    import torch
    sc = rc.scenes
    cfg = {"blas": [(board(), meta)], "instances": [(1, sc.IDENTITY3x4[None], np.zeros(1, np.uint32))]}
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    n = t.n_primitives()
    assert n == 9
    hits = o.get_illumination(VIEWDIR, GRID, nthreads=8)
    assert hits.dtype == np.float32 and len(hits) == n
    trace = o.trace(o.ray_grid(VIEWDIR, GRID), nthreads=8)
    per_triangle = np.bincount(trace["primitive_id"][trace["hit"] == 1], minlength=n)  # (in the order of the built primitives)
    assert (per_triangle >= 1).all(), per_triangle  # every triangle takes a ray ...
    if meta is DISTINCT:
        assert (hits >= 1).all() and hits.sum() == per_triangle.sum()
    else:  # ... and the rays of the two dropped triangles are counted nowhere
        dropped = per_triangle[(o.blas_prims["meta"] == 0) | (o.blas_prims["meta"] == 12)]
        assert len(dropped) == 2 and hits.sum() == per_triangle.sum() - dropped.sum() and hits[[1, 3, 4, 5, 7]].sum() == 0

    d_counts = torch.from_numpy(PREFILL.copy()).cuda()
    want = PREFILL.copy()
    with np.errstate(invalid="ignore"):
        for call in (1, 2):  # the second call accumulates onto the first one's result
            status = rc.lib().rc_get_illumination_device(t._h, VIEWDIR.ctypes.data_as(C.c_void_p), GRID, 0, GRID * GRID, C.c_void_p(d_counts.data_ptr()), None)
            assert status == 0, rc.lib().rc_last_error().decode()
            t.wait_for_gpu()
            torch.cuda.synchronize()
            want = reference_sum(want, hits)
            got = d_counts.cpu().numpy()
            print(f"call {call}: got {got} ({[hex(x) for x in got.view(np.uint32)]}), want {want}")
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (call, got, want)
    t.free()
