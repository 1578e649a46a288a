"""The scene's per-stream pools past their size (rc_stream_slot, raycore.jl_amd/csrc/rc_stream_slots.h; tests/test_stream_slots.py holds the
rule itself on the host): more streams on one scene than it has stack spill regions (8) or totals scratch areas (16).  Round-robin over
the streams every launch misses its stream's entry and takes over another stream's -- an idle one, else after waiting for the oldest -- so
no launch may ever write through an area another launch in flight still uses: results must equal the single-stream ones exactly.

The scene is the deep chain of test_gpu_stress.py::test_overlapping_launches_on_two_streams, whose traversal stacks run through the spill
path.  Each eager spill region is sized for the largest grid any option can ask for (about 268 MB on a 256-CU device), so the first case
holds about 2 GB of device memory while the scene lives."""
import numpy as np
import pytest

from gpu_kit import rc  # noqa: F401

pytestmark = pytest.mark.gpu

N_RAYS = 8192


def chain(levels, fat=0.3):
    tris = []
    for j in range(1, levels + 1):
        for axis in range(3):
            size = 2.0 ** (-j + 1)
            p = np.full(3, fat * size); p[axis] = size
            q = p.copy(); q[(axis + 1) % 3] += 0.5 * size * fat
            r = np.full(3, -1e-4 * (1 + 0.5 * j))
            tris.append(np.concatenate([r, p, q]))
    return np.array(tris, dtype=np.float32)


@pytest.fixture(scope="module")
def scene(rc):
    sc = rc.scenes
    xf = np.tile(sc.IDENTITY3x4, (4, 1)).astype(np.float32)
    xf[1, [0, 5, 10]] = 0.5
    xf[2, [0, 5, 10]] = 0.25
    xf[3, [3, 7, 11]] = [0.01, 0.0, 0.0]
    t = rc.TLAS()
    t.push(chain(10), xf, instance_ids=np.arange(4, dtype=np.uint32))
    t.sync()
    yield t
    t.free()


@pytest.fixture(scope="module")
def batches(rc, scene):
    """Ten batches of rays with their serial results (host-buffer trace, default options), computed once."""
    sc = rc.scenes
    g = sc.rng(33)
    out = []
    for k in range(10):
        rays = sc.make_rays(g.uniform(-0.2, 0.0, size=(N_RAYS, 3)), sc.normalize(g.uniform(0.05, 1.0, size=(N_RAYS, 3))))
        out.append((rays, scene.trace(rays)))
    assert all(int(h["hit"].sum()) > 0 for _, h in out)
    return out


@pytest.mark.parametrize("kernel", [3, -1])
def test_ten_streams_share_eight_spill_regions(rc, scene, batches, kernel):
    import torch
    streams = [torch.cuda.Stream() for _ in batches]
    d_rays = [torch.from_numpy(r.view(np.uint8).reshape(-1)).cuda() for r, _ in batches]
    d_hits = [torch.zeros(N_RAYS * 32, dtype=torch.uint8, device="cuda") for _ in batches]
    torch.cuda.synchronize()
    scene.set_option("kernel", kernel)
    try:
        for rep in range(3):
            for k, st in enumerate(streams):
                scene.trace_device(d_rays[k].data_ptr(), d_hits[k].data_ptr(), N_RAYS, stream=st.cuda_stream)
        torch.cuda.synchronize()
    finally:
        scene.set_option("kernel", -1)
    for k, (_, want) in enumerate(batches):
        got = d_hits[k].cpu().numpy().view(rc.HIT_DT)
        assert got.tobytes() == want.tobytes(), f"stream {k}"


def test_eighteen_streams_share_sixteen_totals_areas(rc, scene):
    import torch
    from raycore_jl_amd._capi import check, lib, ptr
    n, rpt, seed = scene.n_primitives(), 64, 19

    def totals(vec, stream):
        check(lib().rc_view_factor_totals_device(scene._h, rpt, seed, 0, n, 0, rpt, ptr(vec.data_ptr()), ptr(vec.data_ptr() + 8 * n), ptr(stream.cuda_stream)))

    single = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    st0 = torch.cuda.Stream()
    torch.cuda.synchronize()
    totals(single, st0)
    st0.synchronize()
    want = single.cpu().numpy().view(np.uint64)
    assert int(want[:n].sum()) > 0 and int(want[n:].sum()) > 0
    streams = [torch.cuda.Stream() for _ in range(18)]
    vecs = [torch.zeros(2 * n, dtype=torch.int64, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for rep in range(2):
        for v, st in zip(vecs, streams):
            totals(v, st)
    torch.cuda.synchronize()
    for k, v in enumerate(vecs):
        assert np.array_equal(v.cpu().numpy().view(np.uint64), 2 * want), f"stream {k}"


def test_pools_leave_counters_and_status_clean(scene):
    """After the two cases above (this module's scene): every claim counter is back at zero and no launch reported a stack overflow."""
    assert scene.get_option("claim_drift") == 0
    scene.wait_for_gpu()  # raises if the sticky status word was set
