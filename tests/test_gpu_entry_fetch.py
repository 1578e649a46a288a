"""One fetch for triangle lanes and entering lanes (rc_traverse_core.h, the record phase of phased_trace): the traversal copy of a TLAS
leaf carries the entry-cull sphere and the index of its instance (rc_device.h rc_pack_tlas_leaf) at the offset at which a ray inside an
instance finds a triangle.

* The copy holds the spheres after every path that changes one: rc_scene::inst_cull stays the source of truth, and dwords 0-4 of every
  TLAS leaf's record must be the first five words -- (c_w.xyz, A), B -- of its instance's entry there, bit for bit; dword 5 is the instance
  index, the same word as dword 13 (child1).
* Parity, bit for bit against the oracle and across the option settings, on batches that mix triangle lanes, entering lanes, culled
  entries that pop straight into the next TLAS leaf and exits that pop into one, with rays inside and outside the cull's regime.
"""

import numpy as np
import pytest

from gpu_kit import rc  # noqa: F401
from gpu_kit import read_device
from helpers import assert_hits_equal, build_oracle, build_product

pytestmark = pytest.mark.gpu

N_RAYS = 4096


# ---- 1. the traversal copy holds the spheres -------------------------------------------------------------------------------------------


def leaf_records_hold_the_spheres(t, n, what):
    """-> the spheres' words (n, 8), after checking every TLAS leaf record of the traversal copy against them."""
    cull = read_device(t.get_option("debug_inst_cull_ptr"), np.uint32, 8 * n).reshape(n, 8)
    base, off = t.get_option("debug_flat_nodes_ptr"), t.get_option("debug_flat_tlas_off")
    rec = read_device(base + 64 * off, np.uint32, 16 * (2 * n - 1)).reshape(2 * n - 1, 16)
    leaves = rec[n - 1:]                      # node n - 1 + j (1-based) is the leaf of sorted instance j
    inst = leaves[:, 13]
    assert np.array_equal(np.sort(inst), np.arange(n)), f"{what}: the leaves do not name every instance once"
    assert np.array_equal(leaves[:, 5], inst), f"{what}: dword 5 is not the instance index (dword 13)"
    bad = np.nonzero(np.any(leaves[:, :5] != cull[inst, :5], axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} leaf records do not hold their instance's sphere, first: leaf {bad[:3]} {leaves[bad[:3], :5]} != {cull[inst[bad[:3]], :5]}"
    assert np.all(leaves[:, 12] == 0xFFFFFFFF), f"{what}: a TLAS leaf's child0 word"
    return cull


def test_traversal_copy_holds_the_spheres(rc):
    import torch
    sc = rc.scenes
    n = 64
    soup = sc.random_triangles(12, 5, lo=-0.5, hi=0.5, edge=0.3)
    xf = [sc.lattice_transforms(4, 4, 4, 1.5 + 0.3 * f, 40 + f)[0] for f in range(6)]
    t = rc.TLAS()
    h = t.push_instances(t.add_geometry(soup), xf[0], np.arange(n, dtype=np.uint32))
    t.sync()
    seen = [leaf_records_hold_the_spheres(t, n, "sync")]

    def step(what):
        s.synchronize()
        seen.append(leaf_records_hold_the_spheres(t, n, what))
        assert seen[-1].tobytes() != seen[-2].tobytes(), f"{what}: the step was meant to move the spheres"

    s = torch.cuda.Stream()
    d_xf = torch.from_numpy(xf[1]).cuda()
    d_soup = torch.from_numpy(np.ascontiguousarray(soup * np.float32(1.4))).cuda()
    for buf in (d_xf, d_soup):
        buf.record_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        t.update_transforms_device(h, d_xf, stream=s.cuda_stream)
        t.refit_device_async(stream=s.cuda_stream)
    step("update + refit")
    for k, fused in ((2, 1), (3, 0)):
        t.set_option("tlas_rebuild_fused", fused)
        with torch.cuda.stream(s):
            d_xf.copy_(torch.from_numpy(xf[k]))
            t.update_transforms_device(h, d_xf, stream=s.cuda_stream)
            t.rebuild_device_async(stream=s.cuda_stream)
        step(f"update + rebuild (tlas_rebuild_fused = {fused})")
    with torch.cuda.stream(s):
        t.update_geometry_device_async(h, d_soup, stream=s.cuda_stream)  # a larger BLAS: every sphere's radius grows
        t.refit_device_async(stream=s.cuda_stream)
    step("geometry update + refit")
    t.wait_for_gpu()
    torch.cuda.synchronize()

    def frame(st):
        t.update_transforms_device(h, d_xf, stream=st)
        t.refit_device_async(stream=st)

    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        frame(torch.cuda.current_stream().cuda_stream)
    for k in (4, 5):
        with torch.cuda.stream(s):
            d_xf.copy_(torch.from_numpy(xf[k]))
            g.replay()
        step(f"graph replay of update + refit, frame {k}")
    del g
    t.set_option("release_captures", 1)
    t.update_transforms(h, xf[0])             # ... and the host path: upload, per-instance pass, refit
    assert t.sync().last_sync_action == "refit"
    step("host update + sync")


# ---- 2. parity on batches that mix the lane kinds ---------------------------------------------------------------------------------------
def lattice_cfg(sc, soup, dims, pitch, seed):
    xf, ids = sc.lattice_transforms(*dims, pitch, seed)[0], np.arange(int(np.prod(dims)), dtype=np.uint32)
    return {"blas": [(soup, None)], "instances": [(1, xf, ids)]}


def scene_cfg(sc, name):
    """Instances of radius <= 0.5 at pitch 0.8: neighbouring TLAS leaf boxes overlap, so a ray that leaves (or is spared) one instance
    pops the next TLAS leaf straight from its stack."""
    sphere = sc.fan_sphere(10, 6, radius=0.5)
    twelve = sc.random_triangles(12, 9, lo=-0.5, hi=0.5, edge=0.3)
    if name == "2":
        return lattice_cfg(sc, sphere, (2, 1, 1), 0.8, 21)
    if name == "64":
        return lattice_cfg(sc, sphere, (4, 4, 4), 0.8, 22)
    if name == "256":
        return lattice_cfg(sc, sphere, (8, 8, 4), 0.8, 23)
    if name == "300x12":                      # more than 256 instances: the TLAS's top is renumbered, kernel 6 stages it
        cfg = lattice_cfg(sc, twelve, (10, 6, 5), 0.8, 24)
        assert len(cfg["instances"][0][1]) == 300
        return cfg
    if name == "1":                           # the TLAS's root is a leaf
        return lattice_cfg(sc, sphere, (1, 1, 1), 0.8, 25)
    if name == "single-triangle":             # A = inf: never culled; next to instances that are
        cfg = lattice_cfg(sc, sphere, (3, 3, 1), 0.8, 26)
        one = sc.random_triangles(1, 3, lo=-0.3, hi=0.3, edge=0.6)
        xf1 = sc.lattice_transforms(3, 3, 2, 0.8, 27)[0]
        cfg["blas"].append((one, None))
        cfg["instances"].append((2, xf1, np.arange(100, 100 + len(xf1), dtype=np.uint32)))
        return cfg
    if name == "stacked":                     # every instance three times in the same place and more at half a pitch: exact ties, leaf after leaf
        xf = sc.lattice_transforms(3, 3, 2, 0.8, 28)[0]
        half = xf.copy()
        half[:, [3, 7, 11]] += np.float32(0.4)
        xf = np.concatenate([xf, xf, half, xf])
        return {"blas": [(sphere, None)], "instances": [(1, xf, np.arange(len(xf), dtype=np.uint32))]}
    raise KeyError(name)


SCENES = ["2", "64", "256", "300x12", "1", "single-triangle", "stacked"]


def mixed_rays(rc, cfg, seed):
    """N_RAYS rays through the scene's instances from inside and around it, a quarter of them with short or shifted segments, and every
    eighth outside the regime the cull's bounds assume: NaN / Inf components, |d|^2 outside [1e-2, 1e6], a zero direction."""
    sc = rc.scenes
    g = sc.rng(seed)
    centres = np.concatenate([np.asarray(xf, dtype=np.float64).reshape(-1, 3, 4)[:, :, 3] for _, xf, _ in cfg["instances"]])
    lo, hi = centres.min(axis=0) - 0.6, centres.max(axis=0) + 0.6
    org = g.uniform(lo - 0.5 * (hi - lo) - 1.0, hi + 0.5 * (hi - lo) + 1.0, size=(N_RAYS, 3))
    tgt = centres[g.integers(0, len(centres), N_RAYS)] + g.uniform(-0.7, 0.7, size=(N_RAYS, 3))
    rays = sc.make_rays(org, sc.normalize(tgt - org))
    k = np.arange(N_RAYS)
    rays["tmax"][k % 4 == 1] = g.uniform(0.0, 6.0, int(np.sum(k % 4 == 1))).astype(np.float32)
    rays["tmin"][k % 8 == 3] = g.uniform(-2.0, 4.0, int(np.sum(k % 8 == 3))).astype(np.float32)
    for r, f in ((0, 0.0999), (8, 0.1), (16, 1000.0), (24, 1001.0), (32, 1e-7), (40, 1e12)):
        rays["d"][k % 64 == r] *= np.float32(f)
    rays["d"][k % 64 == 48, 0] = np.nan
    rays["d"][k % 64 == 56, 1] = np.inf
    rays["o"][k % 128 == 4, 2] = np.nan
    rays["o"][k % 128 == 12, 0] = -np.inf
    rays["d"][k % 128 == 20] = 0.0
    rays["o"][k % 128 == 28] += np.float32(3e6)
    return rays


@pytest.mark.parametrize("name", SCENES)
def test_parity_on_mixed_lanes(rc, oracle, name):
    cfg = scene_cfg(rc.scenes, name)
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    rays = mixed_rays(rc, cfg, 700 + SCENES.index(name))
    want_c, want_a = o.trace(rays, nthreads=8), o.trace(rays, mode="any", nthreads=8)
    hit = float(want_c["hit"].mean())
    print(f"scene {name}: {len(o.instances)} instances, oracle hit fraction {hit:.3f}")
    assert 0.05 < hit < 0.95, hit
    first_c = first_a = None
    for cull in (1, 0, 2):
        t.set_option("entry_cull", cull)
        for kernel, s16 in ((5, 1), (5, 0), (6, 1), (6, 0), (3, 1)):
            t.set_option("kernel", kernel)
            t.set_option("stack16", s16)
            what = f"scene {name}, entry_cull {cull}, kernel {kernel}, stack16 {s16}"
            got_c, got_a = t.trace(rays), t.trace(rays, mode="any")
            assert_hits_equal(got_c, want_c, f"{what}: closest")
            assert_hits_equal(got_a, want_a, f"{what}: any")
            if first_c is None:
                first_c, first_a = got_c.tobytes(), got_a.tobytes()
            assert got_c.tobytes() == first_c, f"{what}: closest hits differ from the first setting's"
            assert got_a.tobytes() == first_a, f"{what}: any hits differ from the first setting's"
    if name == "64":  # the cull does spare entries on this batch (the counters of the stats kernel)
        t.set_option("entry_cull", 1); t.set_option("kernel", 5); t.set_option("stack16", 1); t.set_option("stats", 1)
        t.trace(rays)
        assert t.get_option("stat19") > 0
        t.set_option("stats", 0)
