"""The wavefront stage kernels and the fused shadow visibility on hostile scenes, bit for bit against the CPU oracle (the bounce against
tests/bounce_model.py): several geometries per scene -- triangle soups and meshes with and without uvs and per-vertex metadata words, in
mixed order, 1 to 1500 triangles -- under the fuzz's hostile instance transforms (mirrors, shears, singular, huge, tiny, zero), with
instance ids that are not the instance's position, rays as the fuzz aims them plus rays lying in a triangle's plane.  hit_frame picks the
primitive by the flat primitive id, the instance by its position and carries the normal through the transposed inverse: on one geometry
under rotations none of that can go wrong visibly; here it can.  Hit records come only from the product's own trace (asserted equal to the
oracle's): hits with NaN t and NaN normals included, never a made-up id.

Every output buffer is poisoned and has a poisoned guard behind it.  After the first pass the first geometry's instances are deleted, so
the flat primitive array and the attribute arrays are renumbered, and the frame and attribute stages run again against a fresh oracle scene.

test_scenes_cover_the_cases (no GPU needed) counts, from the oracle alone, what the module's scenes exercise."""
import functools

import numpy as np
import pytest

import bounce_model as bm
from gpu_kit import GUARD, POISON, dev, poisoned
from gpu_kit import rc  # noqa: F401
from helpers import assert_f32_bits_equal, assert_hits_equal, assert_rays_equal, build_oracle, build_product
from scene_kit import grid_mesh, hostile_transform, scenes_module

gpu = pytest.mark.gpu

BIASES = (1e-3, 0.0, -1e-3)
SEEDS = list(range(24))
FIXED = ["nan", "partial"]
N_VIS = 3997           # rays of the fixed scenes: the largest n of the fused visibility cases
OUTSIDE_LIGHT = np.array([6.0, 7.0, 5.0], np.float32)


# ---- scenes (numpy only) ----------------------------------------------------------------------------------------------------------
def mesh_geometry(nt, seed, variant):
    """The first nt faces of a bumpy grid mesh centred on the origin.  variant: "uv", "nouv" or "meta" (no uvs, one metadata word per vertex)."""
    v, f, nrm, uv = grid_mesh({1: 1, 2: 1, 17: 3, 200: 10, 1500: 28}[nt], seed=seed, with_uv=variant == "uv")
    fm = np.arange(500, 500 + len(v), dtype=np.uint32) if variant == "meta" else None
    return {"verts": v - np.float32(0.5), "faces": f[:nt].copy(), "normals": nrm, "uvs": uv, "face_meta": fm}


def triangles_of(geo):
    return geo["verts"][geo["faces"]] if isinstance(geo, dict) else np.asarray(geo[0], np.float32).reshape(-1, 3, 3)


def instance_group(g, blas_index, kinds, first_position):
    xf = np.stack([hostile_transform(g, k) for k in kinds])
    ids = (100 + 3 * (first_position + np.arange(len(kinds)))).astype(np.uint32)  # distinct, and never the instance's position
    return (blas_index, xf, ids)


def random_scene(seed):
    sc = scenes_module()
    g = np.random.default_rng(7000 + seed)
    n_geo = int(g.integers(2, 5))
    variants = ["soup", "uv", "nouv", "meta"]
    chosen = [variants[(seed + k) % 4] for k in range(n_geo)]  # over four consecutive seeds every variant comes first once
    g.shuffle(chosen[1:])
    blas, instances, kinds = [], [], []
    for b, variant in enumerate(chosen):
        nt = int(g.choice([1, 2, 17, 200, 1500]))
        if variant == "soup":
            verts = sc.random_triangles(nt, 90 * seed + b, lo=-0.5, hi=0.5, edge=float(g.choice([0.3, 1.0])))
            blas.append((verts, None if g.random() < 0.5 else g.integers(1, 1000, nt).astype(np.uint32)))
        else:
            blas.append(mesh_geometry(nt, 90 * seed + b, variant))
        ks = [int(g.choice([1, 2, 2, 3, 4, 5, 6])) if g.random() < 0.5 else 0 for _ in range(int(g.integers(1, 7)))]
        instances.append(instance_group(g, b + 1, ks, len(kinds)))
        kinds += ks
    return {"blas": blas, "instances": instances, "kinds": np.array(kinds), "n_rays": int(g.integers(2000, 4001)), "aim": None}


def nan_scene():
    """Always flattened (kind 3) and all-zero (kind 6) instances, several of them on one-triangle geometries -- a one-leaf tree has no box
    test in front of its triangle, so a ray whose local form is NaN gets through: hits with NaN t and NaN normals are certain -- and half
    of the rays aimed at the flattened ones."""
    sc = scenes_module()
    g = np.random.default_rng(7100)
    blas = [mesh_geometry(200, 1, "uv"), (sc.random_triangles(1, 2, lo=-0.5, hi=0.5, edge=1.0), None), mesh_geometry(1, 3, "meta"),
            (sc.random_triangles(200, 4, lo=-0.5, hi=0.5, edge=0.3), np.arange(1, 201, dtype=np.uint32))]
    instances, kinds = [], []
    for b, ks in enumerate(([3, 0, 6, 2], [3, 1, 3, 3, 6, 3], [3, 3, 2, 3, 6], [2, 3, 0, 1])):
        instances.append(instance_group(g, b + 1, ks, len(kinds)))
        kinds += ks
    kinds = np.array(kinds)
    aim = np.concatenate([xf[:, [3, 7, 11]] for _, xf, _ in instances])[kinds == 3]
    return {"blas": blas, "instances": instances, "kinds": kinds, "n_rays": N_VIS, "aim": aim}


def partial_scene():
    """300 small instances of two geometries, one of them a single triangle (see nan_scene): more than the 256 the LDS kernels take, so
    the drivers stage only the top of the TLAS."""
    sc = scenes_module()
    g = np.random.default_rng(7200)
    blas = [(sc.random_triangles(17, 5, lo=-0.5, hi=0.5, edge=0.3), np.arange(1, 18, dtype=np.uint32)), mesh_geometry(1, 6, "uv")]
    instances, kinds = [], []
    for b in range(2):
        ks = [3 if k % 5 == 0 else (k % 3) for k in range(150)]
        _, xf, ids = instance_group(g, b + 1, ks, len(kinds))
        small = np.array(ks) != 3
        xf[small] = (xf[small].reshape(-1, 3, 4) * np.array([0.4, 0.4, 0.4, 1.0], np.float32)).reshape(-1, 12)
        instances.append((b + 1, xf, ids))
        kinds += ks
    kinds = np.array(kinds)
    aim = np.concatenate([xf[:, [3, 7, 11]] for _, xf, _ in instances])[kinds == 3]
    return {"blas": blas, "instances": instances, "kinds": kinds, "n_rays": N_VIS, "aim": aim}


def scene_config(key):
    return nan_scene() if key == "nan" else partial_scene() if key == "partial" else random_scene(key)


def without_first_geometry(cfg):
    return {"blas": cfg["blas"][1:], "instances": [(b - 1, xf, ids) for b, xf, ids in cfg["instances"][1:]]}


def scene_rays(cfg, seed):
    """Rays as the fuzz aims them (half of them at cfg["aim"] when that is given), with some t ranges cut, plus 200 rays lying in the plane
    of a triangle of an instance, starting outside it and running across it."""
    sc = scenes_module()
    g = np.random.default_rng(7300 + seed)
    n = cfg["n_rays"] - 200
    org = g.uniform(-5, 5, size=(n, 3))
    tgt = g.uniform(-3.5, 3.5, size=(n, 3))
    if cfg["aim"] is not None:
        k = n // 2
        tgt[:k] = cfg["aim"][g.integers(0, len(cfg["aim"]), k)] + g.normal(size=(k, 3)) * 0.25
    xforms = np.concatenate([xf for _, xf, _ in cfg["instances"]]).astype(np.float64).reshape(-1, 3, 4)
    blas_of = np.concatenate([np.full(len(xf), b - 1) for b, xf, _ in cfg["instances"]])
    po, pd = np.zeros((200, 3)), np.zeros((200, 3))
    for j in range(200):
        i = int(g.integers(0, len(xforms)))
        tris = triangles_of(cfg["blas"][blas_of[i]])
        w = tris[int(g.integers(0, len(tris)))].astype(np.float64) @ xforms[i][:, :3].T + xforms[i][:, 3]
        along = g.normal() * (w[1] - w[0]) + g.normal() * (w[2] - w[0])
        length = np.linalg.norm(along)
        along = along / length if length > 0 else np.array([1.0, 0.0, 0.0])  # (a collapsed instance: any direction through the point)
        po[j], pd[j] = w.mean(axis=0) - along * g.uniform(0.5, 3.0), along
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = sc.make_rays(np.concatenate([org, po]), np.concatenate([d, pd]))
    rays["tmin"][::7] = g.uniform(-1, 1, len(rays["tmin"][::7]))
    rays["tmax"][::5] = g.uniform(0, 8, len(rays["tmax"][::5]))
    return rays


def gated_visibility(scene, rays, hits, lights, bias):
    """From the oracle alone -> (visible (n, L) bytes, the shadow rays' t_max (n, L), any_hit of the shadow rays (n, L)):
    visible = hit & (t_max > 0) & ~any_hit, the reference's test_shadow_rays! (`ray.t_max > 0 ? !any_hit : false`)."""
    lit = hits["hit"] == 1
    tmax, occluded = np.zeros((len(rays), len(lights)), np.float32), np.zeros((len(rays), len(lights)), bool)
    for l, light in enumerate(lights):
        sr = scene.shadow_rays(rays, hits, light, bias)
        tmax[:, l] = sr["tmax"]
        occluded[:, l] = scene.trace(sr, mode="any", nthreads=8)["hit"] == 1
    return (lit[:, None] & (tmax > 0) & ~occluded).astype(np.uint8), tmax, occluded


@functools.lru_cache(maxsize=None)
def oracle_side(key):
    """Everything a scene's tests expect, from the oracle alone: the scene, its rays, their hits and the three lights of the stage test --
    one outside, one inside the geometry (an instance's own origin), one that is bit for bit a shadow origin (bias 1e-3) of a hit slot, so
    that slot's distance to it is 0."""
    from oracle import pyoracle as po
    cfg = scene_config(key)
    o = build_oracle(po, cfg)
    rays = scene_rays(cfg, SEEDS[-1] + 1 + FIXED.index(key) if key in FIXED else key)
    hits = o.trace(rays, nthreads=8)
    origins = o.shadow_rays(rays, hits, OUTSIDE_LIGHT, BIASES[0])["o"]
    usable = np.nonzero((hits["hit"] == 1) & np.isfinite(origins).all(axis=1))[0]
    assert len(usable) > 0, f"scene {key}: no finite hit"
    on_surface = origins[usable[len(usable) // 2]].copy()
    inside = cfg["instances"][0][1][0][[3, 7, 11]].copy()
    return {"cfg": cfg, "o": o, "rays": rays, "hits": hits, "lights": np.stack([OUTSIDE_LIGHT, inside, on_surface]), "coincident": usable[len(usable) // 2]}


def coverage(key):
    """What one scene contributes to the conditions below."""
    s = oracle_side(key)
    cfg, o, rays, hits = s["cfg"], s["o"], s["rays"], s["hits"]
    lit = hits["hit"] == 1
    inst, prim = hits["instance_id"][lit], hits["primitive_id"][lit]
    xf = np.concatenate([x for _, x, _ in cfg["instances"]]).astype(np.float64).reshape(-1, 3, 4)
    det = np.linalg.det(xf[:, :, :3])
    first_blas = len(triangles_of(cfg["blas"][0]))  # (no degenerate face in these geometries: every triangle is a primitive)
    tri = o.blas_prims["v"][prim].astype(np.float64)
    inv = o.instances["inv_transform"][inst].astype(np.float64).reshape(-1, 3, 4)[:, :, :3]
    with np.errstate(invalid="ignore", over="ignore"):
        nw = np.einsum("hji,hj->hi", inv, np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]))
        facing = np.einsum("hi,hi->h", nw, rays["d"][lit].astype(np.float64))
    visible, tmax, occluded = gated_visibility(o, rays, hits, s["lights"], BIASES[0])
    return {"hits": int(lit.sum()), "later_blas": int((prim >= first_blas).sum()), "negative_det": int((det[inst] < 0).sum()),
            "kind2": int((cfg["kinds"][inst] == 2).sum()), "nan_t": int(np.isnan(hits["t"][lit]).sum()),
            "flipped": int((facing > 0).sum()), "not_flipped": int((facing < 0).sum()),
            "seen": visible.sum(axis=0).astype(np.int64), "shadowed": (lit[:, None] & occluded).sum(axis=0).astype(np.int64)}


def test_scenes_cover_the_cases():
    """The conditions that keep this module honest, over all its scenes, from the oracle alone."""
    total = {}
    for key in SEEDS + FIXED:
        for name, value in coverage(key).items():
            total[name] = total.get(name, 0) + value
    print(total)
    assert total["hits"] >= 20_000 and total["later_blas"] >= 5_000 and total["negative_det"] >= 500 and total["kind2"] >= 2_000, total
    assert total["nan_t"] >= 100 and total["flipped"] >= 100 and total["not_flipped"] >= 100, total
    assert np.all(total["seen"] >= 100) and np.all(total["shadowed"] >= 100), total
    for key in FIXED:
        kinds = oracle_side(key)["cfg"]["kinds"]
        assert 3 in kinds and (key != "nan" or 6 in kinds)
    assert len(oracle_side("partial")["cfg"]["kinds"]) >= 294


# ---- device buffers ---------------------------------------------------------------------------------------------------------------


def fetch(buf, nbytes, dtype, what):
    """The first nbytes of a poisoned buffer as `dtype`, after checking that nothing behind them was written."""
    import torch
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    assert len(raw) == nbytes + GUARD and np.all(raw[nbytes:] == POISON), f"{what}: bytes behind the output were written"
    return raw[:nbytes].view(dtype)


# ---- 3. every stage kernel -------------------------------------------------------------------------------------------------------------
def product_hits(t, rays, want, what):
    """The product's own hit records of `rays` (default dispatch), equal to the oracle's in kernels -1 and 3."""
    for kernel in (3, -1):
        t.set_option("kernel", kernel)
        got = t.trace(rays)
        assert_hits_equal(got, want, f"{what} closest, kernel {kernel}")
    return got


def check_frames_and_attributes(t, o, rays, hits, d_r, d_h, light, what):
    n = len(rays)
    r, h = d_r.data_ptr(), d_h.data_ptr()
    d_p, d_n = poisoned(n * 12), poisoned(n * 12)
    t.hit_points_device(r, h, n, d_p.data_ptr(), d_n.data_ptr())
    want_p, want_n = o.hit_points(rays, hits)
    assert_f32_bits_equal(fetch(d_p, n * 12, np.float32, what).reshape(n, 3), want_p, f"{what} hit points")
    assert_f32_bits_equal(fetch(d_n, n * 12, np.float32, what).reshape(n, 3), want_n, f"{what} normals")
    d_p = poisoned(n * 12)
    t.hit_points_device(r, h, n, d_p.data_ptr())  # without normals
    assert_f32_bits_equal(fetch(d_p, n * 12, np.float32, what).reshape(n, 3), want_p, f"{what} hit points alone")
    d_sn, d_uv = poisoned(n * 12), poisoned(n * 8)
    t.shading_attributes_device(h, n, d_sn.data_ptr(), d_uv.data_ptr())
    want_sn, want_uv = o.shading_attributes(hits)
    assert_f32_bits_equal(fetch(d_sn, n * 12, np.float32, what).reshape(n, 3), want_sn, f"{what} shading normals")
    assert_f32_bits_equal(fetch(d_uv, n * 8, np.float32, what).reshape(n, 2), want_uv, f"{what} uvs")
    for bias in BIASES:
        d_o = poisoned(n * 32)
        t.reflection_rays_device(r, h, n, d_o.data_ptr(), bias=bias)
        assert_rays_equal(fetch(d_o, n * 32, bm.RAY_DT, what), o.reflection_rays(rays, hits, bias), f"{what} reflection rays, bias {bias}")
        d_o = poisoned(n * 32)
        t.shadow_rays_device(r, h, n, light, d_o.data_ptr(), bias=bias)
        assert_rays_equal(fetch(d_o, n * 32, bm.RAY_DT, what), o.shadow_rays(rays, hits, light, bias), f"{what} shadow rays, bias {bias}")


@gpu
@pytest.mark.parametrize("key", SEEDS + FIXED)
def test_every_stage_on_a_hostile_scene(rc, oracle, key):
    import torch
    s = oracle_side(key)
    cfg, o, rays, lights = s["cfg"], s["o"], s["rays"], s["lights"]
    n = len(rays)
    t = build_product(rc, cfg)
    try:
        assert t.adapt().all_blas_prims.tobytes() == o.blas_prims.tobytes()
        hits = product_hits(t, rays, s["hits"], f"scene {key}")
        d_r, d_h = dev(rays), dev(hits)
        r, h = d_r.data_ptr(), d_h.data_ptr()
        check_frames_and_attributes(t, o, rays, hits, d_r, d_h, lights[0], f"scene {key}")
        # the light inside the geometry, and the one a shadow ray starts on: distance 0, direction 0 / 0
        for l in (1, 2):
            for bias in BIASES:
                d_o = poisoned(n * 32)
                t.shadow_rays_device(r, h, n, lights[l], d_o.data_ptr(), bias=bias)
                got = fetch(d_o, n * 32, bm.RAY_DT, f"scene {key}")
                assert_rays_equal(got, o.shadow_rays(rays, hits, lights[l], bias), f"scene {key} shadow rays, light {l}, bias {bias}")
                if l == 2 and bias == BIASES[0]:
                    assert got["tmax"][s["coincident"]] == 0 and np.isnan(got["d"][s["coincident"]]).all()
        # diffuse bounce: slot-aligned, and through the compacted queue
        idx = np.nonzero(hits["hit"])[0]
        d_idx, d_cnt = poisoned(n * 4), poisoned(4)
        t.compact_hits_device(h, n, d_idx.data_ptr(), d_cnt.data_ptr())
        count = int(fetch(d_cnt, 4, np.uint32, f"scene {key}")[0])
        assert count == len(idx) and np.array_equal(fetch(d_idx, n * 4, np.uint32, f"scene {key}")[:count], idx)
        for k, bias in enumerate(BIASES):
            seed, bounce = 0x5EED0000 + 17 * k, k
            d_o, d_path = poisoned(n * 32), poisoned(n * 4)
            t.bounce_rays_device(r, h, n, d_o.data_ptr(), seed=seed, bounce=bounce, bias=bias, d_path_out=d_path.data_ptr())
            want, want_path = bm.bounce_rays(o, rays, hits, n, seed=seed, bounce=bounce, bias=bias)
            assert_rays_equal(fetch(d_o, n * 32, bm.RAY_DT, f"scene {key}"), want, f"scene {key} bounce, bias {bias}")
            assert np.array_equal(fetch(d_path, n * 4, np.uint32, f"scene {key}"), want_path)
            d_o, d_path = poisoned(n * 32), poisoned(n * 4)
            t.bounce_rays_device(r, h, n, d_o.data_ptr(), seed=seed, bounce=bounce, bias=bias, d_src=d_idx.data_ptr(), d_src_count=d_cnt.data_ptr(),
                                 d_path_out=d_path.data_ptr())
            want, want_path = bm.bounce_rays(o, rays, hits, n, seed=seed, bounce=bounce, bias=bias, src=idx, count=count)
            assert_rays_equal(fetch(d_o, n * 32, bm.RAY_DT, f"scene {key}"), want, f"scene {key} compacted bounce, bias {bias}")
            assert np.array_equal(fetch(d_path, n * 4, np.uint32, f"scene {key}"), want_path)
        # the first geometry goes: the flat primitive array and the attribute arrays are renumbered
        assert t.delete(t.handles[0])
        t.sync()
        o2 = build_oracle(oracle, without_first_geometry(cfg))
        assert t.adapt().all_blas_prims.tobytes() == o2.blas_prims.tobytes(), "the flat primitive array after the deletion"
        hits2 = product_hits(t, rays, o2.trace(rays, nthreads=8), f"scene {key} after the deletion")
        d_h2 = dev(hits2)
        check_frames_and_attributes(t, o2, rays, hits2, d_r, d_h2, lights[0], f"scene {key} after the deletion")
        torch.cuda.synchronize()
        t.wait_for_gpu()
    finally:
        t.free()


# ---- 4. fused shadow visibility and the t_max gate ------------------------------------------------------------------------------------
VIS_BIAS = BIASES[0]
N_LIGHTS = (1, 2, 3, 5, 7, 33)
N_ITEMS = (1, 63, 65, N_VIS)


class VisibilityWorld:
    def __init__(self, rc, key, kernel=None):
        s = oracle_side(key)
        self.o, self.rays = s["o"], s["rays"]
        assert len(self.rays) == N_VIS
        g = np.random.default_rng(7400)
        self.lights = np.concatenate([s["lights"], g.uniform(-6, 6, size=(max(N_LIGHTS) - 3, 3)).astype(np.float32)])
        self.t = build_product(rc, s["cfg"])
        self.hits = product_hits(self.t, self.rays, s["hits"], f"scene {key}")
        if kernel is not None:
            self.t.set_option("kernel", kernel)
        self.visible, tmax, occluded = gated_visibility(self.o, self.rays, self.hits, self.lights, VIS_BIAS)
        lit = (self.hits["hit"] == 1)[:, None]
        self.gated = lit & ~(tmax > 0)
        self.ungated_differs = self.gated & ~occluded          # what hit & ~any_hit alone would light
        # with ONE light already the scene proves something: gated items, and items on which the ungated formula is wrong
        assert self.gated[:, 0].sum() >= 100 and self.ungated_differs[:, 0].sum() >= 50, (key, self.gated[:, 0].sum(), self.ungated_differs[:, 0].sum())
        assert self.gated[s["coincident"], 2] and tmax[s["coincident"], 2] == 0  # the light on a shadow origin: t_max = 0, not NaN
        self.d_rays, self.d_hits = dev(self.rays), dev(self.hits)
        self.composed = {}

    def composed_visibility(self, cull):
        """(b): the same formula from the product's own shadow_rays_device + trace_device(mode="any"), under the current entry_cull."""
        if cull not in self.composed:
            n, t = N_VIS, self.t
            out = np.zeros((n, len(self.lights)), np.uint8)
            for l, light in enumerate(self.lights):
                d_sr, d_sh = poisoned(n * 32), poisoned(n * 32)
                t.shadow_rays_device(self.d_rays.data_ptr(), self.d_hits.data_ptr(), n, light, d_sr.data_ptr(), bias=VIS_BIAS)
                t.trace_device(d_sr.data_ptr(), d_sh.data_ptr(), n, mode="any")
                sr, sh = fetch(d_sr, n * 32, bm.RAY_DT, "shadow rays"), fetch(d_sh, n * 32, bm.HIT_DT, "shadow hits")
                out[:, l] = (self.hits["hit"] == 1) & (sr["tmax"] > 0) & (sh["hit"] == 0)
            self.composed[cull] = out
        return self.composed[cull]


@pytest.fixture(scope="module")
def worlds(rc):
    w = {"lds": VisibilityWorld(rc, "nan"), "partial": VisibilityWorld(rc, "partial"), "plain": VisibilityWorld(rc, "nan", kernel=3)}
    assert w["lds"].t.n_instances() <= 256 and w["partial"].t.n_instances() >= 294 and w["partial"].t.get_option("tlas_top_k") > 0
    yield w
    for x in w.values():
        x.t.free()


@gpu
@pytest.mark.parametrize("shape", ["lds", "partial", "plain"])
@pytest.mark.parametrize("n_lights", N_LIGHTS)
@pytest.mark.parametrize("n", N_ITEMS)
def test_fused_visibility_applies_the_t_max_gate(worlds, shape, n_lights, n):
    import torch
    w = worlds[shape]
    t = w.t
    d_l = torch.from_numpy(np.ascontiguousarray(w.lights[:n_lights])).cuda()
    before = t.get_option("entry_cull")
    try:
        for cull in (before, 2):
            t.set_option("entry_cull", cull)
            composed = w.composed_visibility(cull)
            out = poisoned(n * n_lights)
            t.shadow_visibility_device(w.d_rays.data_ptr(), w.d_hits.data_ptr(), n, d_l.data_ptr(), n_lights, out.data_ptr(), bias=VIS_BIAS)
            got = fetch(out, n * n_lights, np.uint8, f"{shape} n={n} L={n_lights}").reshape(n, n_lights)
            t.wait_for_gpu()
            for want, name in ((w.visible, "the oracle"), (composed, "the composed path")):
                bad = np.nonzero(got != want[:n, :n_lights])
                on_gated = int(w.gated[:n, :n_lights][bad].sum())
                assert len(bad[0]) == 0, (f"{shape} n={n} L={n_lights} entry_cull={cull} against {name}: {len(bad[0])} bytes differ ({on_gated} of them on the "
                                          f"{int(w.gated[:n, :n_lights].sum())} gated items), first (slot, light) {list(zip(bad[0][:5], bad[1][:5]))}")
            assert set(np.unique(got)) <= {0, 1}
    finally:
        t.set_option("entry_cull", before)


# ---- 5. compaction at the scan's block boundaries ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 65_535, 65_537])
def test_compaction_at_scan_boundaries(worlds, n):
    """compact_hits_device reads the hit flag of a record and nothing else: the records here carry a flag and zeros."""
    t = worlds["lds"].t
    g = np.random.default_rng(n)
    for name, flags in (("none", np.zeros(n, bool)), ("all", np.ones(n, bool)), ("alternating", np.arange(n) % 2 == 1), ("random", g.random(n) < 0.37)):
        hits = np.zeros(n, bm.HIT_DT)
        hits["hit"] = flags
        d_h, d_idx, d_cnt = dev(hits), poisoned(n * 4), poisoned(4)
        t.compact_hits_device(d_h.data_ptr(), n, d_idx.data_ptr(), d_cnt.data_ptr())
        count = int(fetch(d_cnt, 4, np.uint32, f"n={n} {name}")[0])
        idx = fetch(d_idx, n * 4, np.uint32, f"n={n} {name}")
        want = np.nonzero(flags)[0]
        assert count == len(want), f"n={n} {name}: count {count}, want {len(want)}"
        assert np.array_equal(idx[:count], want), f"n={n} {name}: indices"
        assert np.all(idx[count:].view(np.uint8) == POISON), f"n={n} {name}: indices behind the count were written"
