"""Shared test helpers: build the same scene in the product (C ABI) and in the CPU oracle."""
import numpy as np


def build_product(rc, cfg, device=0):
    """cfg["blas"]: (verts, meta) triangle soups, or dicts of add_mesh's arguments (verts, faces, normals, uvs, face_meta) for meshes.
    The handles of cfg["instances"]' groups are left in `t.handles`, in order."""
    t = rc.TLAS(device)
    for geo in cfg["blas"]:
        if isinstance(geo, dict):
            t.add_mesh(geo["verts"], geo["faces"], geo["normals"], geo.get("uvs"), geo.get("face_meta"))
        else:
            t.add_geometry(*geo)
    t.handles = [t.push_instances(b, xf, ids) for b, xf, ids in cfg["instances"]]
    return t.sync()


def build_oracle(po, cfg):
    s = po.Scene()
    for geo in cfg["blas"]:
        if isinstance(geo, dict):
            s.add_mesh(geo["verts"], geo["faces"], geo["normals"], geo.get("uvs"), geo.get("face_meta"))
        else:
            s.add_blas(*geo)
    for b, xf, ids in cfg["instances"]:
        for x, i in zip(xf, ids):
            s.add_instance(b, x, int(i))
    return s.build()


def assert_hits_equal(got, want, what=""):
    """Bit-exact comparison of RTHitResult arrays: ids exact, t/u/v identical bit patterns (NaN payloads aside)."""
    assert len(got) == len(want)
    for f in ("hit", "primitive_id", "instance_id", "instance_custom_index"):
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, f"{what}: {len(bad)} rays differ in {f}, first {bad[:5]}: got {got[f][bad[:5]]} want {want[f][bad[:5]]}"
    for f in ("t", "bary_u", "bary_v"):
        a, b = got[f].view(np.uint32), want[f].view(np.uint32)
        # a NaN must be a NaN on both sides; its sign / payload bits are the hardware's (x86 generates 0xFFC00000 for 0*inf,
        # gfx950 0x7FC00000), not the algorithm's
        bad = np.nonzero((a != b) & ~(np.isnan(got[f]) & np.isnan(want[f])))[0]
        assert len(bad) == 0, f"{what}: {len(bad)} rays differ in {f} bits, first {bad[:5]}: got {got[f][bad[:5]]} want {want[f][bad[:5]]}"


def assert_f32_bits_equal(got, want, what=""):
    """Bit-exact comparison of two float32 arrays of one shape, by the rule of assert_hits_equal: identical bit patterns, except that a
    NaN on both sides matches whatever its sign or payload.  Rows are counted along the first axis."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    diff = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    bad = np.nonzero(diff.reshape(len(got), -1).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} entries differ in their bits, first {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"


def assert_rays_equal(got, want, what=""):
    """Bit-exact comparison of RTRay arrays (o, t_min, d, t_max: 8 float32 words per ray), NaN payloads aside."""
    assert len(got) == len(want), f"{what}: {len(got)} rays != {len(want)}"
    assert got.dtype.itemsize == 32 and want.dtype.itemsize == 32
    a, b = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 8), np.ascontiguousarray(want).view(np.uint32).reshape(-1, 8)
    fa, fb = a.view(np.float32), b.view(np.float32)
    bad = np.nonzero(((a != b) & ~(np.isnan(fa) & np.isnan(fb))).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(a)} rays differ in their bits, first {bad[:5]}: got {fa[bad[:3]]} want {fb[bad[:3]]}"


def random_rays(rc, n, seed, lo, hi):
    g = rc.scenes.rng(seed)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    o = g.uniform(lo - 0.5 * (hi - lo), hi + 0.5 * (hi - lo), size=(n, 3))
    target = g.uniform(lo, hi, size=(n, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return rc.scenes.make_rays(o, d)
