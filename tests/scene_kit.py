"""Scenes, rays and input vectors that more than one test file uses.  CPU-importable: numpy only, no torch; the product module is
always passed in (`rc`), never imported here."""
import numpy as np


def room_cfg(rc, meta=None):
    sc = rc.scenes
    verts = np.concatenate([sc.fan_sphere(12, 7, centre=(0, 0, 0), radius=0.5), sc.box_room((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5), 2)])
    n = len(verts)
    m = np.arange(1, n + 1, dtype=np.uint32) if meta is None else meta(n)
    return {"blas": [(verts, m)], "instances": [(1, sc.IDENTITY3x4[None], np.zeros(1, np.uint32))]}


def grid_mesh(n, seed=0, with_uv=True):
    """(n+1)^2 vertex grid over [0,1]^2 with a bumpy z, 2 n^2 faces, analytic-ish normals."""
    g = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.linspace(0, 1, n + 1), np.linspace(0, 1, n + 1), indexing="ij")
    z = 0.1 * np.sin(6 * xs) * np.cos(5 * ys)
    verts = np.stack([xs, ys, z], -1).reshape(-1, 3).astype(np.float32)
    nrm = g.normal(size=verts.shape).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    uv = np.stack([xs, ys], -1).reshape(-1, 2).astype(np.float32) if with_uv else None
    idx = lambda i, j: i * (n + 1) + j
    faces = []
    for i in range(n):
        for j in range(n):
            faces += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    return verts, np.array(faces, np.uint32), nrm, uv


def hostile_transform(g, kind):
    m = np.eye(4, dtype=np.float64)
    a = g.normal(size=(3, 3))
    q, _ = np.linalg.qr(a)
    if kind == 0:      # rotation + uniform scale + translation
        m[:3, :3] = q * g.uniform(0.3, 2.0)
    elif kind == 1:    # mirror
        m[:3, :3] = q @ np.diag([-1.0, 1.0, 1.0])
    elif kind == 2:    # shear + anisotropic scale
        m[:3, :3] = q @ np.diag(g.uniform(0.05, 5.0, 3)) + np.triu(g.normal(size=(3, 3)) * 0.5, 1)
    elif kind == 3:    # flattened along one axis: singular, inverse = Inf / NaN
        m[:3, :3] = q @ np.diag([1.0, 1.0, 0.0])
    elif kind == 4:    # huge
        m[:3, :3] = q * 1e6
    elif kind == 5:    # tiny
        m[:3, :3] = q * 1e-6
    else:              # all-zero linear part
        m[:3, :3] = 0.0
    m[:3, 3] = g.uniform(-3, 3, 3)
    return m.astype(np.float32)[:3, :].reshape(12)


def scenes_module():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raycore.jl_amd", "scenes.py")
    spec = importlib.util.spec_from_file_location("rc_scenes_only", path)   # scene generators only: no HIP library needed
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def cube():
    p = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)        # 8 corners, index = 4x + 2y + z
    quads = [(0, 1, 3, 2, (-1, 0, 0)), (4, 6, 7, 5, (1, 0, 0)), (0, 4, 5, 1, (0, -1, 0)), (2, 3, 7, 6, (0, 1, 0)), (0, 2, 6, 4, (0, 0, -1)), (1, 5, 7, 3, (0, 0, 1))]
    pf, nf, normals = [], [], []
    for k, (a, b, c, d, n) in enumerate(quads):
        normals.append(n)
        pf += [(a, b, c), (a, c, d)]
        nf += [(k, k, k), (k, k, k)]
    return p, np.array(pf), np.array(normals, np.float32), np.array(nf)


MID_STACK, LDS_STACK = 16, 24  # kMidStack (kernels 5, 6, the 768-thread driver shells), kLdsStack (kernels 3, 0, the plain driver shell)


def chain(levels, fat=0.3):
    """The LBVH chain of test_deep_trees_use_the_stack_spill_path: three triangles per level, one leaf split off per level; rays through
    the shared corner keep one pending far child per level."""
    tris = []
    for j in range(1, levels + 1):
        for axis in range(3):
            size = 2.0 ** (-j + 1)
            p = np.full(3, fat * size); p[axis] = size
            q = p.copy(); q[(axis + 1) % 3] += 0.5 * size * fat
            r = np.full(3, -1e-4 * (1 + 0.5 * j))
            tris.append(np.concatenate([r, p, q]))
    return np.array(tris, dtype=np.float32)


def chain_cfg(rc, verts, n_inst=4, fillers=0):
    xf = np.tile(rc.scenes.IDENTITY3x4, (4, 1)).astype(np.float32)
    xf[1, [0, 5, 10]] = 0.5
    xf[2, [0, 5, 10]] = 0.25
    xf[3, [3, 7, 11]] = [0.01, 0.0, 0.0]
    xf = xf[:n_inst]
    if fillers:  # small copies on a lattice inside [1, 2]^3: a top level too large for the LDS shells, clear of the corner
        f = np.tile(rc.scenes.IDENTITY3x4, (fillers, 1)).astype(np.float32)
        k = np.arange(fillers)
        f[:, [0, 5, 10]] = 0.05
        f[:, 3], f[:, 7], f[:, 11] = 1.0 + 0.14 * (k // 49), 1.0 + 0.14 * ((k // 7) % 7), 1.0 + 0.14 * (k % 7)
        xf = np.concatenate([xf, f])
    return {"blas": [(verts, None)], "instances": [(1, xf, np.arange(len(xf), dtype=np.uint32))]}


def corner_rays(rc, n=20000, seed=12):
    g = rc.scenes.rng(seed)
    org = g.uniform(-0.2, 0.0, size=(n, 3))
    d = rc.scenes.normalize(g.uniform(0.05, 1.0, size=(n, 3)))
    return rc.scenes.make_rays(org, d)


def max_depth(o, rays):
    """The deepest stack any of `rays` has at the start of a traversal step (the initial INVALID entry and the top-level sentinel included):
    what the product's kernel 1 reports as stat2.  From the oracle's per-step record of each ray."""
    m = 1
    for i in range(len(rays)):
        dp = o.trace_events(rays[i], cap=8192)[1]
        if len(dp) > 1:
            m = max(m, int(dp[:-1].max()))
    return m


# Prefixes of chain(8) (24 triangles) under the deep test's instances.  Whole levels under its 4 instances give maximum depths 14, 17, 20,
# 23, 26; a prefix that ends inside a level, or 3 of the 4 instances, gives the values between (chosen with the oracle on the CPU;
# tests/test_gpu_stack_boundary.py asserts each through the oracle and through stat2).
BOUNDARY = {14: (4, 11), 15: (3, 13), 16: (4, 13), 17: (4, 14), 18: (3, 16),
            22: (4, 19), 23: (4, 20), 24: (3, 22), 25: (4, 22), 26: (4, 23)}
VIEWDIR, GRID = np.array([0.3, 0.2, 1.0], dtype=np.float32), 192


def grazing_rays(rc, centres, radii, seed, per_instance=400):
    """Rays aimed to pass each sphere at distance radius * f for f around 1 (the geometry), around the cull sphere (~1.1) and far."""
    g = rc.scenes.rng(seed)
    fs = np.array([0.0, 0.5, 0.9, 0.99, 0.999, 1.0, 1.001, 1.01, 1.05, 1.08, 1.09, 1.1, 1.11, 1.12, 1.15, 1.2, 1.5, 3.0])
    org, dirs = [], []
    for c, r in zip(centres, radii):
        for _ in range(per_instance):
            d = g.normal(size=3); d /= np.linalg.norm(d)
            u = np.cross(d, g.normal(size=3)); u /= np.linalg.norm(u)
            f = g.choice(fs) * (1 + g.choice([0, 1e-6, -1e-6, 1e-4, -1e-4]))
            p = np.asarray(c) + u * r * f                      # closest point of the ray to the centre
            dist = g.choice([0.0, 0.3, 3.0, 50.0, 3000.0])     # origin before / inside / far from the instance
            org.append(p - d * dist * g.choice([1, 1, 1, -1])); dirs.append(d)
    return rc.scenes.make_rays(np.array(org), np.array(dirs))


def small_cfg(rc, lattice):
    return rc.scenes.config_c3(lon=16, bands=9, lattice=lattice, pitch=1.0)  # (a dense lattice: every direction of DIRS lights it)


def single_cfg(rc):
    sc = rc.scenes
    verts = sc.fan_sphere(12, 7, centre=(0.2, -0.1, 0.3), radius=0.6)
    return {"blas": [(verts, np.arange(1, len(verts) + 1, dtype=np.uint32))], "instances": [(1, sc.IDENTITY3x4[None], np.ones(1, np.uint32))]}


def bounce_inputs(n, seed):
    rng = np.random.default_rng(seed)
    e = rng.integers(0, 1 << 24, n, dtype=np.uint32)
    e[::17] = 0
    rho = rng.integers(0, 65537, n, dtype=np.uint32)
    rho[:4] = (0, 65536, 1, 65535)
    return e, rho


U32_MAX = (1 << 32) - 1


def meta(n):
    """Metadata with gaps and duplicates for the room's n primitives: sources 5..39 share metadata 7 (row 6 of a matrix keyed by
    metadata), ten primitives have metadata 0, one has N + 50."""
    m = np.arange(1, n + 1, dtype=np.uint32)
    m[5:40] = 7
    m[100:110] = 0
    m[150] = n + 50
    return m


def distinct_x(n, salt=0, with_max=False):
    """Distinct per primitive in every byte lane and over the whole u32 range: a sum that takes another primitive's word (or a lane of
    another source or group) cannot equal the model's.  `with_max` puts 2^32 - 1 among them, so that sums of a few samples pass 2^32."""
    x = ((np.arange(1, n + 1, dtype=np.uint64) + np.uint64(salt)) * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32)
    if with_max:
        x[0] = U32_MAX
    assert len(set(x.tolist())) == n
    return x


def full_range_x(n, seed):
    x = np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint32)
    x[:3] = (U32_MAX, 0, 1 << 31)
    return x
