"""GPU parity fuzz: many small random scenes with hostile instance transforms (mirrors, shears, huge / tiny / zero scales =>
singular matrices whose inverse holds Inf / NaN), mixed BLAS sizes incl. single triangles, duplicate instances, and rays
aimed at them -- device-built arrays byte-identical to the oracle's and hit records bit-identical for every kernel."""
import numpy as np
import pytest

from gpu_kit import rc  # noqa: F401
from helpers import assert_hits_equal, build_oracle, build_product
from scene_kit import hostile_transform

pytestmark = pytest.mark.gpu


import os

N_SEEDS = int(os.environ.get("RC_FUZZ_SEEDS", "200"))  # the default -m gpu run; raise for a longer campaign (rounds 1-2: 9000 seeds clean)
FIRST_SEED = int(os.environ.get("RC_FUZZ_FIRST", "0"))  # a campaign over scenes no earlier campaign has seen: RC_FUZZ_FIRST=27000 RC_FUZZ_SEEDS=60000


@pytest.mark.parametrize("seed", range(FIRST_SEED, FIRST_SEED + N_SEEDS))
def test_random_hostile_scenes(rc, oracle, seed):
    sc = rc.scenes
    g = np.random.default_rng(1000 + seed)
    n_blas = int(g.integers(1, 5))
    blas = []
    for b in range(n_blas):
        nt = int(g.choice([1, 2, 3, 17, 200, 1500]))
        verts = sc.random_triangles(nt, 50 * seed + b, lo=-0.5, hi=0.5, edge=float(g.choice([0.05, 0.3, 1.0])))
        if nt > 3 and g.random() < 0.5:
            verts[1] = verts[0]           # exact duplicate triangle (Morton tie + t tie)
        blas.append((verts, None if g.random() < 0.5 else g.integers(1, 1000, nt).astype(np.uint32)))
    instances = []
    for b in range(n_blas):
        m = int(g.integers(1, 7))
        xf = np.stack([hostile_transform(g, int(g.integers(0, 7)) if g.random() < 0.4 else 0) for _ in range(m)])
        if m > 1 and g.random() < 0.3:
            xf[1] = xf[0]                 # duplicate instance: every hit ties exactly
        instances.append((b + 1, xf, g.integers(0, 100, m).astype(np.uint32)))
    cfg = {"blas": blas, "instances": instances}
    t, o = build_product(rc, cfg), build_oracle(oracle, cfg)
    st = t.adapt()
    assert st.nodes.tobytes() == o.tlas_nodes.tobytes(), "TLAS nodes"
    assert st.all_blas_nodes.tobytes() == o.blas_nodes.tobytes(), "BLAS nodes"
    assert st.instances.tobytes() == o.instances.tobytes(), "instance descriptors (incl. Inf/NaN inverses)"
    n = 6000
    org = g.uniform(-5, 5, size=(n, 3))
    tgt = g.uniform(-3.5, 3.5, size=(n, 3))
    d = tgt - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = sc.make_rays(org, d)
    rays["tmin"][::7] = g.uniform(-1, 1, len(rays["tmin"][::7]))
    rays["tmax"][::5] = g.uniform(0, 8, len(rays["tmax"][::5]))
    want_c, want_a = o.trace(rays, nthreads=4), o.trace(rays, mode="any", nthreads=4)
    for kern in (-1, 0, 1, 3, 5, 6):
        t.set_option("kernel", kern)
        assert_hits_equal(t.trace(rays), want_c, f"seed {seed} closest k{kern}")
        assert_hits_equal(t.trace(rays, mode="any"), want_a, f"seed {seed} any k{kern}")


@pytest.mark.parametrize("seed", range(max(4, N_SEEDS // 4)))
def test_random_bvh4_and_collision(rc, oracle, seed):
    """BVH4 collapse + closest_hit4 / any_hit4 and the collision broad phase on random inputs, bit for bit against the oracle."""
    sc = rc.scenes
    g = np.random.default_rng(5000 + seed)
    nt = int(g.choice([1, 2, 3, 4, 5, 9, 33, 257, 2000]))
    verts = sc.random_triangles(nt, 77 * seed + 1, lo=-0.5, hi=0.5, edge=float(g.choice([0.02, 0.2, 1.0])))
    if nt > 4 and g.random() < 0.4:
        verts[2] = verts[1]
    s = oracle.Scene()
    b = s.add_blas(verts)
    s.add_instance(b)
    s.build()
    blas = rc.build_blas4(verts)
    assert blas.nodes.tobytes() == s.blas4_nodes(b).tobytes()
    n = 4000
    org = g.uniform(-1.5, 1.5, size=(n, 3))
    d = sc.normalize(g.uniform(-0.6, 0.6, size=(n, 3)) - org)
    rays = sc.make_rays(org, d)
    rays["tmax"][::6] = g.uniform(0, 3, len(rays["tmax"][::6]))
    assert_hits_equal(blas.trace(rays), s.trace4(b, rays, nthreads=2), f"seed {seed} closest4")
    assert_hits_equal(blas.trace(rays, mode="any"), s.trace4(b, rays, mode="any", nthreads=2), f"seed {seed} any4")
    # collision: many instances with hostile transforms
    m = int(g.choice([1, 2, 3, 17, 300]))
    xf = np.stack([hostile_transform(g, int(g.integers(0, 7)) if g.random() < 0.3 else 0) for _ in range(m)])
    xf[:, [3, 7, 11]] *= np.float32(g.choice([0.3, 1.0, 3.0]))
    t, o = rc.TLAS(), oracle.Scene()
    t.push(verts, xf.reshape(m, 12))
    ob = o.add_blas(verts)
    for x in xf:
        o.add_instance(ob, x, 0)
    o.build()
    want, _ = o.collide_instances()
    res = rc.collide_instances(t)
    got = np.stack([res.contacts["instance_a"], res.contacts["instance_b"]], axis=1) if res.num_contacts else np.zeros((0, 2), np.uint32)
    assert np.array_equal(got, want), f"seed {seed} contacts"
